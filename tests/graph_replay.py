"""Capture one call sequence of the C ABI into a HIP graph and replay it in place (a plain helper module, like numerics.py).

include/sow_amd.h, DESIGN section 2 and INTEGRATION sections 2 / 3 promise that every call goes only to the stream it is
given, never allocates or synchronises, keeps no state besides the switch table, and is capturable into a HIP graph,
bit-identical on repetition.  `replay` holds one case to that:

  1. eager twins on the current stream: input set I1, outputs and workspaces filled with 0xFF, call -> E1; the same with
     I2 -> E2 (I2: another seed, scaled by 0.5, so that no output element repeats by accident);
  2. one eager warm-up call on a fresh side stream (first-use state), then 0xFF everywhere again;
  3. capture on that side stream with I1 loaded (torch.cuda.graph(g, stream=side), one stream, no fork or join: a linear
     chain).  Every return code is 0, and after the capture every output and workspace still holds 0xFF bytes (a gradient
     accumulated onto: its initial values): capturing ran nothing;
  4. replay 1: bit-identical to E1, guards intact;
  5. replay 2: I2 copied into the same views in place, the accumulated-onto values restored, outputs and workspaces filled
     with 0x00 (not what they held at capture): bit-identical to E2, and checked against float64 by the case's own checker;
  6. replay 3: only the accumulated-onto values restored, the workspaces as replay 2 left them: bit-identical to E2.

What this catches: a launch or memset on the null stream (it invalidates the capture, or runs during it), a decision taken
on the host from values that are only right at capture time (a pack of the factors, a plan, a constant baked into a node),
first-use state created inside a capture, a call that needs a workspace somebody refilled, a packed copy of the factors
that is not rebuilt when they change in place.

The buffers are those of test_gpu_elementwise.Arena: inputs with NaN neighbours, outputs between sentinel guards.
"""
import torch

import test_gpu_elementwise as E

DEV = "cuda"


class Rc:
    """Collects the return code of every C call of a case instead of raising: a call that fails inside a capture must let
    the `with` block end, so that the capture is closed before the case fails."""

    def __init__(self):
        self.calls = []

    def __call__(self, code, what):
        self.calls.append((what, int(code)))
        return code

    def failed(self):
        return [(w, c) for w, c in self.calls if c != 0]


def bits(t):
    if t.dtype in (torch.uint8, torch.int32, torch.int16, torch.int64):
        return t
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


class Bound:
    """The fixed buffers of one case and its two input sets.

    input(ar, (t1, t2)): a guarded view that holds t1 / t2 of input set I1 / I2.
    output(ar, key, shape, init=(t1, t2)): a guarded output compared under `key`; `init`: the values it is accumulated onto
      (or updated in place from), restored before every run.
    extra(key, tensor, (t1, t2)): an in-place operand outside the arenas (int32 counters, byte pools), restored like `init`.
    call(rc): the C calls, each return code handed to rc(code, name); launches nothing else.
    check(k, out): the float64 check of the outputs (CPU tensors by key) of a run on input set k."""

    def __init__(self, name):
        self.name = name
        self.arenas, self.slots, self.outs, self.extras, self.keep = [], [], {}, [], []
        self.call = self.check = None

    def arena(self, dtype, misalign=0):
        ar = E.Arena(dtype, misalign)
        self.arenas.append(ar)
        return ar

    def input(self, ar, pair, **kw):
        if pair is None or pair[0] is None:
            return None
        view = ar.input(pair[0], **kw)
        self.slots.append((view, pair))
        return view

    def output(self, ar, key, shape, init=None, **kw):
        if init is not None and init[0] is None:
            init = None
        view = ar.output(tuple(shape), None if init is None else init[0], **kw)
        if init is not None:
            self.slots.append((ar.outs[-1][4], init))     # the arena's own copy of the initial values
        if key is not None:
            self.outs[key] = view
        return view

    def workspace(self, ar, nbytes, key=None):
        ws = ar.workspace(nbytes)
        if key is not None and ws is not None:
            self.outs[key] = ws
        return ws

    def extra(self, key, tensor, pair):
        init = pair[0].to(tensor.device, tensor.dtype).clone()
        self.slots.append((init, pair))
        self.extras.append((tensor, init))
        if key is not None:
            self.outs[key] = tensor
        return tensor

    def load(self, k):
        for dst, pair in self.slots:
            dst.copy_(pair[k].to(dst.device, dst.dtype).reshape(dst.shape))

    # ---- what the protocol does to the buffers
    def restore_initials(self):
        for ar in self.arenas:
            for buf, off, n, view, init in ar.outs:
                if init is not None:
                    view.copy_(init)
        for t, init in self.extras:
            t.copy_(init)

    def fill(self, byte):
        for ar in self.arenas:
            ar.fill(byte)
        for t, init in self.extras:
            t.copy_(init)

    def check_guards(self, what):
        for ar in self.arenas:
            ar.check_guards(what)

    def assert_nothing_ran(self, what):
        """Every output and workspace holds all-ones bytes, every accumulated-onto operand its initial values."""
        torch.cuda.synchronize()
        for ar in self.arenas:
            for buf, off, n, view, init in ar.outs:
                if init is not None:
                    assert torch.equal(bits(view), bits(init)), f"{what}: an accumulated-onto output was written"
                elif buf.dtype == torch.uint8:
                    assert bool((buf == 0xFF).all()), f"{what}: a workspace was written"
                else:
                    assert bool((bits(view) == -1).all()), f"{what}: an output was written"
        for t, init in self.extras:
            assert torch.equal(bits(t), bits(init)), f"{what}: an in-place operand was written"

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in self.outs.items()}


def _same(got, want, what):
    for k, v in want.items():
        diff = bits(got[k]) != bits(v)
        assert not bool(diff.any()), f"{what}: {k} differs in {int(diff.sum())} of {v.numel()} elements"


def replay(b: Bound, trace=None):
    """The protocol of the module docstring on the case `b`.  `trace`: a list that receives the kernel names of the eager
    run on I1 (torch.profiler).  Returns the outputs of replay 2 on the CPU."""
    name = b.name
    rc = Rc()

    def called(what):
        bad = rc.failed()
        assert not bad, f"{name}: {what}: " + ", ".join(f"{w} returned {c}" for w, c in bad)

    # 1. eager twins on the current stream
    eager = []
    for k in (0, 1):
        b.load(k)
        b.fill(0xFF)
        if k == 0 and trace is not None:
            trace.extend(E._kernel_seq(lambda: b.call(rc)))
        else:
            b.call(rc)
        called(f"eager run on I{k + 1}")
        b.check_guards(f"{name}: eager run on I{k + 1}")
        eager.append(b.snapshot())
    assert any(not torch.equal(bits(eager[0][k]), bits(eager[1][k])) for k in eager[0]), \
        f"{name}: the two input sets give the same outputs: the case cannot tell a stale replay from a fresh one"
    # 2. warm-up on a fresh side stream
    side = torch.cuda.Stream()
    b.load(0)
    b.fill(0xFF)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b.call(rc)
    side.synchronize()
    called("warm-up on the side stream")
    b.fill(0xFF)
    torch.cuda.synchronize()
    # 3. capture: a linear chain on one stream
    graph = torch.cuda.CUDAGraph()
    err = None
    try:
        with torch.cuda.graph(graph, stream=side):
            b.call(rc)
    except Exception as e:     # torch raises at capture end when a call invalidated the capture
        err = e
    bad = rc.failed()
    assert err is None and not bad, (f"{name}: the capture failed: " + ", ".join(f"{w} returned {c}" for w, c in bad)
                                     + (f"; torch: {err}" if err is not None else ""))
    b.assert_nothing_ran(f"{name}: during the capture")
    # 4. replay 1
    graph.replay()
    out = b.snapshot()
    b.check_guards(f"{name}: replay 1")
    _same(out, eager[0], f"{name}: replay 1 against the eager run on I1")
    # 5. replay 2: new inputs in place, zeroed outputs and workspaces
    b.load(1)
    b.fill(0x00)
    torch.cuda.synchronize()
    graph.replay()
    out2 = b.snapshot()
    b.check_guards(f"{name}: replay 2")
    _same(out2, eager[1], f"{name}: replay 2 (inputs changed in place) against the eager run on I2")
    # 6. replay 3: on the leftovers of replay 2
    b.restore_initials()
    torch.cuda.synchronize()
    graph.replay()
    out3 = b.snapshot()
    b.check_guards(f"{name}: replay 3")
    _same(out3, eager[1], f"{name}: replay 3 (workspace left as replay 2 left it) against the eager run on I2")
    del graph
    res = {k: v.cpu() for k, v in out2.items()}
    if b.check is not None:
        b.check(1, res)
    return res


def has_kernel(seq, kernel):
    """Whether the trace holds exactly this kernel: demangled ("sow::chain_kernel<...>") or mangled names."""
    return any(f"sow::{kernel}" in n or f"{len(kernel)}{kernel}" in n or n.split("<")[0].split("(")[0] == kernel for n in seq)
