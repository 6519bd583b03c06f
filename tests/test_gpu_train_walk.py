"""-m gpu: the bucket / sibling-group training path walked through event sequences (tests/train_walk_plan.py).

The kernels are held element-wise to float64 elsewhere; this file holds the HOST state between calls: the sinks' `queued` /
`pending` / workspace, the bucket's block queues, the cached reduction descriptors, the parked sibling outputs, the route
choice of SoWLinear.forward, FactorAdamW's per-group steps, accumulate()'s rebinding.  One walk is one test.

Each walk runs two deep copies of one seeded Encoder (test_gpu_bias_bucket.py):
* `net`: FactorBucket(factor_parameters(net, biases=...)).attach(net), siblings grouped as the walk says, FactorAdamW with a
  factor group and a bias group;
* `twin`: the same parameters, never attached, never grouped: plain autograd into an unattached bucket of its own -- the
  per-layer path that test_gpu_elementwise.py holds to float64.
After every event net's parameters, accumulators, gradients and optimizer state are copied into twin bit for bit, so every
event is judged on its own.

Checks per event (every bound is one of tests/numerics.py / tests/step_numerics.py, none is taken from the code under test):
* y and dX bit-identical to twin's; where the shared-input kernel admits the siblings (16-bit parameters, no accumulator,
  more than 8192 tokens) the siblings' one input gradient is held to the float64 sum of their dh A^T instead, with the bound
  of test_gpu_shared_input.py (the sum is rounded once, twin's three times);
* dA, dB, dbias bit-identical to twin's where both cut the token axis alike (_rows_plan_possible below) and the event is
  the first pass into a zeroed gradient -- twin's AccumulateGrad adds the ROUNDED gradient of a pass to the stored one, the
  bucket's grad_beta = 1 reduction adds the fp32 sum and rounds once, so an accumulation is not bit-comparable.  Everywhere
  else element-wise against float64 on the recorded x and dY of every pass since the gradient was last known: the expectation
  is the stored gradient plus the float64 gradients of the passes, the bound the sum over the passes of one output ulp (at
  the running expectation) and the pass's own terms (test_gpu_bias_bucket._check_dA_dB / _check_dbias, which are used
  unchanged for a single pass into a zeroed gradient);
* a layer that got no gradient in an event (partial_step's dropped sibling or MLP, tied_step's unused layer) holds exactly
  the gradient it held before; a dropped `query` -- the sibling that is called first -- leaves its grouped output parked, and
  the next forward reads the same static input buffer (same id, address and shape, another version) and must not get it;
* eval: every layer's output element-wise against float64 (test_gpu_elementwise.py's y bound with a hidden projection); for
  more than 32 tokens also bit-identical to the training forward on the same input (sow_amd.layer._fuse_acc,
  test_gpu_round3.py); an eval between a step's forward and backward leaves y, dX and the gradients bit-identical to the same
  step without it;
* opt_step against step_numerics.adamw_ref per segment with the test's own lr / weight decay / step counts; reset_state(0)
  zeroes the factor moments alone;
* accumulate: accumulators and new factors bit-identical to twin's (same seeded draw), every parameter and gradient of net a
  view of the flat buffers again;
* host state: one _GradSink.queue call per backward pass through an attached layer; after finalize() no sink is queued or
  pending and no block queue holds anything; two consecutive equal step(T) events reuse the reducer's descriptor tensor
  (ops.DeferredReduce's promise to graph users), a step at another T builds a new one.
"""
import copy

import pytest
import torch
from torch.utils.checkpoint import checkpoint

import test_gpu_bias_bucket as BB
import test_gpu_elementwise as E
import train_walk_plan as WP
from numerics import UNIT_ROUNDOFF, accumulation_term, bound, check_bound, fp32_floor, to64, ulp
from step_numerics import adamw_ref, check_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
U32 = UNIT_ROUNDOFF[F32]
DT = {"bf16": BF16, "f16": F16, "f32": F32, "f32-autocast": F32}
SCALE = BB.SCALE
HP = [dict(lr=1e-2, weight_decay=0.1), dict(lr=2e-3, weight_decay=0.0)]    # the factor group and the bias group
# eps = 1e-4: 16-bit moments are stored in the bucket dtype, and an f16 second moment below 6e-8 is stored as 0 -- with the
# usual 1e-8 the next step of such an element (m / eps) is in the thousands and the model overflows f16 a few events on
BETAS, EPS = (0.9, 0.999), 1e-4
PLAN = WP.plan()
WORST = {}      # check class -> (worst err / limit, where)
COUNT = {}      # check class -> number of comparisons (the bit-for-bit classes have no ratio)


def _note(cls, st=None, where=""):
    COUNT[cls] = COUNT.get(cls, 0) + 1
    if st is not None and st["worst"] >= WORST.get(cls, (-1.0, ""))[0]:
        WORST[cls] = (st["worst"], where)


# ---- the model surface of the events ------------------------------------------------------------------------------------------
def _block(side, bi, b, x, drop, out_layer):
    """Block.forward of test_gpu_bias_bucket.py with the events' variations.  The siblings read a view of x, so that a tensor
    hook on the view sees the gradient that comes from the siblings alone (the shared-input kernel's one dX)."""
    a = b.attention
    xs = x.view_as(x)
    if xs.requires_grad:
        xs.register_hook(lambda g, bi=bi: side.sib_dx.__setitem__(bi, g.detach().clone()))
    q = None if drop == "query" else a.query(xs)         # (the siblings are called in Block.forward's order)
    att = torch.sigmoid(a.key(xs))
    if q is not None:
        att = torch.tanh(q) * att
    if drop != "value":
        att = att + a.value(xs)
    x = x + a.dense(att)
    if drop == "mlp":
        return x
    return x + (out_layer or b.output)(torch.tanh(b.intermediate(x)))


def _forward(side, ev, x, autocast):
    blocks = side.model.layer
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        for bi, b in enumerate(blocks):
            drop = {("value", 0): "value", ("query", 0): "query", ("mlp", 1): "mlp"}.get((ev.drop, bi)) if ev.kind == "partial_step" else None
            out_layer = blocks[0].output if (ev.kind == "tied_step" and bi == 1) else None
            fn = lambda t, bi=bi, b=b, drop=drop, out_layer=out_layer: _block(side, bi, b, t, drop, out_layer)   # noqa: E731
            if ev.kind == "ckpt_step":
                x = checkpoint(fn, x, use_reentrant=ev.reentrant, preserve_rng_state=False)
            else:
                x = fn(x)
    return x


class Side:
    """One of the two models with its bucket, optimizer, static input buffers and the record of its layer passes."""

    def __init__(self, model, spec, attach):
        from sow_amd.dp import FactorBucket, factor_parameters
        from sow_amd.optimizer import FactorAdamW
        self.model, self.spec = model, spec
        self.layers = model.sow()
        params = factor_parameters(model, biases=spec.bucket_biases)
        self.n_fac = len(factor_parameters(model))
        self.bucket = FactorBucket(params)
        if attach:
            assert self.bucket.attach(model) == (12 if spec.bucket_biases else 0)
        groups = [dict(params=params[:self.n_fac], **HP[0])] + ([dict(params=params[self.n_fac:], **HP[1])] if spec.bucket_biases else [])
        self.opt = FactorAdamW(self.bucket, betas=BETAS, eps=EPS, param_groups=groups)
        self.rec, self.sib_dx, self.bufs = {}, {}, {}
        for name, m in self.layers:
            m.register_forward_hook(lambda mod, inp, out, name=name: self._hook(name, inp[0], out))

    def _hook(self, name, x, out):
        """One entry per pass through a layer: its input, its output and, once backward has reached it, the
        gradient of its output -- the exact dY the kernels read.  A pass that backward never reaches keeps dy = None (the
        no-grad first forward of a reentrant checkpoint, an output the loss does not depend on)."""
        e = {"x": x.detach().clone(), "y": out.detach(), "nograd": not out.requires_grad, "dy": None}
        self.rec.setdefault(name, []).append(e)
        if out.requires_grad:
            out.register_hook(lambda g, e=e: e.__setitem__("dy", None if g is None else g.detach().clone()))

    def passes(self):
        """name -> [(x, dY)] of the backward passes recorded since the record was cleared."""
        return {name: [(e["x"], e["dy"]) for e in self.rec.get(name, []) if e["dy"] is not None] for name, _ in self.layers}

    def inputs(self, role, T, fresh):
        """Static input buffers (as a training loop with static buffers keeps them): refreshed IN PLACE, so the tensor keeps
        its id, address and shape from event to event and only its version tells the contents apart."""
        key = (role, T)
        if key not in self.bufs:
            dt = DT[self.spec.dtype]
            self.bufs[key] = (torch.zeros(T, self.spec.hidden, device=DEV, dtype=dt).requires_grad_(role == "train"),
                              torch.zeros(T, self.spec.hidden, device=DEV))
        x, w = self.bufs[key]
        with torch.no_grad():
            x.copy_(fresh[0])
            w.copy_(fresh[1])
        x.grad = None
        return x, w

    def grads(self):
        """name -> (dA, dB, dbias) clones; a gradient autograd has not created yet reads as zeros."""
        g = lambda p: torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()   # noqa: E731
        return {n: (g(m.downscale_weights[0]), g(m.upscale_weights[0]), g(m.bias)) for n, m in self.layers}

    def loose_biases(self):
        return [] if self.spec.bucket_biases else [m.bias for _, m in self.layers]


def _sync(net, twin):
    """twin <- net, bit for bit: parameters, gradients, optimizer state, accumulators."""
    with torch.no_grad():
        twin.bucket.flat_param.copy_(net.bucket.flat_param)
        twin.bucket.flat_grad.copy_(net.bucket.flat_grad)
        twin.opt.exp_avg.copy_(net.opt.exp_avg)
        twin.opt.exp_avg_sq.copy_(net.opt.exp_avg_sq)
        twin.opt.group_steps, twin.opt.step_count = list(net.opt.group_steps), net.opt.step_count
        for (_, a), (_, b) in zip(net.layers, twin.layers):
            for what in ("acc_downweight", "acc_upweight"):
                getattr(b, what).data.copy_(getattr(a, what).data)
        for p, q in zip(net.loose_biases(), twin.loose_biases()):
            q.data.copy_(p.data)
            q.grad = None if p.grad is None else p.grad.detach().clone()


def _rows_plan_possible(T, cdt):
    """Whether an attached block's weight gradients can take the row-owner kernel with slab counts planned over the block
    (skinny_tn.hip tn_rows_plan, mirrored by fuzz_plan.tn_rows_plan): 16-bit compute, and 160 or more slabs of at least 512
    tokens over the block's 12 operands (x and dY of six layers) -- 12 * (T // 512) >= 160, from 7168 tokens on.  Below that
    no subset of the block can plan it either (fewer operands, the same cap per operand), and both models cut the token axis
    alike.  test_gpu_bias_bucket.ROWS_PLAN says the same of its own token counts (700, 8257, 32769)."""
    return cdt != F32 and 12 * max(T // 512, 1) >= 160


# ---- float64 references ---------------------------------------------------------------------------------------------------
def _pass_refs(m, x, dy, cdt):
    """(reference, noise) of dA, dB and dbias of one backward pass in float64 on the recorded x and dY: the references and the
    terms of test_gpu_bias_bucket._check_dA_dB / _check_dbias without their output ulp.  fp32 compute adds what
    test_gpu_elementwise._check adds there: h and dh are fp32 sums themselves (d_in / d_out terms), and where they cancel the
    error of those sums, not of their rounding, carries into the products."""
    A, B = m.downscale_weights[0].detach(), m.upscale_weights[0].detach()
    x64, dy64 = to64(x.reshape(-1, x.shape[-1]).to(cdt)), to64(dy.reshape(-1, dy.shape[-1]))
    A64, B64 = to64(A.to(cdt)), to64(B.to(cdt))
    T, r = x64.shape[0], A64.shape[1]
    u = UNIT_ROUNDOFF[cdt]
    h, dh = SCALE * (x64 @ A64), SCALE * (dy64 @ B64.t())
    xx, dydy = x64 * x64, dy64 * dy64
    dA_ref, dA_sq = x64.t() @ dh, xx.t() @ (dh * dh)
    dB_ref, dB_sq = h.t() @ dy64, (h * h).t() @ dydy
    nA = accumulation_term(dA_sq, u, 1) + fp32_floor(dA_sq, T)
    nB = accumulation_term(dB_sq, u, 1) + fp32_floor(dB_sq, T)
    if cdt == F16:
        nA = nA + E._sub_term(xx.sum(0)[:, None].expand(-1, r), cdt)
        nB = nB + E._sub_term(dydy.sum(0)[None, :].expand(r, -1), cdt)
    if cdt == F32:
        nA = nA + accumulation_term(xx.t() @ (SCALE * SCALE * (dydy @ (B64 * B64).t())), U32, B64.shape[1])
        nB = nB + accumulation_term((SCALE * SCALE * (xx @ (A64 * A64))).t() @ dydy, U32, A64.shape[0])
    return (dA_ref, nA), (dB_ref, nB), (dy64.sum(0), fp32_floor(dydy.sum(0), T))


def _check_accumulated(tag, m, passes, cdt, first, got):
    """The stored gradient `first` plus the passes, in float64; per pass one output ulp at the running expectation (the
    grad_beta = 1 reduction rounds once per pass) and the pass's own terms."""
    refs = [to64(t) for t in first]
    bnds = [torch.zeros_like(t) for t in refs]
    for x, dy in passes:
        for k, (ref, noise) in enumerate(_pass_refs(m, x, dy, cdt)):
            refs[k] = refs[k] + ref
            bnds[k] = bnds[k] + ulp(refs[k], got[k].dtype) + noise
    for k, what in enumerate(("dA", "dB", "dbias")):
        _note(f"{what} accumulated (float64)", check_bound(got[k], refs[k], bnds[k], name=f"{tag}: {what} over {len(passes)} passes"), tag)


def _check_shared_dx(tag, side, bi, cdt):
    """The one input gradient of block bi's q / k / v against the float64 sum of their dh A^T (test_gpu_shared_input.py:364-377)."""
    a = side.model.layer[bi].attention
    ref = sq = None
    n_x = 0
    passes = side.passes()
    for nm, m in (("query", a.query), ("key", a.key), ("value", a.value)):
        for _, dy in passes[f"layer.{bi}.attention.{nm}"]:
            A, B = to64(m.downscale_weights[0].detach()), to64(m.upscale_weights[0].detach())
            dh = SCALE * (to64(dy.reshape(-1, dy.shape[-1])) @ B.t())
            ref = dh @ A.t() + (0 if ref is None else ref)
            sq = (dh * dh) @ (A * A).t() + (0 if sq is None else sq)
            n_x += m.out_features + 64
    got = side.sib_dx[bi]
    st = check_bound(got.reshape(ref.shape), ref, bound(ref, got.dtype, accumulation_term(sq, UNIT_ROUNDOFF[cdt], 1), fp32_floor(sq, n_x)),
                     name=f"{tag}: shared dX of block {bi}")
    _note("shared-input dX (float64)", st, tag)


def _check_eval_y(tag, m, x, y, cdt):
    """y of a no-grad pass against float64: test_gpu_elementwise._check's bound for a projection the test cannot see (one
    hidden rounding of h, and of x Q with a low-rank accumulator), one more output ulp where an accumulator product may be
    written before the live term is added."""
    f = lambda t: to64(t.detach().to(cdt))   # noqa: E731  (fp32 parameters under autocast: rounded once by the library)
    x64 = to64(x.reshape(-1, x.shape[-1]).to(cdt))
    A, B, bias = f(m.downscale_weights[0]), f(m.upscale_weights[0]), f(m.bias)
    u = UNIT_ROUNDOFF[cdt]
    xx, BBsq = x64 * x64, B * B
    T = x64.shape[0]
    hv = SCALE * (x64 @ A)
    hh = hv * hv
    y_ref, y_sq = hv @ B + bias, hh @ BBsq
    terms = [accumulation_term(hh @ BBsq, u)]
    if cdt == F16:
        terms.append(E._sub_term(BBsq.sum(0).expand(T, -1), cdt))
    if m.acc_downweight.numel() and not m.acc_upweight.numel():
        W = f(m.acc_downweight)
        first, y_sq = x64 @ W, y_sq + xx @ (W * W)
    elif m.acc_downweight.numel():
        Q, R = f(m.acc_downweight), f(m.acc_upweight)
        t = x64 @ Q
        first, y_sq = t @ R, y_sq + xx @ (Q * Q) @ (R * R)
        terms.append(accumulation_term((t * t) @ (R * R), u))
        if cdt == F16:
            terms.append(E._sub_term((R * R).sum(0).expand(T, -1), cdt))
    else:
        first = None
    if first is not None:
        y_ref = y_ref + first
        terms.append(ulp(first, cdt))
    n_y = x64.shape[1] + 64
    st = check_bound(y.reshape(y_ref.shape), y_ref, bound(y_ref, cdt, accumulation_term(y_sq, U32, n_y), *terms), name=f"{tag}: y")
    _note("eval y (float64)" + (" skinny" if T <= 32 else ""), st, tag)


# ---- the runner ---------------------------------------------------------------------------------------------------------------
class Runner:
    def __init__(self, walk, monkeypatch):
        from sow_amd import dp, ops
        self.walk, self.spec = walk, walk.model
        s = self.spec
        self.pdt = DT[s.dtype]
        self.autocast = s.dtype == "f32-autocast"
        self.gen = torch.Generator().manual_seed(sum(map(ord, walk.id)))
        base = BB.Encoder(s.hidden, s.inter, self.pdt, s.acc, rank=s.rank, gen=self.gen)
        self.net, self.twin = Side(copy.deepcopy(base), s, True), Side(copy.deepcopy(base), s, False)
        self.attached = s.bucket_biases
        self.grouping = "ungrouped"
        self._regroup(s.grouping)
        self.kind = s.acc                         # the accumulator kind every layer holds now
        self.n_acc = 0
        self.steps = [0, 0]                       # the test's own step counts of the two param groups
        self.dirty = {n: False for n, _ in self.net.layers}     # a backward pass since the last zero_grad
        self.held, self.held_before = None, None  # passes of a step whose accumulation a micro-batch continues
        self.last_step = None                     # (signature, T, descriptor tensor) of the last plain step
        self.queue_calls, self.shared_rc = [], []
        orig_q, orig_s = dp._GradSink.queue, ops.SharedInputGroup.backward
        monkeypatch.setattr(dp._GradSink, "queue", lambda sink, *a: (self.queue_calls.append(sink), orig_q(sink, *a))[1])

        def shared_backward(grp, *a, **k):
            rc = orig_s(grp, *a, **k)
            self.shared_rc.append(rc)
            return rc

        monkeypatch.setattr(ops.SharedInputGroup, "backward", shared_backward)

    # ---- small helpers
    def cdt(self):
        return BF16 if self.autocast else self.pdt

    def _regroup(self, mode):
        from sow_amd import group_siblings, ungroup_siblings
        ungroup_siblings(self.net.model)
        if mode != "ungrouped":
            assert group_siblings(self.net.model, shared_input=(mode == "shared")) == 2
        self.grouping = mode

    def _fresh(self, T):
        h = self.spec.hidden
        return torch.randn(T, h, generator=self.gen), torch.randn(T, h, generator=self.gen)

    def _shared_admitted(self, T):
        """group.py's module docstring: bf16 / f16 parameters, no accumulator, rank <= 64, more than 8192 tokens."""
        return self.grouping == "shared" and self.pdt != F32 and self.kind == "none" and T > 8192

    def _host_state_clean(self, tag):
        b = self.net.bucket
        for name, m in self.net.layers:
            s = getattr(m, "_grad_sink", None)
            assert s is None or not (s.queued or s.pending), f"{tag}: the sink of {name} is still queued / pending after finalize()"
        assert all(not blk["queue"] for blk in b._blocks.values()) and not b._sinks_pending, f"{tag}: a block queue is not empty"

    # ---- gradient events
    def _fwd(self, side, ev, x, eval_inside=0):
        side.rec, side.sib_dx = {}, {}
        x.grad = None
        y = _forward(side, ev, x, self.autocast)
        if eval_inside:
            train_rec, side.rec = side.rec, {}
            xe, _ = side.inputs("eval", eval_inside, self._fresh(eval_inside))
            with torch.no_grad():
                _forward(side, WP.ev(eval_inside), xe, self.autocast)
            self._check_eval_record(f"{self.tag} (eval of {eval_inside} tokens inside)", side)
            side.rec = train_rec
        return y

    @staticmethod
    def _bwd(y, x, w):
        (y.float() * w).sum().backward()
        return x.grad.detach().clone()

    def grad_event(self, ev, hold):
        net, twin, T, tag, cdt = self.net, self.twin, ev.T, self.tag, self.cdt()
        fresh = self._fresh(T)
        (xn, wn), (xt, wt) = net.inputs("train", T, fresh), twin.inputs("train", T, fresh)
        if self.held is None:
            self.held, self.held_before = {n: [] for n, _ in net.layers}, net.grads()
        del self.queue_calls[:], self.shared_rc[:]
        # both forwards first: a wrong output is reported as such, before backward walks its graph
        y1, y0 = self._fwd(net, ev, xn, ev.eval_T), self._fwd(twin, ev, xt)
        assert torch.equal(y1.detach(), y0.detach()), f"{tag}: y differs from the autograd copy"
        _note("y (bit for bit)")
        dx1 = self._bwd(y1, xn, wn)
        n_queue = len(self.queue_calls)
        dx0 = self._bwd(y0, xt, wt)
        y1 = y1.detach()
        passes = net.passes()
        # ---- host state: one queue call per backward pass through an attached layer (a sibling whose output the loss does
        # not use still queues its zero dY with the group)
        want = sum(len(p) for p in passes.values()) if self.attached else 0
        if self.attached and ev.kind == "partial_step" and ev.drop in ("value", "query") and self.grouping != "ungrouped":
            want += 1
        assert n_queue == want, f"{tag}: {n_queue} _GradSink.queue calls for {want} backward passes through attached layers"
        shared = self._shared_admitted(T)
        if self.grouping == "shared":
            assert bool(self.shared_rc) and all(bool(rc) == shared for rc in self.shared_rc), \
                f"{tag}: the shared-input data gradient returned {self.shared_rc}, expected admitted = {shared}"
        # ---- input gradient
        if shared:
            for bi in (0, 1):
                _check_shared_dx(tag, net, bi, cdt)
        else:
            assert torch.equal(dx1, dx0), f"{tag}: dX differs from the autograd copy"
            _note("dX (bit for bit)")
        for n in self.held:
            self.held[n] += passes[n]
        if hold:
            return                                # a micro-batch follows: no finalize(), the gradients are judged after it
        net.bucket.finalize()
        torch.cuda.synchronize()
        self._host_state_clean(tag)
        g1, g0 = net.grads(), twin.grads()
        self._check_grads(ev, g1, g0)
        self._check_descriptors(ev)
        if ev.eval_T:
            # the same step without the eval, on the state the event started from: bit-identical y, dX and gradients
            with torch.no_grad():
                for (n, m), before in zip(net.layers, self.held_before.values()):
                    for p, b in zip((m.downscale_weights[0], m.upscale_weights[0], m.bias), before):
                        if p.grad is not None:
                            p.grad.copy_(b)
            y2 = self._fwd(net, ev, xn)
            dx2 = self._bwd(y2, xn, wn)
            net.bucket.finalize()
            torch.cuda.synchronize()
            assert torch.equal(y2, y1) and torch.equal(dx2, dx1), f"{tag}: y / dX depend on the eval between forward and backward"
            for n, g in net.grads().items():
                assert all(torch.equal(a, b) for a, b in zip(g, g1[n])), f"{tag}: gradients of {n} depend on the eval inside the step"
            _note("step with / without eval inside (bit for bit)")
        for n, p in self.held.items():
            self.dirty[n] = self.dirty[n] or bool(p)
        self.held = self.held_before = None

    def _check_grads(self, ev, g1, g0):
        tag, cdt = self.tag, self.cdt()
        for name, m in self.net.layers:
            passes, before = self.held[name], self.held_before[name]
            t = f"{tag} {name}"
            if not passes:
                assert all(torch.equal(a, b) for a, b in zip(g1[name], before)), f"{t}: no backward pass, but its gradient changed"
                _note("gradient of a layer without a pass unchanged (bit for bit)")
                continue
            single = len(passes) == 1 and not self.dirty[name]
            T = passes[0][0].reshape(-1, passes[0][0].shape[-1]).shape[0]
            if single and not _rows_plan_possible(T, cdt):
                for k, what in enumerate(("dA", "dB", "dbias")):
                    assert torch.equal(g1[name][k], g0[name][k]), f"{t}: {what} differs from the autograd copy"
                _note("dA / dB / dbias (bit for bit)")
            elif single:
                x, dy = passes[0]
                sa, sb = BB._check_dA_dB(t, m, x, dy, cdt, g1[name][0], g1[name][1])
                _note("dA row-owner plan (float64)", sa, t), _note("dB row-owner plan (float64)", sb, t)
                _note("dbias row-owner plan (float64)", BB._check_dbias(t, g1[name][2], dy, cdt), t)
            else:
                _check_accumulated(t, m, passes, cdt, before, g1[name])

    def _check_descriptors(self, ev):
        if not self.attached:
            return
        d = self.net.bucket._reducer._d_descs
        sig = (self.grouping, self.autocast, self.n_acc)
        plain = ev.kind == "step" and self.single_step
        if plain and self.last_step is not None and self.last_step[0] == sig:
            if self.last_step[1] == ev.T:
                assert d is self.last_step[2], f"{self.tag}: a second equal step({ev.T}) rebuilt the reduction descriptors"
                _note("descriptors reused by an equal step")
            else:
                assert d is not self.last_step[2], f"{self.tag}: step({ev.T}) after step({self.last_step[1]}) reused the descriptors"
                _note("descriptors rebuilt at another T")
        self.last_step = (sig, ev.T, d) if plain else None

    # ---- eval
    def _check_eval_record(self, tag, side):
        for name, m in side.layers:
            for e in side.rec.get(name, []):
                assert e["nograd"], f"{tag}: {name} built an autograd graph under no_grad"
                _check_eval_y(f"{tag} {name}", m, e["x"], e["y"], self.cdt())

    def eval_event(self, ev):
        net, tag = self.net, self.tag
        x, _ = net.inputs("eval", ev.T, self._fresh(ev.T))
        net.rec = {}
        with torch.no_grad():
            y = _forward(net, ev, x, self.autocast)
        rec = net.rec
        self._check_eval_record(tag, net)
        if ev.T > 32:
            # the training forward on the same input (no backward follows: the forward touches no sink)
            net.rec = {}
            y_train = _forward(net, ev, x.detach().clone().requires_grad_(True), self.autocast)
            for name, _ in net.layers:
                for a, c in zip(rec[name], net.rec[name]):
                    assert not c["nograd"] and torch.equal(a["y"], c["y"]), f"{tag} {name}: the no-grad output differs from the training forward"
            assert torch.equal(y, y_train.detach()), f"{tag}: the no-grad output differs from the training forward"
            _note("eval against the training forward (bit for bit)")
            del y_train
        net.rec = rec

    # ---- optimizer
    def _segments(self):
        b = self.net.bucket
        cut = b.offsets[self.net.n_fac] if self.spec.bucket_biases else b.padded_numel
        return [(0, 0, cut)] + ([(1, cut, b.padded_numel)] if self.spec.bucket_biases else [])

    def opt_event(self):
        net, twin, tag = self.net, self.twin, self.tag
        b, o = net.bucket, net.opt
        p0, g, m0, v0 = (t.detach().clone() for t in (b.flat_param, b.flat_grad, o.exp_avg, o.exp_avg_sq))
        o.step()
        twin.opt.step()
        torch.cuda.synchronize()
        for what, a, c in (("parameters", b.flat_param, twin.bucket.flat_param), ("exp_avg", o.exp_avg, twin.opt.exp_avg),
                           ("exp_avg_sq", o.exp_avg_sq, twin.opt.exp_avg_sq)):
            assert torch.equal(a, c), f"{tag}: {what} differ from the autograd copy's optimizer"
        assert torch.equal(b.flat_grad, g), f"{tag}: the optimizer step changed the gradients"
        for gi, lo, hi in self._segments():
            self.steps[gi] += 1
            refs, mags = adamw_ref(p0[lo:hi], g[lo:hi], m0[lo:hi], v0[lo:hi], lr=HP[gi]["lr"], betas=BETAS, eps=EPS,
                                   wd=HP[gi]["weight_decay"], step=self.steps[gi], grad_scale=1.0)
            out = dict(p=b.flat_param[lo:hi], m=o.exp_avg[lo:hi], v=o.exp_avg_sq[lo:hi])
            for k, st in check_step(out, refs, mags, self.pdt, o.exp_avg.dtype, f"{tag} group {gi}").items():
                _note(f"opt_step {k} (float64)", st, f"{tag} group {gi}")
        assert list(o.group_steps) == self.steps[:len(o.group_steps)], f"{tag}: group steps {o.group_steps}, expected {self.steps}"

    def reset_event(self, ev):
        net, tag = self.net, self.tag
        o = net.opt
        m0, v0 = o.exp_avg.clone(), o.exp_avg_sq.clone()
        o.reset_state(ev.group)
        self.twin.opt.reset_state(ev.group)
        torch.cuda.synchronize()
        self.steps[ev.group] = 0
        for gi, lo, hi in self._segments():
            if gi == ev.group:
                assert not o.exp_avg[lo:hi].any() and not o.exp_avg_sq[lo:hi].any(), f"{tag}: moments of group {gi} are not zero"
            else:
                assert torch.equal(o.exp_avg[lo:hi], m0[lo:hi]) and torch.equal(o.exp_avg_sq[lo:hi], v0[lo:hi]), \
                    f"{tag}: reset_state({ev.group}) touched the moments of group {gi}"
        assert list(o.group_steps) == self.steps[:len(o.group_steps)], f"{tag}: group steps {o.group_steps}, expected {self.steps}"
        _note("reset_state (exact)")

    def zero_event(self):
        for side in (self.net, self.twin):
            side.opt.zero_grad()
            for p in side.loose_biases():
                p.grad = None
        torch.cuda.synchronize()
        assert not self.net.bucket.flat_grad.any(), f"{self.tag}: zero_grad left a gradient"
        self.dirty = {n: False for n in self.dirty}

    # ---- accumulate
    def accumulate_event(self):
        import sow_amd
        net, twin, tag = self.net, self.twin, self.tag
        for side in (net, twin):
            for li, (name, m) in enumerate(side.layers):
                def draw(shape, device, dtype, seed=1000 * (self.n_acc + 1) + li):
                    g = torch.Generator().manual_seed(seed)
                    return (torch.randn(*shape, generator=g) * 0.02).to(device, dtype)
                m._fresh_gaussian = draw        # the seeded draw in place of the layer's own (as test_gpu_parity.py does)
        for name, m in net.layers:
            for what, t in (("A", m.downscale_weights[0]), ("B", m.upscale_weights[0]), ("acc_down", m.acc_downweight), ("acc_up", m.acc_upweight)):
                assert torch.isfinite(t).all(), f"{tag} {name}: {what} is not finite before accumulate() (max |.| {float(t.float().abs().max())})"
        sow_amd.accumulate(net.model)
        sow_amd.accumulate(twin.model)
        twin.bucket.rebind()                     # (accumulate() finds a bucket through the sinks; twin has none)
        if not self.attached:
            net.bucket.rebind()                  # (nor has a net whose biased layers stayed on autograd)
        torch.cuda.synchronize()
        self.n_acc += 1
        self.kind = "lowrank"
        want_r = WP.acc_after(self.spec, self.n_acc)[1] if self.spec.acc == "none" else None
        for (name, a), (_, c) in zip(net.layers, twin.layers):
            for what in ("acc_downweight", "acc_upweight"):
                p, q = getattr(a, what), getattr(c, what)
                assert p.shape == q.shape and p.numel() and torch.equal(p.data, q.data), f"{tag} {name}: {what} differs from the autograd copy's"
            if want_r is not None:
                assert a.acc_downweight.shape[1] == want_r, f"{tag} {name}: accumulator of rank {a.acc_downweight.shape[1]}, expected {want_r}"
            assert torch.equal(a.downscale_weights[0].data, c.downscale_weights[0].data), f"{tag} {name}: the new A differs"
            assert not a.upscale_weights[0].data.any() and not c.upscale_weights[0].data.any(), f"{tag} {name}: the new B is not zero"
        b = net.bucket
        es = b.flat_param.element_size()
        for p, off in zip(b.params, b.offsets):
            assert p.data.data_ptr() == b.flat_param.data_ptr() + off * es, f"{tag}: a parameter left the flat buffer"
            assert p.grad is not None and p.grad.data_ptr() == b.grad_ptr(p), f"{tag}: a gradient left the flat buffer"
            assert torch.equal(p.data.reshape(-1), b.flat_param[off:off + p.numel()])
        _note("accumulate (bit for bit)")

    # ---- the walk
    def run(self):
        evs = self.walk.events
        for i, ev in enumerate(evs):
            self.tag = f"{self.walk.id} event {i} {ev}"
            nxt = evs[i + 1].kind if i + 1 < len(evs) else None
            if ev.kind in WP.GRAD_KINDS:
                self.single_step = self.held is None and nxt != "micro"
                self.grad_event(ev, hold=(nxt == "micro"))
            elif ev.kind == "eval":
                self.eval_event(ev)
            elif ev.kind == "opt_step":
                self.opt_event()
            elif ev.kind == "reset_state":
                self.reset_event(ev)
            elif ev.kind == "zero_grad":
                self.zero_event()
            elif ev.kind == "accumulate":
                self.accumulate_event()
            elif ev.kind == "regroup":
                self._regroup(ev.mode)
            elif ev.kind == "autocast":
                self.autocast = ev.on
            else:
                raise AssertionError(f"unknown event {ev}")
            if self.held is None:
                _sync(self.net, self.twin)
        assert self.held is None


@pytest.mark.parametrize("walk", PLAN, ids=[w.id for w in PLAN])
def test_walk(walk, monkeypatch):
    Runner(walk, monkeypatch).run()


def test_zz_report_worst_ratios():
    """Prints the worst err / limit of every check class of this module's walks, and how many comparisons each class made
    (run with -s to see it)."""
    for cls in sorted(COUNT):
        w = WORST.get(cls)
        print(f"train walk {cls:58s} {COUNT[cls]:5d} checks" + ("" if w is None else f"  worst err/limit {w[0]:.3f}  ({w[1]})"))
    assert all(w[0] <= 1.0 for w in WORST.values())
