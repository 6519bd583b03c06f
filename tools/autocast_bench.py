"""What fp32 master factors under torch.autocast cost: bench.py's headline stack (llama_60m, 56 SoW layers, T = 32768,
r = 50, bf16 compute, HIP graph, device events) timed three ways in one process, alternating:

  bf16      bf16 factors (bench.py's headline step)
  mixed     fp32 factors with SOW_PARAM_F32: each forward / data-gradient call packs its factors (pack_params_kernel), the
            weight gradients are written as fp32 into the fp32 flat gradient buffer
  bf16_launches  bf16 factors plus one launch of the pack's size before every call that packs in `mixed` (a
            sow_cast_copy of an fp32 buffer holding as many elements as the group's factors): what the extra launches alone
            cost, so that mixed - bf16 splits into the launches and the rest (fp32 gradients, factors read from the packed copies)
  mixed_x   the same as mixed plus the fp32 input casts of an fp32 model under autocast: the residual stream feeds q/k/v and gate/up,
            so per decoder block two [T, hidden] inputs are cast to bf16 before the forward and two input gradients back to
            fp32 after the data gradients (sow_cast_copy); o_proj and down_proj read bf16 products and need no cast

    python tools/autocast_bench.py [--rounds 5] [--replays 20]      # prints one JSON line per variant and a summary
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/autocast_bench.py --only mixed_x --rounds 1 --replays 5
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from sow_amd import _lib, ops  # noqa: E402


def mixed_stack(shapes, T, r, device):
    """bench.Stack with fp32 factors (and an fp32 FactorBucket) over bf16 activations: every layer call flagged."""
    s = bench.Stack(shapes, T, r, torch.float32, device, "none")
    s.x = [x.to(torch.bfloat16) for x in s.x]
    s.dy = [d.to(torch.bfloat16) for d in s.dy]
    torch.cuda.empty_cache()
    s.calls = []
    for li, (d_in, d_out) in enumerate(shapes):
        ws = torch.empty(ops.workspace_bytes(T, d_in, d_out, r, 0, 0, torch.bfloat16, param_f32=True) + 256,
                         dtype=torch.uint8, device=device)
        s.calls.append(ops.LayerCall(s.x[li], s.A[li].data, s.B[li].data, scale=1.0,
                                     y=torch.empty(T, d_out, dtype=torch.bfloat16, device=device), dy2=s.dy[li],
                                     dx=torch.empty(T, d_in, dtype=torch.bfloat16, device=device),
                                     out=(s.A[li].grad, s.B[li].grad, None), grad_beta=0.0, workspace=ws, param_f32=True))
    s.groups = [ops.LayerGroup([s.calls[li] for li in ids]) for ids in s.group_layers]
    s.tn_groups = [ops.LayerGroup([s.calls[li] for li in ids]) for ids in s.tn_layers]
    return s


class InputCasts:
    """The fp32 <-> bf16 casts of an fp32 model's residual stream around `stack` (q/k/v and gate/up inputs of each block)."""

    def __init__(self, stack, device):
        nb = len(bench.BLOCK_NAMES)
        self.stack = stack
        self.layers = [blk * nb + i for blk in range(len(stack.shapes) // nb) for i in (0, 4)]     # q, gate of each block
        self.x32 = {li: stack.x[li].float() for li in self.layers}
        self.dx32 = {li: torch.empty_like(self.x32[li]) for li in self.layers}

    def step(self):
        s = self.stack
        for li in self.layers:
            ops.cast(self.x32[li], torch.bfloat16, out=s.x[li])
        s.forward_all()
        s.backward_all()
        for li in self.layers:
            ops.cast(s.calls[li].dx, torch.float32, out=self.dx32[li])


class PackSizedLaunches:
    """Wraps a LayerGroup of a bf16 stack: one fp32 -> bf16 cast of the group's factor size before its forward and before its
    data-gradient backward, where the flagged calls of `mixed` launch the pack."""

    def __init__(self, group, device):
        self.group = group
        n = sum(c.args.d_in * c.args.r_live + c.args.r_live * c.args.d_out for c in group.calls)
        self.src = torch.randn(n, device=device)
        self.dst = torch.empty(n, dtype=torch.bfloat16, device=device)

    def forward(self):
        ops.cast(self.src, torch.bfloat16, out=self.dst)
        self.group.forward()

    def backward(self, phases):
        if phases & _lib.BWD_DATA:
            ops.cast(self.src, torch.bfloat16, out=self.dst)
        self.group.backward(phases)


def capture(fn, stream):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def time_replays(g, stream, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(n):
        g.replay()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=128 * 256)
    ap.add_argument("--rank", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds (one timing of every variant per round)")
    ap.add_argument("--replays", type=int, default=20, help="graph replays per timing")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=["bf16", "bf16_launches", "mixed", "mixed_x"], default=None,
                    help="one variant (a profiler run per variant keeps the per-launch statistics apart)")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    shapes = bench.layer_shapes()
    T, r = args.tokens, args.rank
    stream = torch.cuda.Stream(device=device)
    with torch.cuda.stream(stream):
        want = lambda k: args.only in (None, k)
        plain = bench.Stack(shapes, T, r, torch.bfloat16, device, "none") if want("bf16") or want("bf16_launches") else None
        mixed = mixed_stack(shapes, T, r, device) if want("mixed") or want("mixed_x") else None
        casts = InputCasts(mixed, device) if want("mixed_x") else None
        graphs = {}
        if want("bf16"):
            graphs["bf16"] = capture(plain.step, stream)
        wrapped = []   # the wrappers own buffers the bf16_launches graph writes: they live as long as the graph is replayed
        if want("bf16_launches"):      # the same stack, its groups wrapped (the bf16 graph above is already captured)
            groups = plain.groups
            wrapped = [PackSizedLaunches(g, device) for g in groups]
            plain.groups = wrapped
            graphs["bf16_launches"] = capture(plain.step, stream)
            plain.groups = groups
        if want("mixed"):
            graphs["mixed"] = capture(mixed.step, stream)
        if want("mixed_x"):
            graphs["mixed_x"] = capture(casts.step, stream)
        for g in graphs.values():
            time_replays(g, stream, args.warmup)
        ms = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for k, g in graphs.items():
                ms[k].append(time_replays(g, stream, args.replays))
    base = statistics.median(ms["bf16"]) if "bf16" in ms else None
    steps = 2 + args.warmup + args.rounds * args.replays      # per variant, for a profiler's call counts
    for k, v in ms.items():
        med = statistics.median(v)
        print(json.dumps({"variant": k, "ms_per_step": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                          "rounds": len(v), "vs_bf16": None if base is None else round(med / base, 4), "T": T, "rank": r,
                          "layers": len(shapes), "steps_run": steps}))
    if plain is not None and mixed is not None:
        # the mixed step's weight gradients are fp32 sums of the same partials: rounded to bf16 they are the plain step's
        same = all(torch.equal(a.grad.to(torch.bfloat16), b.grad) for a, b in zip(mixed.A + mixed.B, plain.A + plain.B))
        print(json.dumps({"grads_match_bf16_step": same, "pack_launches_per_step": 2 * len(mixed.groups),
                          "cast_launches_per_step": 2 * len(casts.layers)}))


if __name__ == "__main__":
    main()
