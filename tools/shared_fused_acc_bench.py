#!/usr/bin/env python3
"""Sibling layers with low-rank accumulators on one input: the backward DATA pass through the shared-input kernel
(sow_backward_shared under SOW_FUSE_ACC, chain_shared_acc.hip) against the grouped path it replaces.

Per sibling set and r_acc, through the C ABI, HIP events around every pass:
  grouped  sow_backward_group(SOW_BWD_DATA) with the flagged dtype -- one fused pass (pack + chain_wide_acc_kernel) per sibling,
           each writing its own dX_i -- followed by the adds the module surface performs on them
           (group._SoWGroupFunction._input_grad: dX = dX_{n-1} + ... + dX_0, one torch add per sibling after the first);
  shared   sow_backward_shared(SOW_BWD_DATA) with the flagged dtype: one pack launch, one kernel, ONE dX.
The two variants alternate pass by pass in one process; 3 warm-up passes, then REPEATS windows of TIMED passes each: the
figure of a variant is the median of the window medians, its spread the distance between the largest and the smallest
window median.  Every pass takes the next copy of the dY_i and of the dX buffers, rotating over more than 256 MiB per
stream, so that the token rows come from HBM as they do in a training step.

"pays" is the rule of the module surface: the shared pass below the grouped pass by more than the grouped pass's own spread.

  python tools/shared_fused_acc_bench.py [--out profiles/shared_fused_acc.txt] [--T 32768]
  python tools/shared_fused_acc_bench.py --one qkv|gate_up R_ACC [--variant shared|grouped]     (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from sow_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
WARM, TIMED, REPEATS = 3, 24, 3
LR = _lib.ACC_LOWRANK
R = 50
SETS = {"qkv": (512, (512, 512, 512)), "gate_up": (512, (1376, 1376))}
R_ACCS = (50, 100, 200)
VARIANTS = ("grouped", "shared")


class Siblings:
    def __init__(self, T, d_in, d_outs, r, r_acc):
        lib = _lib.load()
        self.T, self.d_in, self.d_outs, self.r, self.r_acc, self.n = T, d_in, d_outs, r, r_acc, len(d_outs)
        self.dt = _lib.BF16 | _lib.FUSE_ACC
        self.copies = max(2, -(-288 * 1024 * 1024 // (T * min(d_in, *d_outs) * 2)))   # the narrowest stream rotates over > 256 MiB
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *s, std: (torch.randn(*s, device=DEV, dtype=torch.float32, generator=g) * std).to(BF16)   # noqa: E731
        self.x = rnd(T, d_in, std=1.0)        # not read by the data pass
        self.sib = []
        for d_out in d_outs:
            s = dict(A=rnd(d_in, r, std=0.05), B=rnd(r, d_out, std=0.05), Q=rnd(d_in, r_acc, std=0.05), R=rnd(r_acc, d_out, std=0.05),
                     dy=[rnd(T, d_out, std=1.0) for _ in range(self.copies)],
                     dx=[torch.empty(T, d_in, device=DEV, dtype=BF16) for _ in range(self.copies)],
                     h=torch.empty(T * 64, device=DEV, dtype=BF16), dA=torch.empty(d_in, r, device=DEV, dtype=BF16),
                     dB=torch.empty(r, d_out, device=DEV, dtype=BF16),
                     ws=torch.empty(lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, LR, self.dt), device=DEV, dtype=torch.uint8))
            self.sib.append(s)
        self.dx_shared = [torch.empty(T, d_in, device=DEV, dtype=BF16) for _ in range(self.copies)]
        self.args = {v: [self._args(v, k) for k in range(self.copies)] for v in VARIANTS}

    def _args(self, variant, k):
        arr = (_lib.LayerArgs * self.n)()
        for i, (s, d_out) in enumerate(zip(self.sib, self.d_outs)):
            dx = s["dx"][k] if variant == "grouped" else (self.dx_shared[k] if i == 0 else None)
            arr[i] = _lib.LayerArgs(x=self.x.data_ptr(), A=s["A"].data_ptr(), B=s["B"].data_ptr(), acc_down=s["Q"].data_ptr(),
                                    acc_up=s["R"].data_ptr(), bias=None, y=None, h_save=s["h"].data_ptr(), dy=s["dy"][k].data_ptr(),
                                    dx=None if dx is None else dx.data_ptr(), dA=s["dA"].data_ptr(), dB=s["dB"].data_ptr(),
                                    dbias=None, T=self.T, d_in=self.d_in, d_out=d_out, r_live=self.r, r_acc=self.r_acc,
                                    acc_kind=LR, scale=0.5, grad_beta=0.0, workspace=s["ws"].data_ptr(),
                                    workspace_bytes=s["ws"].numel())
        return arr

    def call(self, variant, j):
        """One backward data pass; returns the input gradient."""
        lib, st, k = _lib.load(), torch.cuda.current_stream().cuda_stream, j % self.copies
        if variant == "shared":
            _lib.check(lib.sow_backward_shared(self.args[variant][k], self.n, self.dt, _lib.BWD_DATA, st), "sow_backward_shared")
            return self.dx_shared[k]
        _lib.check(lib.sow_backward_group(self.args[variant][k], self.n, self.dt, _lib.BWD_DATA, st), "sow_backward_group")
        dxs = [s["dx"][k] for s in self.sib]
        dx = dxs[-1]
        for d in reversed(dxs[:-1]):     # the module surface's adds
            dx = dx + d
        return dx


def measure(S):
    """{variant: (median of the window medians, spread of the window medians)} in us."""
    for j in range(WARM):
        for v in VARIANTS:
            S.call(v, j)
    torch.cuda.synchronize()
    meds = {v: [] for v in VARIANTS}
    j = 0
    for _ in range(REPEATS):
        times = {v: [] for v in VARIANTS}
        for _ in range(TIMED):
            for v in VARIANTS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                S.call(v, j)
                e1.record()
                e1.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1e3)
            j += 1
        for v in VARIANTS:
            meds[v].append(statistics.median(times[v]))
    return {v: (statistics.median(m), max(m) - min(m)) for v, m in meds.items()}


def same_results(S):
    """Faster and different is not faster: max |shared - grouped| / max |grouped| of dX on the same inputs (the shared pass
    rounds once where the grouped path rounds per sibling and per add)."""
    ref = S.call("grouped", 0).float()
    got = S.call("shared", 0).float()
    torch.cuda.synchronize()
    return float((got - ref).abs().max() / ref.abs().max())


def sweep(out_path, T):
    lines = [f"# tools/shared_fused_acc_bench.py on {torch.cuda.get_device_name(0)}; sow_version {_lib.load().sow_version()}; bf16, "
             f"T = {T}, r = {R}",
             f"# us per backward data pass: median of {REPEATS} window medians ({TIMED} passes each, {WARM} warm-up), +- = spread of "
             "the window medians; dY_i / dX rotate over > 256 MiB",
             "# grouped = sow_backward_group(DATA, SOW_FUSE_ACC): a fused pass per sibling + the module surface's dX adds; shared = "
             "sow_backward_shared(DATA, SOW_FUSE_ACC); pays = shared below grouped by more than grouped's spread; ddx = max |shared - "
             "grouped| / max |grouped|",
             f"{'set':>8} {'shapes':>14} {'r_acc':>5} {'r_pad':>5} {'LDS KiB':>7} | {'grouped':>13} {'shared':>13} {'sh/gr':>6} {'pays':>4} | {'ddx':>7}"]
    print("\n".join(lines), flush=True)
    for name, (d_in, d_outs) in SETS.items():
        for r_acc in R_ACCS:
            S = Siblings(T, d_in, d_outs, R, r_acc)
            diff = same_results(S)
            m = measure(S)
            g, s = m["grouped"], m["shared"]
            r_pad = (R + r_acc + 63) // 64 * 64
            lds = (len(d_outs) * r_pad * 128 + max(r_pad * 128 + 8192, 24576)) // 1024
            cell = lambda v: f"{v[0]:8.1f}+-{v[1]:<4.1f}"   # noqa: E731
            line = (f"{name:>8} {f'{d_in}->{d_outs[0]} x{len(d_outs)}':>14} {r_acc:5d} {r_pad:5d} {lds:7d} | {cell(g)} {cell(s)} "
                    f"{s[0] / g[0]:6.3f} {'yes' if s[0] < g[0] - g[1] else 'no':>4} | {diff:7.1e}")
            print(line, flush=True)
            lines.append(line)
            del S
            torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def one(name, r_acc, variant, T):
    d_in, d_outs = SETS[name]
    S = Siblings(T, d_in, d_outs, R, r_acc)
    for j in range(20):
        S.call(variant, j)
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--T", type=int, default=32768)
    ap.add_argument("--one", nargs=2, metavar=("SET", "R_ACC"))
    ap.add_argument("--variant", default="shared", choices=VARIANTS)
    a = ap.parse_args()
    if a.one:
        one(a.one[0], int(a.one[1]), a.variant, a.T)
    else:
        sweep(a.out, a.T)
