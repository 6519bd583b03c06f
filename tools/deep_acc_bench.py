#!/usr/bin/env python3
"""Low-rank-accumulator layers past 256 columns: the fused pass in column groups (SOW_FUSE_ACC_DEEP, chain_deep_acc.hip)
against the unflagged path it replaces (two generic GEMM launches through a [T, r_acc] intermediate, then the live chain with
beta = 1).

Per shape, r_live, r_acc and dtype, through the C ABI (no Python wrapper in the timed region), HIP events around every call:
  plain  sow_forward / sow_backward_ex(SOW_BWD_DATA) without the flag -- the parent's kernels, which the flag's existence
         does not touch (its own workspace query);
  deep   the same calls with SOW_FUSE_ACC_DEEP in the dtype and the flagged workspace.
Forward and data gradient are timed separately.  The four variants alternate call by call in one process; 3 warm-up calls,
then REPEATS windows of TIMED calls each: the figure of a variant is the median of the window medians, its spread the
distance between the largest and the smallest window median.  Every call takes the next copy of x / y / dY / dX, rotating
over more than 256 MiB per stream, so that the token rows come from HBM as they do in a training step.

"pays" is the rule ops.deep_acc_pays is derived from: the deep median below the plain median by more than the plain variant's
own spread -- for the forward, for the data gradient, and for their sum (the permission covers both directions).

  python tools/deep_acc_bench.py [--out profiles/deep_acc.txt] [--T 32768]
  python tools/deep_acc_bench.py --one D_IN D_OUT R R_ACC [--variant deep|plain]     (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from sow_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
BF16, F16 = torch.bfloat16, torch.float16
WARM, TIMED, REPEATS = 3, 24, 3
LR = _lib.ACC_LOWRANK
# (T or None = --T, d_in, d_out, r, r_acc, dtype)
CONFIGS = ([(None, di, do, 50, ra, BF16) for (di, do) in ((512, 512), (512, 1376), (1376, 512)) for ra in (250, 300, 400, 450, 500)]
           + [(None, 768, 768, 50, 600, BF16), (None, 1024, 1024, 50, 900, BF16)]
           + [(None, 512, 512, 50, 300, F16), (16384, 512, 1376, 50, 450, BF16), (None, 768, 768, 8, 504, BF16)])
# llama_60m: 8 decoder blocks of q, k, v, o (512 -> 512), gate, up (512 -> 1376), down (1376 -> 512)
LLAMA_60M = {(512, 512): 32, (512, 1376): 16, (1376, 512): 8}


class Layer:
    def __init__(self, T, d_in, d_out, r, r_acc, dtype):
        lib = _lib.load()
        self.T, self.d_in, self.d_out, self.r, self.r_acc = T, d_in, d_out, r, r_acc
        self.dt = {BF16: _lib.BF16, F16: _lib.F16}[dtype]
        per_copy = T * min(d_in, d_out) * 2
        self.copies = max(2, -(-288 * 1024 * 1024 // per_copy))     # the narrower stream alone rotates over > 256 MiB
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *s, std: (torch.randn(*s, device=DEV, dtype=torch.float32, generator=g) * std).to(dtype)   # noqa: E731
        self.A, self.B = rnd(d_in, r, std=0.05), rnd(r, d_out, std=0.05)
        self.Q, self.R = rnd(d_in, r_acc, std=0.05), rnd(r_acc, d_out, std=0.05)
        self.x = [rnd(T, d_in, std=1.0) for _ in range(self.copies)]
        self.dy = [rnd(T, d_out, std=1.0) for _ in range(self.copies)]
        self.y = [torch.empty(T, d_out, device=DEV, dtype=dtype) for _ in range(self.copies)]
        self.dx = [torch.empty(T, d_in, device=DEV, dtype=dtype) for _ in range(self.copies)]
        self.h = torch.empty(T * 64, device=DEV, dtype=dtype)
        self.dA, self.dB = torch.empty(d_in, r, device=DEV, dtype=dtype), torch.empty(r, d_out, device=DEV, dtype=dtype)
        self.ws = {}
        for flag, name in ((0, "plain"), (_lib.FUSE_ACC_DEEP, "deep")):
            nf = lib.sow_forward_workspace_bytes(T, d_in, d_out, r, r_acc, LR, self.dt | flag)
            nb = lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, LR, self.dt | flag)
            self.ws[name] = (torch.empty(nf, device=DEV, dtype=torch.uint8) if nf else None,
                             torch.empty(nb, device=DEV, dtype=torch.uint8))

    def call(self, variant, direction, j):
        lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
        dt = self.dt | (_lib.FUSE_ACC_DEEP if variant == "deep" else 0)
        fws, bws = self.ws[variant]
        k = j % self.copies
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        if direction == "fwd":
            rc = lib.sow_forward(p(self.x[k]), p(self.A), p(self.B), p(self.Q), p(self.R), None, p(self.y[k]), p(self.h), self.T,
                                 self.d_in, self.d_out, self.r, self.r_acc, LR, 0.5, dt, p(fws), 0 if fws is None else fws.numel(), st)
        else:
            rc = lib.sow_backward_ex(p(self.dy[k]), p(self.x[k]), p(self.h), p(self.A), p(self.B), p(self.Q), p(self.R),
                                     p(self.dx[k]), p(self.dA), p(self.dB), None, self.T, self.d_in, self.d_out, self.r, self.r_acc,
                                     LR, 0.5, 0.0, dt, p(bws), bws.numel(), _lib.BWD_DATA, st)
        _lib.check(rc, f"{variant} {direction}")


VARIANTS = [(v, d) for d in ("fwd", "bwd") for v in ("plain", "deep")]


def measure(L):
    """{(variant, direction): (median of the window medians, spread of the window medians)} in us."""
    for j in range(WARM):
        for v, d in VARIANTS:
            L.call(v, d, j)
    torch.cuda.synchronize()
    meds = {k: [] for k in VARIANTS}
    j = 0
    for _ in range(REPEATS):
        times = {k: [] for k in VARIANTS}
        for _ in range(TIMED):
            for k in VARIANTS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                L.call(*k, j)
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
            j += 1
        for k in VARIANTS:
            meds[k].append(statistics.median(times[k]))
    return {k: (statistics.median(m), max(m) - min(m)) for k, m in meds.items()}


def same_results(L):
    """Faster and different is not faster: y and dX of the two variants on the same inputs agree to two roundings of the
    compute dtype (the deep pass rounds once where the unflagged path rounds twice).  Returns the largest |difference| over
    the largest |value| of y and of dX."""
    out = []
    for d, bufs in (("fwd", L.y), ("bwd", L.dx)):
        L.call("plain", d, 0)
        ref = bufs[0].float().clone()
        L.call("deep", d, 0)
        out.append(float((bufs[0].float() - ref).abs().max() / ref.abs().max()))
    torch.cuda.synchronize()
    return out


def sweep(out_path, T):
    lines = [f"# tools/deep_acc_bench.py on {torch.cuda.get_device_name(0)}; sow_version {_lib.load().sow_version()}; T = {T} "
             "where a row does not say otherwise",
             f"# us per call: median of {REPEATS} window medians ({TIMED} calls each, {WARM} warm-up), +- = spread of the window "
             "medians; x / y / dY / dX rotate over > 256 MiB",
             "# pl = the unflagged call (generic GEMM pair + live chain), dp = deep pass (SOW_FUSE_ACC_DEEP); sum = forward + data "
             "gradient; pays f / b / s = the deep median is below the plain one by more than the plain spread (forward / data "
             "gradient / sum); dy / ddx = max |deep - plain| / max |plain|",
             f"{'T':>6} {'shape':>10} {'dt':>4} {'r':>3} {'r_acc':>5} {'r_pad':>5} {'LDS':>4} | {'fwd pl':>13} {'fwd dp':>13} | {'bwd pl':>13} {'bwd dp':>13} |"
             f" {'sum pl':>13} {'sum dp':>8} {'dp/pl':>6} {'pays f b s':>10} | {'dy':>7} {'ddx':>7}"]
    print("\n".join(lines), flush=True)
    saved = {}
    for Tc, d_in, d_out, r, r_acc, dtype in CONFIGS:
        Tc = Tc or T
        L = Layer(Tc, d_in, d_out, r, r_acc, dtype)
        diff = same_results(L)
        m = measure(L)
        f2, ff, b2, bf = m[("plain", "fwd")], m[("deep", "fwd")], m[("plain", "bwd")], m[("deep", "bwd")]
        s2, s2s, sf = f2[0] + b2[0], f2[1] + b2[1], ff[0] + bf[0]
        pays = (ff[0] < f2[0] - f2[1], bf[0] < b2[0] - b2[1], sf < s2 - s2s)
        cell = lambda v: f"{v[0]:8.1f}+-{v[1]:<4.1f}"   # noqa: E731
        r_pad = (r + r_acc + 63) // 64 * 64
        line = (f"{Tc:6d} {f'{d_in}->{d_out}':>10} {'bf16' if dtype == BF16 else 'f16':>4} {r:3d} {r_acc:5d} {r_pad:5d} {r_pad // 8 + 40:3d}K | "
                f"{cell(f2)} {cell(ff)} | {cell(b2)} {cell(bf)} | {cell((s2, s2s))} {sf:8.1f} {sf / s2:6.3f} "
                f"{' '.join('yes' if q else ' no' for q in pays):>10} | {diff[0]:7.1e} {diff[1]:7.1e}")
        print(line, flush=True)
        lines.append(line)
        if dtype == BF16 and r == 50 and Tc == T and (d_in, d_out) in LLAMA_60M:
            saved[(d_in, d_out, r_acc)] = (s2, sf, pays[2])
        del L
        torch.cuda.empty_cache()
    # per-step sum over the 56 layers of llama_60m of (plain - chosen path), per accumulator width of a rank-50 run
    for r_acc in sorted({k[2] for k in saved}):
        if not all((di, do, r_acc) in saved for (di, do) in LLAMA_60M):
            continue
        tot2 = sum(n * saved[(di, do, r_acc)][0] for (di, do), n in LLAMA_60M.items())
        totc = sum(n * (saved[(di, do, r_acc)][1] if saved[(di, do, r_acc)][2] else saved[(di, do, r_acc)][0])
                   for (di, do), n in LLAMA_60M.items())
        line = (f"# llama_60m, 56 layers, r_acc = {r_acc:3d}: forward + data gradient plain {tot2 / 1e3:7.2f} ms, chosen path "
                f"{totc / 1e3:7.2f} ms, saved {(tot2 - totc) / 1e3:6.2f} ms per micro-batch of {T} tokens")
        print(line, flush=True)
        lines.append(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def one(d_in, d_out, r, r_acc, variant, T):
    L = Layer(T, d_in, d_out, r, r_acc, BF16)
    for j in range(20):
        for d in ("fwd", "bwd"):
            L.call(variant, d, j)
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--T", type=int, default=32768)
    ap.add_argument("--one", nargs=4, type=int, metavar=("D_IN", "D_OUT", "R", "R_ACC"))
    ap.add_argument("--variant", default="deep", choices=("deep", "plain"))
    a = ap.parse_args()
    if a.one:
        one(*a.one, a.variant, a.T)
    else:
        sweep(a.out, a.T)
