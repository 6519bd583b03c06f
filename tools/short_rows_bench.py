#!/usr/bin/env python3
"""Dense-accumulator layers of 65 ... 1024 rows, forward and data gradient: sow_forward_short / sow_backward_short against the
path the same calls take today (sow_forward with h_save, then the SOW_BWD_DATA phase of sow_backward_ex).

The method of tools/skinny_rows_bench.py: through the C ABI (no Python wrapper in the timed region), HIP events around every
call, 3 warm-up and 24 timed calls per variant, the variants alternated call by call in one process, medians; +- = the spread
(max - min) of the medians of three windows of 8.  Every call reads another copy of the accumulator, rotating over more than
256 MiB of them; the copy rate is measured in the same process (128 MiB buffers, read + write bytes).

  a   today's path through the same entry points: sow_forward (h_save written), sow_backward_ex(SOW_BWD_DATA)
  n   the new pair: sow_forward_short (h_save written), sow_backward_short
  f / d / s   forward alone, data gradient alone, both in one timed region
  c   the accumulator's bytes, read once per direction, at the copy rate (n reads them once per 64-row block)
A row is marked '+' where n's sum is below a's by more than the larger spread of the two: the rows sow_amd.ops.short_rows_pays admits.

  python tools/short_rows_bench.py [--out profiles/short_rows.txt] [--quick]
  python tools/short_rows_bench.py --one T d_in d_out r variant      (variant a | n; for rocprofv3 --kernel-trace --stats)
"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.abspath(__file__)))
from skinny_bench import copy_rate  # noqa: E402
from sow_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
# (model, shapes, ranks, row counts)
SWEEP = [("RoBERTa-base", [(768, 768), (768, 3072), (3072, 768)], (8,), (128, 256, 512, 1024)),
         ("llama-7b", [(4096, 4096), (4096, 11008), (11008, 4096)], (8, 50), (65, 128, 256, 512, 1024)),
         ("llama_60m", [(512, 512), (512, 1376)], (50,), (256, 1024))]
WARM, TIMED = 3, 24
VARIANTS = ("af", "nf", "ad", "nd", "as", "ns")


class Set:
    """The calls of one (shape, T, r): one LayerArgs per copy of the accumulator; both paths share every buffer but the workspace."""

    def __init__(self, weights, T, r):
        lib = _lib.load()
        self.T, self.r, self.copies = T, r, len(weights)
        d_in, d_out = weights[0].shape
        self.d_in, self.d_out = d_in, d_out
        g = torch.Generator(device="cuda").manual_seed(2)
        rnd = lambda *s, std: torch.randn(*s, device=DEV, dtype=BF16, generator=g) * std   # noqa: E731
        self.x, self.dy = rnd(T, d_in, std=1.0), rnd(T, d_out, std=1.0)
        self.A, self.B, self.bias = rnd(d_in, r, std=0.05), rnd(r, d_out, std=0.05), rnd(d_out, std=0.1)
        self.y, self.dx = torch.empty(T, d_out, device=DEV, dtype=BF16), torch.empty(T, d_in, device=DEV, dtype=BF16)
        self.h = torch.empty(T * 64, device=DEV, dtype=BF16)
        self.dA, self.dB = torch.empty(d_in, r, device=DEV, dtype=BF16), torch.empty(r, d_out, device=DEV, dtype=BF16)
        dt = _lib.BF16
        nws = {"a": max(lib.sow_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_DENSE, dt), lib.sow_forward_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_DENSE, dt)),
               "n": lib.sow_short_workspace_bytes(T, d_in, d_out, r, _lib.ACC_DENSE, dt)}
        assert nws["a"] > 0 and nws["n"] > 0
        self.ws = {k: torch.empty(v, device=DEV, dtype=torch.uint8) for k, v in nws.items()}
        self.keep = weights
        self.calls = {"a": [], "n": []}
        for W in weights:
            for k in ("a", "n"):
                arr = (_lib.LayerArgs * 1)()
                a = arr[0]
                a.x, a.A, a.B, a.acc_down, a.bias = self.x.data_ptr(), self.A.data_ptr(), self.B.data_ptr(), W.data_ptr(), self.bias.data_ptr()
                a.y, a.h_save, a.dy, a.dx = self.y.data_ptr(), self.h.data_ptr(), self.dy.data_ptr(), self.dx.data_ptr()
                a.dA, a.dB = self.dA.data_ptr(), self.dB.data_ptr()      # (not written by the data phase; the entry wants them)
                a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, _lib.ACC_DENSE, 0.5
                a.workspace, a.workspace_bytes = self.ws[k].data_ptr(), nws[k]
                self.calls[k].append(arr)

    def call(self, v, j):
        lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
        arr = self.calls[v[0]][j % self.copies]
        a = arr[0]
        if v[1] in "fs":
            if v[0] == "n":
                _lib.check(lib.sow_forward_short(arr, 1, _lib.BF16, st), "sow_forward_short")
            else:
                _lib.check(lib.sow_forward(a.x, a.A, a.B, a.acc_down, None, a.bias, a.y, a.h_save, a.T, a.d_in, a.d_out, a.r_live, 0,
                                           a.acc_kind, a.scale, _lib.BF16, a.workspace, a.workspace_bytes, st), "sow_forward")
        if v[1] in "ds":
            if v[0] == "n":
                _lib.check(lib.sow_backward_short(arr, 1, _lib.BF16, st), "sow_backward_short")
            else:
                _lib.check(lib.sow_backward_ex(a.dy, a.x, a.h_save, a.A, a.B, a.acc_down, None, a.dx, a.dA, a.dB, None, a.T, a.d_in, a.d_out,
                                               a.r_live, 0, a.acc_kind, a.scale, 0.0, _lib.BF16, a.workspace, a.workspace_bytes,
                                               _lib.BWD_DATA, st), "sow_backward_ex")


def measure(s, variants=VARIANTS):
    """{variant: (median us per call, spread = max - min of the medians of three windows of 8)}; variants alternate call by call."""
    for j in range(WARM):
        for v in variants:
            s.call(v, j)
    torch.cuda.synchronize()
    times = {v: [] for v in variants}
    for j in range(TIMED):
        for v in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.call(v, j)
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1) * 1e3)
    out = {}
    for v, t in times.items():
        w = [statistics.median(t[i:i + 8]) for i in range(0, TIMED, 8)]
        out[v] = (statistics.median(t), max(w) - min(w))
    return out


def weights_of(d_in, d_out):
    copies = max(2, -(-320 * 1024 * 1024 // (d_in * d_out * 2)) + 1)
    g = torch.Generator(device="cuda").manual_seed(1)
    return [torch.randn(d_in, d_out, device=DEV, dtype=BF16, generator=g) * 0.02 for _ in range(copies)]


def sweep(out_path, plan):
    rate = copy_rate()
    lines = [f"# tools/short_rows_bench.py on {torch.cuda.get_device_name(0)}; sow_version {_lib.load().sow_version()}",
             f"# copy rate (128 MiB buffers, read + write): {rate:.0f} GB/s; bf16; times in us per call, median of {TIMED} (after {WARM} "
             "warm-up), variants alternated, accumulators rotating over > 256 MiB; +- = spread of the medians of three windows of 8",
             "# a = sow_forward (h_save) / sow_backward_ex(SOW_BWD_DATA); n = sow_forward_short (h_save) / sow_backward_short; f = forward, "
             "d = data gradient, s = both in one timed region; c = the accumulator read once per direction at the copy rate; "
             "'+' = n's sum below a's by more than the larger spread",
             f"{'model':>12} {'shape':>12} {'r':>3} {'T':>5} | {'a f':>7} {'+-':>5} {'n f':>7} {'+-':>5} | {'a d':>7} {'+-':>5} {'n d':>7} {'+-':>5} |"
             f" {'a s':>7} {'+-':>5} {'n s':>7} {'+-':>5} | {'c':>6} {'a/n':>5}"]
    print("\n".join(lines), flush=True)
    wins = {}
    for model, shapes, ranks, ts in plan:
        for d_in, d_out in shapes:
            w = weights_of(d_in, d_out)
            for r in ranks:
                for T in ts:
                    s = Set(w, T, r)
                    m = measure(s)
                    c = 2 * d_in * d_out * 2 / rate * 1e-3
                    win = m["as"][0] - m["ns"][0] > max(m["as"][1], m["ns"][1])
                    wins.setdefault((d_in, d_out), {}).setdefault(T, []).append(win)
                    cols = " | ".join(" ".join(f"{m[v][0]:7.1f} {m[v][1]:5.1f}" for v in pair) for pair in (("af", "nf"), ("ad", "nd"), ("as", "ns")))
                    line = (f"{model:>12} {f'{d_in}->{d_out}':>12} {r:3d} {T:5d} | {cols} | {c:6.1f} {m['as'][0] / m['ns'][0]:5.2f} "
                            f"{'+' if win else ''}")
                    print(line, flush=True)
                    lines.append(line)
                    del s
            del w
            torch.cuda.empty_cache()
    lines.append("# the rule these rows give (largest T up to which n wins at every measured row count and rank; 0 = never):")
    for (d_in, d_out), by_t in wins.items():
        tmax = 0
        for T in sorted(by_t):
            if not all(by_t[T]):
                break
            tmax = T
        lines.append(f"#   {d_in}->{d_out}: T <= {tmax}")
    print("\n".join(lines[-len(wins) - 1:]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def one(T, d_in, d_out, r, variant):
    s = Set(weights_of(d_in, d_out), T, r)
    for j in range(30):
        s.call(variant + "s", j)
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="768->768 and 4096->4096 at r = 8, T = 128 and 1024 only (A/B builds)")
    ap.add_argument("--one", nargs=5, metavar=("T", "D_IN", "D_OUT", "R", "VARIANT"))
    a = ap.parse_args()
    if a.one:
        one(int(a.one[0]), int(a.one[1]), int(a.one[2]), int(a.one[3]), a.one[4])
    elif a.quick:
        sweep(a.out, [("RoBERTa-base", [(768, 768)], (8,), (128, 1024)), ("llama-7b", [(4096, 4096)], (8,), (128, 1024))])
    else:
        sweep(a.out, SWEEP)
