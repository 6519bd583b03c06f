#!/usr/bin/env python3
"""Decode steps of 33 ... 64 rows (dense accumulator in bf16, as E4M3 codes, as MXFP4 codes): sow_forward_skinny_rows against
what the module runs today and against two sow_forward_skinny calls on the row halves.

The method of tools/skinny_bench.py: through the C ABI (no Python wrapper in the timed region), HIP events around every call,
3 warm-up and 24 timed calls per variant, the variants alternated call by call in one process, medians; +- = the spread (max -
min) of the medians of three windows of 8.  Every call reads another copy of the weights, rotating over more than 256 MiB of
them in the format they are streamed in; the copy rate is measured in the same process (128 MiB buffers, read + write bytes).

  a   what the module runs at these row counts today: sow_forward with an h_save scratch (sow_forward_group for the q + k + v
      group); for codes the image pass (sow_acc_dequantize / _fp4 into one scratch image per layer) comes first
  b2  two sow_forward_skinny calls, rows [0, ceil(T / 2)) and the rest: what a user can do today by hand (W streamed twice)
  n   sow_forward_skinny_rows
  c   the bytes of n (accumulator in its format, scales, factors) at the copy rate
The T = 32 rows give the step this entry removes: there a = n = sow_forward_skinny (the module's path at 32 rows), b2 is empty.

  python tools/skinny_rows_bench.py [--out profiles/skinny_rows.txt] [--quick]
  python tools/skinny_rows_bench.py --one T d_in d_out fmt variant      (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.abspath(__file__)))
from skinny_bench import copy_rate  # noqa: E402
from sow_amd import _lib, acc_quant  # noqa: E402

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SHAPES = [((4096, 4096), 1), ((4096, 11008), 1), ((11008, 4096), 1), ((512, 512), 1), ((512, 1376), 1), ((4096, 4096), 3)]
TS = (32, 33, 48, 64)
RANKS = (8, 50)
FMTS = ("bf16", "fp8", "fp4")
KIND = {"bf16": _lib.ACC_DENSE, "fp8": _lib.ACC_DENSE_FP8, "fp4": _lib.ACC_DENSE_FP4}
PER_ELEM = {"bf16": 2.0, "fp8": 1.0, "fp4": 0.5}
WARM, TIMED = 3, 24


class Weights:
    """`copies` x n accumulators of one shape in one format: (acc_down, acc_up) as the streaming entry reads them."""

    def __init__(self, d_in, d_out, n, fmt):
        self.d_in, self.d_out, self.n, self.fmt = d_in, d_out, n, fmt
        per = int(n * d_in * d_out * PER_ELEM[fmt])
        self.copies = max(2, -(-320 * 1024 * 1024 // per) + 1)
        g = torch.Generator(device="cuda").manual_seed(1)
        self.sets = []
        for _ in range(self.copies * n):
            W = torch.randn(d_in, d_out, device=DEV, dtype=BF16, generator=g) * 0.02
            if fmt == "bf16":
                self.sets.append((W, None))
            else:
                self.sets.append(tuple(acc_quant.quantize_tensor(W, "mxfp4" if fmt == "fp4" else "fp8_e4m3")))
            del W
        self.images = [torch.empty(d_in, d_out, device=DEV, dtype=BF16) for _ in range(n)] if fmt != "bf16" else None

    def scale_bytes(self):
        return 0 if self.fmt == "bf16" else self.sets[0][1].numel() * self.sets[0][1].element_size()


class Set:
    """The calls of one (weights, T, r): LayerArgs per copy and variant."""

    def __init__(self, w, T, r):
        lib = _lib.load()
        self.w, self.T, self.r = w, T, r
        d_in, d_out, n, fmt = w.d_in, w.d_out, w.n, w.fmt
        g = torch.Generator(device="cuda").manual_seed(2)
        rnd = lambda *s, std: torch.randn(*s, device=DEV, dtype=BF16, generator=g) * std   # noqa: E731
        self.x = rnd(T, d_in, std=1.0)
        kind, dt = KIND[fmt], _lib.BF16
        lo = (T + 1) // 2
        self.rows = {"a": (0, T), "n": (0, T), "lo": (0, lo), "hi": (lo, T - lo)}
        old = {"bf16": lambda t: lib.sow_forward_skinny_workspace_bytes(t, d_in, d_out, r, kind, dt),
               "fp8": lambda t: lib.sow_forward_skinny_fp8_workspace_bytes(t, d_in, d_out, r, dt),
               "fp4": lambda t: lib.sow_forward_skinny_fp4_workspace_bytes(t, d_in, d_out, r, dt)}[fmt]
        nws = {"a": lib.sow_forward_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_DENSE, dt),
               "n": lib.sow_forward_skinny_rows_workspace_bytes(T, d_in, d_out, r, kind, dt), "lo": old(lo), "hi": old(T - lo) if T > lo else 0}
        assert nws["n"] > 0 and nws["lo"] > 0
        self.split = T > 32
        self.A = [rnd(d_in, r, std=0.05) for _ in range(n)]
        self.B = [rnd(r, d_out, std=0.05) for _ in range(n)]
        self.y = [torch.empty(T, d_out, device=DEV, dtype=BF16) for _ in range(n)]
        self.h = [torch.empty(T * 64, device=DEV, dtype=BF16) for _ in range(n)]
        self.ws = {k: [torch.empty(max(v, 256), device=DEV, dtype=torch.uint8) for _ in range(n)] for k, v in nws.items()}
        self.calls = {k: [] for k in self.rows}
        for j in range(w.copies):
            for k, (t0, tn) in self.rows.items():
                arr = (_lib.LayerArgs * n)()
                for i in range(n):
                    down, up = w.sets[j * n + i]
                    a = arr[i]
                    a.x, a.A, a.B = self.x.data_ptr() + t0 * d_in * 2, self.A[i].data_ptr(), self.B[i].data_ptr()
                    a.y = self.y[i].data_ptr() + t0 * d_out * 2
                    a.T, a.d_in, a.d_out, a.r_live, a.scale = tn, d_in, d_out, r, 0.5
                    a.workspace, a.workspace_bytes = self.ws[k][i].data_ptr(), nws[k]
                    if k == "a":
                        a.acc_down, a.acc_kind = (down if fmt == "bf16" else w.images[i]).data_ptr(), _lib.ACC_DENSE
                        a.h_save = self.h[i].data_ptr()
                        if not nws[k]:
                            a.workspace = None
                    else:
                        a.acc_down, a.acc_up, a.acc_kind = down.data_ptr(), None if up is None else up.data_ptr(), kind
                self.calls[k].append(arr)

    def call(self, v, j):
        lib, st, w = _lib.load(), torch.cuda.current_stream().cuda_stream, self.w
        j %= w.copies
        if v == "n" or (v == "a" and not self.split):
            _lib.check(lib.sow_forward_skinny_rows(self.calls["n"][j], w.n, _lib.BF16, st), "sow_forward_skinny_rows")
        elif v == "b2":
            _lib.check(lib.sow_forward_skinny(self.calls["lo"][j], w.n, _lib.BF16, st), "sow_forward_skinny lo")
            _lib.check(lib.sow_forward_skinny(self.calls["hi"][j], w.n, _lib.BF16, st), "sow_forward_skinny hi")
        else:
            if w.fmt != "bf16":
                deq = lib.sow_acc_dequantize if w.fmt == "fp8" else lib.sow_acc_dequantize_fp4
                for i in range(w.n):
                    q, e = w.sets[j * w.n + i]
                    _lib.check(deq(q.data_ptr(), e.data_ptr(), w.d_in, w.d_out, w.images[i].data_ptr(), w.d_out, _lib.BF16, st), "image")
            arr = self.calls["a"][j]
            if w.n > 1:
                _lib.check(lib.sow_forward_group(arr, w.n, _lib.BF16, st), "sow_forward_group")
            else:
                a = arr[0]
                _lib.check(lib.sow_forward(a.x, a.A, a.B, a.acc_down, None, None, a.y, a.h_save, a.T, a.d_in, a.d_out, a.r_live, 0,
                                           a.acc_kind, a.scale, _lib.BF16, a.workspace, a.workspace_bytes, st), "sow_forward")

    def bytes(self):
        w = self.w
        return w.n * (int(w.d_in * w.d_out * PER_ELEM[w.fmt]) + w.scale_bytes() + (w.d_in * self.r + self.r * w.d_out) * 2)


def measure(s, variants):
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


def sweep(out_path, shapes, ts, ranks, fmts):
    rate = copy_rate()
    lines = [f"# tools/skinny_rows_bench.py on {torch.cuda.get_device_name(0)}; sow_version {_lib.load().sow_version()}",
             f"# copy rate (128 MiB buffers, read + write): {rate:.0f} GB/s; times in us per call, median of {TIMED} (after {WARM} "
             "warm-up), variants alternated, weights rotating over > 256 MiB; +- = spread of the medians of three windows of 8",
             "# a = today's module path (image pass first for codes; at T = 32: sow_forward_skinny); b2 = two sow_forward_skinny "
             "calls on the row halves; n = sow_forward_skinny_rows; c = the bytes of n at the copy rate; '*' = a - n within the spread;"
             " '!' = b2 below n by more than the spread",
             f"{'shape':>18} {'fmt':>4} {'T':>3} {'r':>3} | {'a':>8} {'+-':>5} {'b2':>8} {'+-':>5} {'n':>8} {'+-':>5} {'c':>7} |"
             f" {'n/c':>5} {'a/n':>5} {'b2/n':>5}"]
    print("\n".join(lines), flush=True)
    for (d_in, d_out), n in shapes:
        for fmt in fmts:
            w = Weights(d_in, d_out, n, fmt)
            for r in ranks:
                for T in ts:
                    s = Set(w, T, r)
                    m = measure(s, ("a", "b2", "n") if T > 32 else ("a", "n"))
                    c = s.bytes() / rate * 1e-3
                    a, nn = m["a"], m["n"]
                    b2 = m.get("b2")
                    flag = ("*" if a[0] - nn[0] <= max(a[1], nn[1]) else "") + ("!" if b2 and nn[0] - b2[0] > max(b2[1], nn[1]) else "")
                    name = f"{'3x ' if n > 1 else ''}{d_in}->{d_out}"
                    b2s = f"{b2[0]:8.1f} {b2[1]:5.1f}" if b2 else f"{'-':>8} {'-':>5}"
                    line = (f"{name:>18} {fmt:>4} {T:3d} {r:3d} | {a[0]:8.1f} {a[1]:5.1f} {b2s} {nn[0]:8.1f} {nn[1]:5.1f} {c:7.1f} |"
                            f" {nn[0] / c:5.2f} {a[0] / nn[0]:5.2f} {(b2[0] / nn[0] if b2 else 0):5.2f} {flag}")
                    print(line, flush=True)
                    lines.append(line)
                    del s
            del w
            torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def one(T, d_in, d_out, fmt, variant):
    s = Set(Weights(d_in, d_out, 1, fmt), T, 50)
    for j in range(30):
        s.call(variant, j)
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the three llama-7b shapes at r = 50, T = 33 and 64 only (A/B builds)")
    ap.add_argument("--one", nargs=5, metavar=("T", "D_IN", "D_OUT", "FMT", "VARIANT"))
    a = ap.parse_args()
    if a.one:
        one(int(a.one[0]), int(a.one[1]), int(a.one[2]), a.one[3], a.one[4])
    elif a.quick:
        sweep(a.out, SHAPES[:3], (33, 64), (50,), FMTS)
    else:
        sweep(a.out, SHAPES, TS, RANKS, FMTS)
