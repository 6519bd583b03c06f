#!/usr/bin/env python3
"""Layers with a quantised (E4M3 / MXFP4) dense accumulator at 65 ... 1024 rows, forward and data gradient in one timed region:
the pair that reads the codes in place (sow_forward_short_codes / sow_backward_short_codes) against what such a layer runs inside
sow_amd.short_rows() without sow_amd.short_codes().

The method of tools/short_rows_bench.py: through the C ABI (no Python wrapper in the timed region), HIP events around every
call, 3 warm-up and 24 timed calls per variant, the variants alternated call by call in one process, medians; +- = the spread
(max - min) of the medians of three windows of 8.  Every call reads another copy of the codes, rotating over more than 256 MiB of
them; the copy rate is measured in the same process (128 MiB buffers, read + write bytes).

  a   the image path: sow_acc_dequantize[_fp4] into one arena buffer, the forward on the image, the image pass AGAIN, the data
      gradient on the image -- the forward and data gradient being sow_forward_short / sow_backward_short where
      ops.short_rows_pays admits (T, shape), else sow_forward (h_save) / sow_backward_ex(SOW_BWD_DATA): what the module does
  n   sow_forward_short_codes (h_save written) + sow_backward_short_codes
  c   the codes read once per direction at the copy rate (n reads them once per 64-row block)
A row is marked '+' where n is below a by more than the larger spread of the two.  The rule printed at the end -- per format and
shape the largest T up to which n wins at every measured row count below it and at every measured rank -- is what
sow_amd.acc_format.SHORT_CODES_TABLE holds.

  python tools/short_codes_bench.py [--out profiles/short_codes.txt] [--quick]
  python tools/short_codes_bench.py --one fmt T d_in d_out r variant      (variant a | n; for rocprofv3 --kernel-trace --stats)
"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.abspath(__file__)))
from skinny_bench import copy_rate  # noqa: E402
from sow_amd import _lib, ops  # noqa: E402

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SHAPES = list(ops.SHORT_ROWS_TABLE)      # the eight shapes of profiles/short_rows.txt
RANKS, TS = (8, 50), (65, 128, 256, 512, 1024)
WARM, TIMED = 3, 24
KIND = {"fp8_e4m3": _lib.ACC_DENSE_FP8, "mxfp4": _lib.ACC_DENSE_FP4}


def codes_of(fmt, d_in, d_out):
    """Copies of a random code matrix with its scales, more than 256 MiB of codes (at least two).  Random bytes are codes: the two
    E4M3 NaN codes are replaced; the scales keep every value near 2^-6."""
    per = d_in * d_out if fmt == "fp8_e4m3" else d_in * d_out // 2
    copies = max(2, -(-272 * 1024 * 1024 // per) + 1)
    g = torch.Generator(device="cuda").manual_seed(1)
    out = []
    for _ in range(copies):
        if fmt == "fp8_e4m3":
            q = torch.randint(0, 256, (d_in, d_out), device=DEV, dtype=torch.uint8, generator=g)
            q[(q & 0x7F) == 0x7F] = 0x30
            e = torch.randint(-8, -5, (d_out,), device=DEV, generator=g).to(torch.int8)
        else:
            q = torch.randint(0, 256, (d_in // 2, d_out), device=DEV, dtype=torch.uint8, generator=g)
            e = torch.randint(119, 122, (d_in // 32, d_out), device=DEV, generator=g).to(torch.uint8)
        out.append((q, e))
    return out


class Set:
    """The calls of one (format, shape, T, r): one LayerArgs per copy of the codes for either path; the image path shares ONE image."""

    def __init__(self, fmt, codes, T, r):
        lib = _lib.load()
        self.fmt, self.T, self.r, self.copies = fmt, T, r, len(codes)
        d_in, d_out = (codes[0][0].shape[0] * (2 if fmt == "mxfp4" else 1), codes[0][0].shape[1])
        self.d_in, self.d_out = d_in, d_out
        g = torch.Generator(device="cuda").manual_seed(2)
        rnd = lambda *s, std: torch.randn(*s, device=DEV, dtype=BF16, generator=g) * std   # noqa: E731
        self.x, self.dy = rnd(T, d_in, std=1.0), rnd(T, d_out, std=1.0)
        self.A, self.B, self.bias = rnd(d_in, r, std=0.05), rnd(r, d_out, std=0.05), rnd(d_out, std=0.1)
        self.y, self.dx = torch.empty(T, d_out, device=DEV, dtype=BF16), torch.empty(T, d_in, device=DEV, dtype=BF16)
        self.h = torch.empty(T * 64, device=DEV, dtype=BF16)
        self.dA, self.dB = torch.empty(d_in, r, device=DEV, dtype=BF16), torch.empty(r, d_out, device=DEV, dtype=BF16)
        self.img = torch.empty(d_in, d_out, device=DEV, dtype=BF16)
        self.short = ops.short_rows_pays(T, d_in, d_out)      # the pair the image path takes
        dt = _lib.BF16
        nws = {"a": max(lib.sow_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_DENSE, dt), lib.sow_forward_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_DENSE, dt),
                        lib.sow_short_workspace_bytes(T, d_in, d_out, r, _lib.ACC_DENSE, dt)),
               "n": lib.sow_short_codes_workspace_bytes(T, d_in, d_out, r, KIND[fmt], dt)}
        assert nws["a"] > 0 and nws["n"] > 0
        self.ws = {k: torch.empty(v, device=DEV, dtype=torch.uint8) for k, v in nws.items()}
        self.keep = codes
        self.calls = {"a": [], "n": []}
        for q, e in codes:
            for k in ("a", "n"):
                arr = (_lib.LayerArgs * 1)()
                a = arr[0]
                a.x, a.A, a.B, a.bias = self.x.data_ptr(), self.A.data_ptr(), self.B.data_ptr(), self.bias.data_ptr()
                a.acc_down, a.acc_up = (self.img.data_ptr(), None) if k == "a" else (q.data_ptr(), e.data_ptr())
                a.y, a.h_save, a.dy, a.dx = self.y.data_ptr(), self.h.data_ptr(), self.dy.data_ptr(), self.dx.data_ptr()
                a.dA, a.dB = self.dA.data_ptr(), self.dB.data_ptr()      # (not written by the data phase; the entry wants them)
                a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, _lib.ACC_DENSE if k == "a" else KIND[fmt], 0.5
                a.workspace, a.workspace_bytes = self.ws[k].data_ptr(), nws[k]
                self.calls[k].append(arr)

    def image(self, j, st):
        lib = _lib.load()
        q, e = self.keep[j % self.copies]
        fn = lib.sow_acc_dequantize if self.fmt == "fp8_e4m3" else lib.sow_acc_dequantize_fp4
        _lib.check(fn(q.data_ptr(), e.data_ptr(), self.d_in, self.d_out, self.img.data_ptr(), self.d_out, _lib.BF16, st), "image")

    def call(self, v, j):
        lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
        arr = self.calls[v][j % self.copies]
        a = arr[0]
        if v == "n":
            _lib.check(lib.sow_forward_short_codes(arr, 1, _lib.BF16, st), "sow_forward_short_codes")
            _lib.check(lib.sow_backward_short_codes(arr, 1, _lib.BF16, st), "sow_backward_short_codes")
            return
        self.image(j, st)
        if self.short:
            _lib.check(lib.sow_forward_short(arr, 1, _lib.BF16, st), "sow_forward_short")
        else:
            _lib.check(lib.sow_forward(a.x, a.A, a.B, a.acc_down, None, a.bias, a.y, a.h_save, a.T, a.d_in, a.d_out, a.r_live, 0,
                                       a.acc_kind, a.scale, _lib.BF16, a.workspace, a.workspace_bytes, st), "sow_forward")
        self.image(j, st)
        if self.short:
            _lib.check(lib.sow_backward_short(arr, 1, _lib.BF16, st), "sow_backward_short")
        else:
            _lib.check(lib.sow_backward_ex(a.dy, a.x, a.h_save, a.A, a.B, a.acc_down, None, a.dx, a.dA, a.dB, None, a.T, a.d_in, a.d_out,
                                           a.r_live, 0, a.acc_kind, a.scale, 0.0, _lib.BF16, a.workspace, a.workspace_bytes,
                                           _lib.BWD_DATA, st), "sow_backward_ex")


def measure(s, variants=("a", "n")):
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


def sweep(out_path, shapes, ranks, ts):
    rate = copy_rate()
    lines = [f"# tools/short_codes_bench.py on {torch.cuda.get_device_name(0)}; sow_version {_lib.load().sow_version()}",
             f"# copy rate (128 MiB buffers, read + write): {rate:.0f} GB/s; bf16; times in us per call, median of {TIMED} (after {WARM} "
             "warm-up), variants alternated, codes rotating over > 256 MiB; +- = spread of the medians of three windows of 8",
             "# forward + data gradient in ONE timed region.  a = image pass, forward on the image, image pass, data gradient on the image "
             "(pair = s: sow_forward_short / sow_backward_short where short_rows_pays admits the row, g: sow_forward / sow_backward_ex(DATA)); "
             "n = sow_forward_short_codes + sow_backward_short_codes; c = the codes read once per direction at the copy rate; "
             "'+' = n below a by more than the larger spread",
             f"{'format':>9} {'shape':>12} {'r':>3} {'T':>5} {'pair':>4} | {'a':>7} {'+-':>5} {'n':>7} {'+-':>5} | {'c':>6} {'a/n':>5}"]
    print("\n".join(lines), flush=True)
    wins = {}
    for fmt in KIND:
        for d_in, d_out in shapes:
            w = codes_of(fmt, d_in, d_out)
            for r in ranks:
                for T in ts:
                    s = Set(fmt, w, T, r)
                    m = measure(s)
                    c = 2 * w[0][0].numel() / rate * 1e-3
                    win = m["a"][0] - m["n"][0] > max(m["a"][1], m["n"][1])
                    wins.setdefault((fmt, d_in, d_out), {}).setdefault(T, []).append(win)
                    line = (f"{fmt:>9} {f'{d_in}->{d_out}':>12} {r:3d} {T:5d} {'s' if s.short else 'g':>4} | {m['a'][0]:7.1f} {m['a'][1]:5.1f} "
                            f"{m['n'][0]:7.1f} {m['n'][1]:5.1f} | {c:6.1f} {m['a'][0] / m['n'][0]:5.2f} {'+' if win else ''}")
                    print(line, flush=True)
                    lines.append(line)
                    del s
            del w
            torch.cuda.empty_cache()
    lines.append("# the rule these rows give (largest T up to which n wins at every measured row count and rank; 0 = never):")
    for (fmt, d_in, d_out), by_t in wins.items():
        tmax = 0
        for T in sorted(by_t):
            if not all(by_t[T]):
                break
            tmax = T
        lines.append(f"#   {fmt} {d_in}->{d_out}: T <= {tmax}")
    print("\n".join(lines[-len(wins) - 1:]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def one(fmt, T, d_in, d_out, r, variant):
    s = Set(fmt, codes_of(fmt, d_in, d_out), T, r)
    for j in range(30):
        s.call(variant, j)
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the llama-7b shapes at r = 8, T = 65 and 128 only (A/B builds)")
    ap.add_argument("--one", nargs=6, metavar=("FMT", "T", "D_IN", "D_OUT", "R", "VARIANT"))
    a = ap.parse_args()
    if a.one:
        one(a.one[0], int(a.one[1]), int(a.one[2]), int(a.one[3]), int(a.one[4]), a.one[5])
    elif a.quick:
        sweep(a.out, [(4096, 4096), (4096, 11008), (11008, 4096)], (8,), (65, 128))
    else:
        sweep(a.out, SHAPES, RANKS, TS)
