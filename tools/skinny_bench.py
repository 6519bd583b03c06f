#!/usr/bin/env python3
"""Generation-sized layer calls (T <= 32, dense accumulator): the fused skinny forward against the path it replaces.

Per shape, T and rank, through the C ABI (no Python wrapper in the timed region), HIP events around every call, 3 warm-up
and 24 timed calls per variant, the variants alternated call by call in one process, medians:
  (a)  sow_forward with h_save = NULL (sow_forward_group for the q + k + v group) -- the parent path of the C ABI;
  (a') the same with an h_save scratch buffer, which is what ops.sow_forward passes for a dense accumulator at r <= 64;
  (b)  sow_forward_skinny;
  (c)  the floor: (d_in d_out + d_in r + r d_out) * 2 bytes at the copy rate measured here as tools/membw.py measures it
       (torch copy_ of 128 MiB buffers rotating past the Infinity Cache, read + write bytes).
Every call reads another copy of the weights, rotating over more than 256 MiB of them, so that the accumulator comes from
HBM as it does in a 224-layer generate() step, not from the Infinity Cache.  "b2b" is the same rotation issued back to back
between one pair of events, per call: the rate at which a decode loop can retire layer calls when the host keeps ahead.

  python tools/skinny_bench.py [--out profiles/skinny_forward.txt]
  python tools/skinny_bench.py --one T d_in d_out [--variant parent|skinny|both]     (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from sow_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SHAPES = [(4096, 4096), (4096, 11008), (11008, 4096), (512, 512), (512, 1376)]
TS = (1, 4, 16, 32)
RANKS = (8, 50)
WARM, TIMED = 3, 24


def copy_rate():
    """GB/s of a device copy (read + write bytes), 128 MiB buffers, 8 rotating pairs, median of 5 passes."""
    n = 128 * 1024 * 1024 // 2
    a = [torch.randn(n, device=DEV, dtype=BF16) for _ in range(8)]
    b = [torch.empty(n, device=DEV, dtype=BF16) for _ in range(8)]
    for x, y in zip(a, b):
        y.copy_(x)
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for x, y in zip(a, b):
            y.copy_(x)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 8)
    del a, b
    torch.cuda.empty_cache()
    return 2 * n * 2 / (statistics.median(ts) * 1e-3) / 1e9


class Set:
    """`copies` independent parameter sets of `n` layers of one shape (n = 3: the q + k + v group on one x)."""

    def __init__(self, T, d_in, d_out, r, n=1):
        lib = _lib.load()
        wbytes = n * d_in * d_out * 2
        self.copies = max(2, -(-320 * 1024 * 1024 // wbytes) + 1)
        self.T, self.d_in, self.d_out, self.r, self.n = T, d_in, d_out, r, n
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *s, std: torch.randn(*s, device=DEV, dtype=BF16, generator=g) * std   # noqa: E731
        self.x = rnd(T, d_in, std=1.0)
        kind, dt = _lib.ACC_DENSE, _lib.BF16
        nfw = lib.sow_forward_workspace_bytes(T, d_in, d_out, r, 0, kind, dt)
        nsk = lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, kind, dt)
        assert nsk > 0
        self.keep, self.parent, self.parent_h, self.skinny = [], [], [], []
        for _ in range(self.copies):
            arrs = [(_lib.LayerArgs * n)() for _ in range(3)]
            for i in range(n):
                W, A, B = rnd(d_in, d_out, std=0.02), rnd(d_in, r, std=0.05), rnd(r, d_out, std=0.05)
                y = torch.empty(T, d_out, device=DEV, dtype=BF16)
                h = torch.empty(T * 64, device=DEV, dtype=BF16)
                ws = torch.empty(max(nfw, nsk, 256), device=DEV, dtype=torch.uint8)
                self.keep += [W, A, B, y, h, ws]
                for k, a in enumerate(arrs):
                    a = a[i]
                    a.x, a.A, a.B, a.acc_down, a.y = self.x.data_ptr(), A.data_ptr(), B.data_ptr(), W.data_ptr(), y.data_ptr()
                    a.h_save = h.data_ptr() if k == 1 else None
                    a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, kind, 0.5
                    a.workspace, a.workspace_bytes = ws.data_ptr(), (nsk if k == 2 else nfw)
                    if k != 2 and not nfw:
                        a.workspace = None
            self.parent.append(arrs[0]), self.parent_h.append(arrs[1]), self.skinny.append(arrs[2])

    def call(self, variant, j):
        lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
        if variant == "skinny":
            rc = lib.sow_forward_skinny(self.skinny[j % self.copies], self.n, _lib.BF16, st)
        else:
            arr = (self.parent if variant == "parent" else self.parent_h)[j % self.copies]
            if self.n > 1:
                rc = lib.sow_forward_group(arr, self.n, _lib.BF16, st)
            else:
                a = arr[0]
                rc = lib.sow_forward(a.x, a.A, a.B, a.acc_down, None, None, a.y, a.h_save, a.T, a.d_in, a.d_out, a.r_live, 0,
                                     a.acc_kind, a.scale, _lib.BF16, a.workspace, a.workspace_bytes, st)
        _lib.check(rc, variant)

    def bytes(self):
        return self.n * (self.d_in * self.d_out + self.d_in * self.r + self.r * self.d_out) * 2


def measure(s, variants=("parent", "parent_h", "skinny")):
    """{variant: (median us per call, back-to-back us per call)}; the variants alternate call by call."""
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
    for v in variants:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for j in range(TIMED):
            s.call(v, j)
        e1.record()
        torch.cuda.synchronize()
        out[v] = (statistics.median(times[v]), e0.elapsed_time(e1) * 1e3 / TIMED)
    return out


def sweep(out_path):
    rate = copy_rate()
    lines = [f"# tools/skinny_bench.py on {torch.cuda.get_device_name(0)}; sow_version {_lib.load().sow_version()}",
             f"# copy rate (128 MiB buffers, read + write): {rate:.0f} GB/s; times in us per call, median of {TIMED} "
             f"(after {WARM} warm-up), weights rotating over > 256 MiB",
             "# a = sow_forward(h_save = NULL) / sow_forward_group; a' = the same with an h_save scratch; b = sow_forward_skinny;"
             " c = floor at the copy rate; b2b = back-to-back per call",
             f"{'shape':>18} {'T':>3} {'r':>3} | {'a':>8} {'a_prime':>8} {'b':>8} {'c':>7} | {'b/c':>6} {'a/b':>6} {'a_prime/b':>9} |"
             f" {'a b2b':>8} {'a_prime b2b':>11} {'b b2b':>8}"]
    print("\n".join(lines), flush=True)
    for (d_in, d_out), n in [(sh, 1) for sh in SHAPES] + ([((4096, 4096), 3)] if len(SHAPES) > 3 else []):
        for r in RANKS:
            for T in TS:
                s = Set(T, d_in, d_out, r, n)
                m = measure(s)
                c = s.bytes() / rate * 1e-3
                a, ah, b = m["parent"], m["parent_h"], m["skinny"]
                name = f"{'3x ' if n > 1 else ''}{d_in}->{d_out}"
                line = (f"{name:>18} {T:3d} {r:3d} | {a[0]:8.1f} {ah[0]:8.1f} {b[0]:8.1f} {c:7.1f} | {b[0] / c:6.2f} {a[0] / b[0]:6.2f} "
                        f"{ah[0] / b[0]:9.2f} | {a[1]:8.1f} {ah[1]:11.1f} {b[1]:8.1f}")
                print(line, flush=True)
                lines.append(line)
                del s
                torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def one(T, d_in, d_out, variant):
    s = Set(T, d_in, d_out, 50)
    for v in (("parent", "skinny") if variant == "both" else (variant,)):
        for j in range(30):
            s.call(v, j)
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the three llama-7b shapes at r = 50, T = 4 and 32 only (A/B builds)")
    ap.add_argument("--one", nargs=3, type=int, metavar=("T", "D_IN", "D_OUT"))
    ap.add_argument("--variant", default="both", choices=("parent", "skinny", "both"))
    a = ap.parse_args()
    if a.quick:
        SHAPES, TS, RANKS = SHAPES[:3], (4, 32), (50,)
    if a.one:
        one(*a.one, a.variant)
    else:
        sweep(a.out)
