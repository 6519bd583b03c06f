#!/usr/bin/env python3
"""E4M3 dense accumulators (SOW_ACC_DENSE_FP8) against the bf16 accumulator they replace.

Through the C ABI (no Python wrapper in the timed region), HIP events around every call, 3 warm-up and 24 timed calls per
variant, the variants alternated call by call in one process, medians; every call reads another copy of the weights, rotating
over more than 256 MiB of them (tools/skinny_bench.py), so that the accumulator comes from HBM.

  (i)   T <= 32, every row of DESIGN section 4.5a:  b = sow_forward_skinny on the bf16 accumulator, q = the same on the E4M3
        codes, d = sow_acc_dequantize into a scratch image followed by b on the image (what the module would do instead of q);
        cb / cq = the bytes of the call (2 or 1 per accumulator element) at the copy rate measured here.
  (ii)  T >= 33, forward + data gradient (sow_forward, then sow_backward_ex with SOW_BWD_DATA):  u = on the bf16 accumulator,
        q = with sow_acc_dequantize ahead of each of the two calls (autograd keeps the codes, the backward builds the image
        again); q - u is the cost of the two image passes.  deq = the image pass alone, GB/s of codes read + image written.

  python tools/fp8_acc_bench.py [--out profiles/fp8_acc.txt] [--quick]
"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from sow_amd import _lib, acc_quant  # noqa: E402
from tools.skinny_bench import copy_rate  # noqa: E402

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SHAPES = [(4096, 4096), (4096, 11008), (11008, 4096), (512, 512), (512, 1376)]
TS = (1, 4, 16, 32)
RANKS = (8, 50)
LONG_SHAPES = [(4096, 4096), (4096, 11008)]
LONG_TS = (1024, 4096, 32768)
WARM, TIMED = 3, 24


def _weights(d_in, d_out, g):
    W = torch.randn(d_in, d_out, device=DEV, dtype=BF16, generator=g) * 0.02
    q, e = acc_quant.quantize_tensor(W)
    return W, q, e


class Skinny:
    """`copies` parameter sets of n layers of one shape; per set a bf16 call, an E4M3 call and an image + bf16 call."""

    def __init__(self, T, d_in, d_out, r, n=1):
        lib = _lib.load()
        self.copies = max(2, -(-320 * 1024 * 1024 // (n * d_in * d_out * 2)) + 1)
        self.T, self.d_in, self.d_out, self.r, self.n = T, d_in, d_out, r, n
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *s, std: torch.randn(*s, device=DEV, dtype=BF16, generator=g) * std   # noqa: E731
        self.x = rnd(T, d_in, std=1.0)
        nb = lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, _lib.ACC_DENSE, _lib.BF16)
        nq = lib.sow_forward_skinny_fp8_workspace_bytes(T, d_in, d_out, r, _lib.BF16)
        assert nb > 0 and nq > 0
        self.images = [torch.empty(d_in, d_out, device=DEV, dtype=BF16) for _ in range(n)]     # the scratch arena of variant d
        self.keep, self.calls = [], {"b": [], "q": [], "d": []}
        for _ in range(self.copies):
            arrs = {k: (_lib.LayerArgs * n)() for k in self.calls}
            for i in range(n):
                W, q, e = _weights(d_in, d_out, g)
                A, B = rnd(d_in, r, std=0.05), rnd(r, d_out, std=0.05)
                y = torch.empty(T, d_out, device=DEV, dtype=BF16)
                ws = torch.empty(max(nb, nq), device=DEV, dtype=torch.uint8)
                self.keep += [W, q, e, A, B, y, ws]
                for k, arr in arrs.items():
                    a = arr[i]
                    a.x, a.A, a.B, a.y = self.x.data_ptr(), A.data_ptr(), B.data_ptr(), y.data_ptr()
                    a.T, a.d_in, a.d_out, a.r_live, a.scale = T, d_in, d_out, r, 0.5
                    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
                    if k == "q":
                        a.acc_down, a.acc_up, a.acc_kind = q.data_ptr(), e.data_ptr(), _lib.ACC_DENSE_FP8
                    else:
                        a.acc_down, a.acc_kind = (W if k == "b" else self.images[i]).data_ptr(), _lib.ACC_DENSE
            for k in self.calls:
                self.calls[k].append(arrs[k])

    def call(self, v, j):
        lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
        j %= self.copies
        if v == "d":
            for i in range(self.n):
                q, e = self.keep[7 * (j * self.n + i) + 1], self.keep[7 * (j * self.n + i) + 2]
                _lib.check(lib.sow_acc_dequantize(q.data_ptr(), e.data_ptr(), self.d_in, self.d_out, self.images[i].data_ptr(),
                                                  self.d_out, _lib.BF16, st), "sow_acc_dequantize")
        _lib.check(lib.sow_forward_skinny(self.calls[v][j], self.n, _lib.BF16, st), v)

    def bytes(self, per_elem):
        return self.n * (self.d_in * self.d_out * per_elem + (self.d_in * self.r + self.r * self.d_out) * 2)


class Long:
    """Forward + data gradient of one layer at T >= 33 on rotating weights: u = bf16 accumulator, q = image pass + the same."""

    def __init__(self, T, d_in, d_out, r=50):
        lib = _lib.load()
        self.copies = max(2, -(-320 * 1024 * 1024 // (d_in * d_out * 2)) + 1)
        self.T, self.d_in, self.d_out, self.r = T, d_in, d_out, r
        g = torch.Generator(device="cuda").manual_seed(2)
        rnd = lambda *s, std: torch.randn(*s, device=DEV, dtype=BF16, generator=g) * std   # noqa: E731
        self.x, self.dy = rnd(T, d_in, std=1.0), rnd(T, d_out, std=1.0)
        self.y, self.dx = torch.empty(T, d_out, device=DEV, dtype=BF16), torch.empty(T, d_in, device=DEV, dtype=BF16)
        self.h = torch.empty(T * 64, device=DEV, dtype=BF16)
        self.dA, self.dB = torch.empty(d_in, r, device=DEV, dtype=BF16), torch.empty(r, d_out, device=DEV, dtype=BF16)
        self.ws = torch.empty(lib.sow_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_DENSE, _lib.BF16) + 256, device=DEV, dtype=torch.uint8)
        self.image = torch.empty(d_in, d_out, device=DEV, dtype=BF16)
        self.sets = [(*_weights(d_in, d_out, g), rnd(d_in, r, std=0.05), rnd(r, d_out, std=0.05)) for _ in range(self.copies)]

    def deq(self, j):
        _, q, e, _, _ = self.sets[j % self.copies]
        _lib.check(_lib.load().sow_acc_dequantize(q.data_ptr(), e.data_ptr(), self.d_in, self.d_out, self.image.data_ptr(), self.d_out,
                                                  _lib.BF16, torch.cuda.current_stream().cuda_stream), "sow_acc_dequantize")

    def call(self, v, j):
        lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
        if v == "deq":
            return self.deq(j)
        W, _, _, A, B = self.sets[j % self.copies]
        acc = W if v == "u" else self.image
        p = lambda t: t.data_ptr()   # noqa: E731
        if v == "q":
            self.deq(j)
        _lib.check(lib.sow_forward(p(self.x), p(A), p(B), p(acc), None, None, p(self.y), p(self.h), self.T, self.d_in, self.d_out, self.r,
                                   0, _lib.ACC_DENSE, 0.5, _lib.BF16, p(self.ws), self.ws.numel(), st), "sow_forward")
        if v == "q":
            self.deq(j)
        _lib.check(lib.sow_backward_ex(p(self.dy), p(self.x), p(self.h), p(A), p(B), p(acc), None, p(self.dx), p(self.dA), p(self.dB), None,
                                       self.T, self.d_in, self.d_out, self.r, 0, _lib.ACC_DENSE, 0.5, 0.0, _lib.BF16, p(self.ws),
                                       self.ws.numel(), _lib.BWD_DATA, st), "sow_backward_ex")


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


def sweep(out_path, quick):
    rate = copy_rate()
    lines = [f"# tools/fp8_acc_bench.py on {torch.cuda.get_device_name(0)}; sow_version {_lib.load().sow_version()}",
             f"# copy rate (128 MiB buffers, read + write): {rate:.0f} GB/s; times in us per call, median of {TIMED} (after {WARM} "
             f"warm-up), variants alternated, weights rotating over > 256 MiB; +- = spread of the medians of three windows of 8",
             "# (i) T <= 32: b = sow_forward_skinny, bf16 accumulator; q = E4M3 codes; d = sow_acc_dequantize + b on the image;",
             "#     cb / cq = the call's bytes (2 / 1 per accumulator element) at the copy rate",
             f"{'shape':>18} {'T':>3} {'r':>3} | {'b':>7} {'+-':>5} {'q':>7} {'+-':>5} {'d':>7} | {'cb':>6} {'cq':>6} | {'q/b':>5} {'q/cq':>6} {'q/d':>5}"]
    print("\n".join(lines), flush=True)
    shapes = [(sh, 1) for sh in (SHAPES[:2] if quick else SHAPES)] + ([] if quick else [((4096, 4096), 3)])
    for (d_in, d_out), n in shapes:
        for r in ((50,) if quick else RANKS):
            for T in ((4, 32) if quick else TS):
                s = Skinny(T, d_in, d_out, r, n)
                m = measure(s, ("b", "q", "d"))
                cb, cq = s.bytes(2) / rate * 1e-3, s.bytes(1) / rate * 1e-3
                b, q, d = m["b"], m["q"], m["d"]
                name = f"{'3x ' if n > 1 else ''}{d_in}->{d_out}"
                line = (f"{name:>18} {T:3d} {r:3d} | {b[0]:7.1f} {b[1]:5.1f} {q[0]:7.1f} {q[1]:5.1f} {d[0]:7.1f} | {cb:6.1f} {cq:6.1f} | "
                        f"{q[0] / b[0]:5.2f} {q[0] / cq:6.2f} {q[0] / d[0]:5.2f}")
                print(line, flush=True)
                lines.append(line)
                del s
                torch.cuda.empty_cache()
    head = ["# (ii) T >= 33, forward + data gradient, r = 50: u = bf16 accumulator; q = an image pass ahead of each of the two calls;",
            "#      deq = one image pass alone, GB/s of codes read + image written (3 bytes per element)",
            f"{'shape':>18} {'T':>6} | {'u':>8} {'+-':>6} {'q':>8} {'+-':>6} | {'q - u':>7} {'q/u':>5} | {'deq us':>7} {'GB/s':>6}"]
    print("\n".join(head), flush=True)
    lines += head
    for d_in, d_out in LONG_SHAPES:
        for T in ((1024,) if quick else LONG_TS):
            s = Long(T, d_in, d_out)
            m = measure(s, ("u", "q", "deq"))
            u, q, dq = m["u"], m["q"], m["deq"]
            line = (f"{f'{d_in}->{d_out}':>18} {T:6d} | {u[0]:8.1f} {u[1]:6.1f} {q[0]:8.1f} {q[1]:6.1f} | {q[0] - u[0]:7.1f} {q[0] / u[0]:5.2f} | "
                    f"{dq[0]:7.1f} {3 * d_in * d_out / (dq[0] * 1e-6) / 1e9:6.0f}")
            print(line, flush=True)
            lines.append(line)
            del s
            torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="two shapes at r = 50, T = 4 and 32, and T = 1024 only")
    a = ap.parse_args()
    sweep(a.out, a.quick)
