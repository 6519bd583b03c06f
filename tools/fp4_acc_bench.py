#!/usr/bin/env python3
"""MXFP4 dense accumulators (SOW_ACC_DENSE_FP4) against the bf16 accumulator they replace and the E4M3 form.

The method of tools/fp8_acc_bench.py: through the C ABI (no Python wrapper in the timed region), HIP events around every call,
3 warm-up and 24 timed calls per variant, the variants alternated call by call in one process, medians; every call reads another
copy of the weights, rotating over more than 256 MiB of them, so that the accumulator comes from HBM; the copy rate is measured
in the same process.

  (i)   T <= 32, every row of DESIGN section 4.5a:  b = sow_forward_skinny on the bf16 accumulator, q8 = on the E4M3 codes,
        q4 = on the MXFP4 codes, d4 = sow_acc_dequantize_fp4 into a scratch image followed by b on the image (what the module
        would do instead of q4); c4 = the bytes of the q4 call (0.53125 per accumulator element) at the copy rate.
  (ii)  T >= 33, forward + data gradient (sow_forward, then sow_backward_ex with SOW_BWD_DATA):  u = on the bf16 accumulator,
        q = with sow_acc_dequantize_fp4 ahead of each of the two calls; q - u is the cost of the two image passes.  deq = the
        image pass alone, GB/s of codes and scales read + image written.

  python tools/fp4_acc_bench.py [--out profiles/fp4_acc.txt] [--quick]
"""
import argparse
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from sow_amd import _lib, acc_quant  # noqa: E402
from tools import fp8_acc_bench as B8  # noqa: E402
from tools.skinny_bench import copy_rate  # noqa: E402

DEV, BF16 = B8.DEV, B8.BF16
FP4_BYTES = 0.5 + 1 / 32


class Skinny:
    """`copies` parameter sets of n layers of one shape; per set a bf16 call, an E4M3 call, an MXFP4 call and an image + bf16 call."""

    def __init__(self, T, d_in, d_out, r, n=1):
        lib = _lib.load()
        self.copies = max(2, -(-320 * 1024 * 1024 // (n * d_in * d_out * 2)) + 1)
        self.T, self.d_in, self.d_out, self.r, self.n = T, d_in, d_out, r, n
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *s, std: torch.randn(*s, device=DEV, dtype=BF16, generator=g) * std   # noqa: E731
        self.x = rnd(T, d_in, std=1.0)
        nws = max(lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, _lib.ACC_DENSE, _lib.BF16),
                  lib.sow_forward_skinny_fp8_workspace_bytes(T, d_in, d_out, r, _lib.BF16),
                  lib.sow_forward_skinny_fp4_workspace_bytes(T, d_in, d_out, r, _lib.BF16))
        assert nws > 0
        self.images = [torch.empty(d_in, d_out, device=DEV, dtype=BF16) for _ in range(n)]     # the scratch arena of variant d4
        self.fp4, self.calls = [], {"b": [], "q8": [], "q4": [], "d4": []}
        self.keep = []
        for _ in range(self.copies):
            arrs = {k: (_lib.LayerArgs * n)() for k in self.calls}
            for i in range(n):
                W = torch.randn(d_in, d_out, device=DEV, dtype=BF16, generator=g) * 0.02
                q8, e8 = acc_quant.quantize_tensor(W)
                q4, e4 = acc_quant.quantize_tensor(W, "mxfp4")
                A, Bm = rnd(d_in, r, std=0.05), rnd(r, d_out, std=0.05)
                y = torch.empty(T, d_out, device=DEV, dtype=BF16)
                ws = torch.empty(nws, device=DEV, dtype=torch.uint8)
                self.keep += [W, q8, e8, q4, e4, A, Bm, y, ws]
                self.fp4.append((q4, e4))
                for k, arr in arrs.items():
                    a = arr[i]
                    a.x, a.A, a.B, a.y = self.x.data_ptr(), A.data_ptr(), Bm.data_ptr(), y.data_ptr()
                    a.T, a.d_in, a.d_out, a.r_live, a.scale = T, d_in, d_out, r, 0.5
                    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
                    if k == "q8":
                        a.acc_down, a.acc_up, a.acc_kind = q8.data_ptr(), e8.data_ptr(), _lib.ACC_DENSE_FP8
                    elif k == "q4":
                        a.acc_down, a.acc_up, a.acc_kind = q4.data_ptr(), e4.data_ptr(), _lib.ACC_DENSE_FP4
                    else:
                        a.acc_down, a.acc_kind = (W if k == "b" else self.images[i]).data_ptr(), _lib.ACC_DENSE
            for k in self.calls:
                self.calls[k].append(arrs[k])

    def call(self, v, j):
        lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
        j %= self.copies
        if v == "d4":
            for i in range(self.n):
                q, e = self.fp4[j * self.n + i]
                _lib.check(lib.sow_acc_dequantize_fp4(q.data_ptr(), e.data_ptr(), self.d_in, self.d_out, self.images[i].data_ptr(),
                                                      self.d_out, _lib.BF16, st), "sow_acc_dequantize_fp4")
        _lib.check(lib.sow_forward_skinny(self.calls[v][j], self.n, _lib.BF16, st), v)

    def bytes(self, per_elem):
        return self.n * (self.d_in * self.d_out * per_elem + (self.d_in * self.r + self.r * self.d_out) * 2)


class Long(B8.Long):
    """tools/fp8_acc_bench.Long with the MXFP4 image pass."""

    def __init__(self, T, d_in, d_out, r=50):
        super().__init__(T, d_in, d_out, r)
        self.fp4 = [acc_quant.quantize_tensor(s[0], "mxfp4") for s in self.sets]

    def deq(self, j):
        q, e = self.fp4[j % self.copies]
        _lib.check(_lib.load().sow_acc_dequantize_fp4(q.data_ptr(), e.data_ptr(), self.d_in, self.d_out, self.image.data_ptr(), self.d_out,
                                                      _lib.BF16, torch.cuda.current_stream().cuda_stream), "sow_acc_dequantize_fp4")


def sweep(out_path, quick):
    rate = copy_rate()
    W, TI = B8.WARM, B8.TIMED
    lines = [f"# tools/fp4_acc_bench.py on {torch.cuda.get_device_name(0)}; sow_version {_lib.load().sow_version()}",
             f"# copy rate (128 MiB buffers, read + write): {rate:.0f} GB/s; times in us per call, median of {TI} (after {W} "
             f"warm-up), variants alternated, weights rotating over > 256 MiB; +- = spread of the medians of three windows of 8",
             "# (i) T <= 32: b = sow_forward_skinny, bf16 accumulator; q8 = E4M3 codes; q4 = MXFP4 codes; d4 = sow_acc_dequantize_fp4 + b on",
             "#     the image; c4 = the q4 call's bytes (0.53125 per accumulator element) at the copy rate",
             f"{'shape':>18} {'T':>3} {'r':>3} | {'b':>7} {'+-':>5} {'q8':>7} {'+-':>5} {'q4':>7} {'+-':>5} {'d4':>7} {'+-':>5} | {'c4':>6} | "
             f"{'q4/b':>5} {'q4/q8':>5} {'q4/c4':>6} {'q4/d4':>5}"]
    print("\n".join(lines), flush=True)
    shapes = [(sh, 1) for sh in (B8.SHAPES[:2] if quick else B8.SHAPES)] + ([] if quick else [((4096, 4096), 3)])
    for (d_in, d_out), n in shapes:
        for r in ((50,) if quick else B8.RANKS):
            for T in ((4, 32) if quick else B8.TS):
                s = Skinny(T, d_in, d_out, r, n)
                m = B8.measure(s, ("b", "q8", "q4", "d4"))
                c4 = s.bytes(FP4_BYTES) / rate * 1e-3
                b, q8, q4, d4 = m["b"], m["q8"], m["q4"], m["d4"]
                name = f"{'3x ' if n > 1 else ''}{d_in}->{d_out}"
                line = (f"{name:>18} {T:3d} {r:3d} | {b[0]:7.1f} {b[1]:5.1f} {q8[0]:7.1f} {q8[1]:5.1f} {q4[0]:7.1f} {q4[1]:5.1f} {d4[0]:7.1f} "
                        f"{d4[1]:5.1f} | {c4:6.1f} | {q4[0] / b[0]:5.2f} {q4[0] / q8[0]:5.2f} {q4[0] / c4:6.2f} {q4[0] / d4[0]:5.2f}")
                print(line, flush=True)
                lines.append(line)
                del s
                torch.cuda.empty_cache()
    head = ["# (ii) T >= 33, forward + data gradient, r = 50: u = bf16 accumulator; q = an MXFP4 image pass ahead of each of the two calls;",
            "#      deq = one image pass alone, GB/s of codes and scales read + image written (2.53125 bytes per element)",
            f"{'shape':>18} {'T':>6} | {'u':>8} {'+-':>6} {'q':>8} {'+-':>6} | {'q - u':>7} {'q/u':>5} | {'deq us':>7} {'GB/s':>6}"]
    print("\n".join(head), flush=True)
    lines += head
    for d_in, d_out in B8.LONG_SHAPES:
        for T in ((1024,) if quick else B8.LONG_TS):
            s = Long(T, d_in, d_out)
            m = B8.measure(s, ("u", "q", "deq"))
            u, q, dq = m["u"], m["q"], m["deq"]
            line = (f"{f'{d_in}->{d_out}':>18} {T:6d} | {u[0]:8.1f} {u[1]:6.1f} {q[0]:8.1f} {q[1]:6.1f} | {q[0] - u[0]:7.1f} {q[0] / u[0]:5.2f} | "
                    f"{dq[0]:7.1f} {(2 + FP4_BYTES) * d_in * d_out / (dq[0] * 1e-6) / 1e9:6.0f}")
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
