#!/usr/bin/env python3
"""fp32 master factors over a bf16 accumulator read in place (SOW_PARAM_F32 | SOW_ACC_NATIVE) against the two forms it sits
between: everything bf16, and SOW_PARAM_F32 with an fp32 accumulator that every call rounds into the workspace again.

The method of tools/fp8_acc_bench.py: through the C ABI (no Python wrapper in the timed region), HIP events around every call,
3 warm-up and 24 timed calls per variant, the variants alternated call by call in one process, medians and the spread of the
medians of three windows of 8; every call reads another copy of the weights, rotating over more than 256 MiB of them, and the
copy rate is measured in the same process (tools/skinny_bench.py).

  (i)   forward + data gradient of one layer (sow_forward, then sow_backward_ex with SOW_BWD_DATA), r = 8:
          a = all bf16;  b = SOW_PARAM_F32, fp32 accumulator;  c = SOW_PARAM_F32 | SOW_ACC_NATIVE, bf16 accumulator.
        b - c against the accumulator pack (4 bytes read + 2 written per element) of the two calls at the copy rate; c - a against
        the pack of A and B alone.
  (ii)  sow_forward_skinny, 4096 -> 4096: h = bf16 factors, f = fp32 factors (the pair of flags), for a bf16, an E4M3 and an
        MXFP4 accumulator.  A row whose |f - h| exceeds the larger spread of the two is marked, and the kernel times of both
        variants (torch.profiler, mean of 8 calls) say which phase holds the difference.

  python tools/acc_native_bench.py [--out profiles/acc_native.txt] [--quick]
"""
import argparse
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from sow_amd import _lib, acc_quant  # noqa: E402
from tools.fp8_acc_bench import TIMED, WARM, measure  # noqa: E402
from tools.skinny_bench import copy_rate  # noqa: E402

DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
PF, NATIVE = _lib.PARAM_F32, _lib.ACC_NATIVE
LONG_SHAPES = [(4096, 4096), (4096, 11008)]
LONG_TS = (1024, 4096)
SK_SHAPE = (4096, 4096)
SK_TS = (4, 32)
SK_RANKS = (8, 50)
CODES = {"a": _lib.BF16, "b": _lib.BF16 | PF, "c": _lib.BF16 | PF | NATIVE}


def _p(t):
    return None if t is None else t.data_ptr()


class Long:
    """Forward + data gradient of one dense-accumulator layer on rotating parameter sets, in the three forms."""

    def __init__(self, T, d_in, d_out, r=8):
        lib = _lib.load()
        self.copies = max(2, -(-320 * 1024 * 1024 // (d_in * d_out * 2)) + 1)
        self.T, self.d_in, self.d_out, self.r = T, d_in, d_out, r
        g = torch.Generator(device="cuda").manual_seed(2)
        rnd = lambda *s, std, dt=BF16: (torch.randn(*s, device=DEV, dtype=F32, generator=g) * std).to(dt)   # noqa: E731
        self.x, self.dy = rnd(T, d_in, std=1.0), rnd(T, d_out, std=1.0)
        self.y, self.dx = torch.empty(T, d_out, device=DEV, dtype=BF16), torch.empty(T, d_in, device=DEV, dtype=BF16)
        self.h = torch.empty(T * 64, device=DEV, dtype=BF16)
        self.grads = {BF16: (torch.empty(d_in, r, device=DEV, dtype=BF16), torch.empty(r, d_out, device=DEV, dtype=BF16)),
                      F32: (torch.empty(d_in, r, device=DEV, dtype=F32), torch.empty(r, d_out, device=DEV, dtype=F32))}
        self.ws = {v: torch.empty(lib.sow_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_DENSE, c) + 256, device=DEV, dtype=torch.uint8)
                   for v, c in CODES.items()}
        self.sets = []
        for _ in range(self.copies):
            W = rnd(d_in, d_out, std=0.02)
            A32, B32 = rnd(d_in, r, std=0.05, dt=F32), rnd(r, d_out, std=0.05, dt=F32)
            self.sets.append(dict(W=W, W32=W.float(), A32=A32, B32=B32, A=A32.to(BF16), B=B32.to(BF16)))

    def call(self, v, j):
        lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
        s = self.sets[j % self.copies]
        A, B = (s["A"], s["B"]) if v == "a" else (s["A32"], s["B32"])
        acc = s["W32"] if v == "b" else s["W"]
        dA, dB = self.grads[BF16 if v == "a" else F32]
        code, ws = CODES[v], self.ws[v]
        _lib.check(lib.sow_forward(_p(self.x), _p(A), _p(B), _p(acc), None, None, _p(self.y), _p(self.h), self.T, self.d_in, self.d_out,
                                   self.r, 0, _lib.ACC_DENSE, 0.5, code, _p(ws), ws.numel(), st), "sow_forward " + v)
        _lib.check(lib.sow_backward_ex(_p(self.dy), _p(self.x), _p(self.h), _p(A), _p(B), _p(acc), None, _p(self.dx), _p(dA), _p(dB), None,
                                       self.T, self.d_in, self.d_out, self.r, 0, _lib.ACC_DENSE, 0.5, 0.0, code, _p(ws), ws.numel(),
                                       _lib.BWD_DATA, st), "sow_backward_ex " + v)


class Skinny:
    """sow_forward_skinny of one layer on rotating parameter sets: h = bf16 factors, f = fp32 factors (the pair of flags)."""

    def __init__(self, T, d_in, d_out, r, kind):
        lib = _lib.load()
        self.copies = max(2, -(-320 * 1024 * 1024 // (d_in * d_out * 2)) + 1)
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *s, std: torch.randn(*s, device=DEV, dtype=F32, generator=g) * std   # noqa: E731
        self.x = rnd(T, d_in, std=1.0).to(BF16)
        q = {"plain": lambda c: lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, _lib.ACC_DENSE, c),
             "e4m3": lambda c: lib.sow_forward_skinny_fp8_workspace_bytes(T, d_in, d_out, r, c),
             "mxfp4": lambda c: lib.sow_forward_skinny_fp4_workspace_bytes(T, d_in, d_out, r, c)}[kind]
        nws = q(_lib.BF16)
        assert nws > 0 and q(_lib.BF16 | PF | NATIVE) == nws
        ck = {"plain": _lib.ACC_DENSE, "e4m3": _lib.ACC_DENSE_FP8, "mxfp4": _lib.ACC_DENSE_FP4}[kind]
        self.keep, self.calls = [], {"h": [], "f": []}
        for _ in range(self.copies):
            W = rnd(d_in, d_out, std=0.02).to(BF16)
            acc_down, acc_up = ((W, None) if kind == "plain" else acc_quant.quantize_tensor(W) if kind == "e4m3"
                                else acc_quant.quantize_tensor(W, "mxfp4"))
            A32, B32, b32 = rnd(d_in, r, std=0.05), rnd(r, d_out, std=0.05), rnd(d_out, std=0.1)
            y = torch.empty(T, d_out, device=DEV, dtype=BF16)
            ws = torch.empty(nws, device=DEV, dtype=torch.uint8)
            for v, (A, B, b) in (("h", (A32.to(BF16), B32.to(BF16), b32.to(BF16))), ("f", (A32, B32, b32))):
                arr = (_lib.LayerArgs * 1)()
                a = arr[0]
                a.x, a.A, a.B, a.bias, a.y, a.acc_down, a.acc_up = _p(self.x), _p(A), _p(B), _p(b), _p(y), _p(acc_down), _p(acc_up)
                a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, ck, 0.5
                a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
                self.calls[v].append(arr)
                self.keep += [A, B, b]
            self.keep += [acc_down, acc_up, y, ws]

    def call(self, v, j):
        code = _lib.BF16 | (PF | NATIVE if v == "f" else 0)
        _lib.check(_lib.load().sow_forward_skinny(self.calls[v][j % self.copies], 1, code, torch.cuda.current_stream().cuda_stream), v)


def phase_times(s, v, n=8):
    """Mean kernel time (us) of the two phases of variant v over n calls (torch.profiler)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for j in range(n):
            s.call(v, j)
        torch.cuda.synchronize()
    out = {"skinny_a_kernel": [], "skinny_b_kernel": []}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            for k in out:
                if k in e.name:
                    out[k].append(e.time_range.elapsed_us())
    return {k: (sum(t) / len(t) if t else float("nan")) for k, t in out.items()}


def sweep(out_path, quick):
    rate = copy_rate()
    lines = [f"# tools/acc_native_bench.py on {torch.cuda.get_device_name(0)}; sow_version {_lib.load().sow_version()}",
             f"# copy rate (128 MiB buffers, read + write): {rate:.0f} GB/s; times in us per call, median of {TIMED} (after {WARM} "
             f"warm-up), variants alternated, weights rotating over > 256 MiB; +- = spread of the medians of three windows of 8",
             "# (i) forward + data gradient, r = 8, bf16: a = all bf16; b = SOW_PARAM_F32, fp32 accumulator; c = SOW_PARAM_F32 |",
             "#     SOW_ACC_NATIVE, bf16 accumulator.  acc pack = 2 x 6 d_in d_out bytes at the copy rate (one pack per call, two calls);",
             "#     AB pack = 2 x 6 (d_in r + r d_out) bytes at the copy rate (next to one more launch per call)",
             f"{'shape':>14} {'T':>5} | {'a':>7} {'+-':>5} {'b':>7} {'+-':>5} {'c':>7} {'+-':>5} | {'b - c':>6} {'acc pack':>8} {'ratio':>5} | "
             f"{'c - a':>6} {'AB pack':>7}"]
    print("\n".join(lines), flush=True)
    for d_in, d_out in (LONG_SHAPES[:1] if quick else LONG_SHAPES):
        for T in ((1024,) if quick else LONG_TS):
            s = Long(T, d_in, d_out)
            m = measure(s, ("a", "b", "c"))
            a, b, c = m["a"], m["b"], m["c"]
            accp, abp = 2 * 6 * d_in * d_out / rate * 1e-3, 2 * 6 * (d_in * s.r + s.r * d_out) / rate * 1e-3
            line = (f"{f'{d_in}->{d_out}':>14} {T:5d} | {a[0]:7.1f} {a[1]:5.1f} {b[0]:7.1f} {b[1]:5.1f} {c[0]:7.1f} {c[1]:5.1f} | "
                    f"{b[0] - c[0]:6.1f} {accp:8.1f} {(b[0] - c[0]) / accp:5.2f} | {c[0] - a[0]:6.1f} {abp:7.2f}")
            print(line, flush=True)
            lines.append(line)
            del s
            torch.cuda.empty_cache()
    head = ["# (ii) sow_forward_skinny, one layer: h = bf16 factors, f = fp32 factors (SOW_PARAM_F32 | SOW_ACC_NATIVE); `out` = |f - h|",
            "#      exceeds the larger spread of the two; then A / B = the mean kernel time of phase A / phase B, h -> f",
            f"{'shape':>14} {'kind':>6} {'T':>3} {'r':>3} | {'h':>7} {'+-':>5} {'f':>7} {'+-':>5} | {'f - h':>6} {'f/h':>5} {'out':>4}"]
    print("\n".join(head), flush=True)
    lines += head
    d_in, d_out = SK_SHAPE
    for kind in ("plain", "e4m3", "mxfp4"):
        for r in ((50,) if quick else SK_RANKS):
            for T in SK_TS:
                s = Skinny(T, d_in, d_out, r, kind)
                m = measure(s, ("h", "f"))
                h, f = m["h"], m["f"]
                outside = abs(f[0] - h[0]) > max(h[1], f[1])
                line = (f"{f'{d_in}->{d_out}':>14} {kind:>6} {T:3d} {r:3d} | {h[0]:7.1f} {h[1]:5.1f} {f[0]:7.1f} {f[1]:5.1f} | "
                        f"{f[0] - h[0]:6.1f} {f[0] / h[0]:5.2f} {'yes' if outside else 'no':>4}")
                if outside:
                    ph, pf = phase_times(s, "h"), phase_times(s, "f")
                    line += (f" | A {ph['skinny_a_kernel']:.1f} -> {pf['skinny_a_kernel']:.1f}, "
                             f"B {ph['skinny_b_kernel']:.1f} -> {pf['skinny_b_kernel']:.1f}")
                print(line, flush=True)
                lines.append(line)
                del s
                torch.cuda.empty_cache()
    lines.append("# not measured: f16 timings, a full finetune step, generate()")
    print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="one long shape at T = 1024, the skinny rows at r = 50 only")
    a = ap.parse_args()
    sweep(a.out, a.quick)
