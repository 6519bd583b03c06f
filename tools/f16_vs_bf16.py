"""f16 against bf16 on the streaming kernels: one SoWLinear forward and data-gradient pass per point, the same bytes and the
same MFMA cycles per element type.  Prints one line per point (median of `--iters` timed launches after warm-up).

    python tools/f16_vs_bf16.py [--iters 50]
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -- python tools/f16_vs_bf16.py    (kernel names and per-kernel times)
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sow_amd import _lib, ops  # noqa: E402

POINTS = [   # (name, T, d_in, d_out, r, accumulator)
    ("llama_60m 512x512 r50", 32768, 512, 512, 50, "none"),
    ("llama_60m 512x512 r50 dense (gemm4h, K=512)", 32768, 512, 512, 50, "dense"),
    ("north-star 768x768 r50", 32768, 768, 768, 50, "none"),
]


def _time(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    dev = "cuda"
    torch.manual_seed(0)
    for name, T, d_in, d_out, r, acc in POINTS:
        res = {}
        for dt in (torch.bfloat16, torch.float16):
            x = torch.randn(T, d_in, device=dev).to(dt)
            A = (torch.randn(d_in, r, device=dev) / d_in ** 0.5).to(dt)
            B = (torch.randn(r, d_out, device=dev) / r ** 0.5).to(dt)
            W = (torch.randn(d_in, d_out, device=dev) / d_in ** 0.5).to(dt) if acc == "dense" else None
            dy = torch.randn(T, d_out, device=dev).to(dt)
            y, h = ops.sow_forward(x, A, B, W, None, None, 0.5)
            nws = ops.workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_DENSE if W is not None else _lib.ACC_NONE, dt)
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            dx = torch.empty(T, d_in, device=dev, dtype=dt)
            fwd = _time(lambda: ops.sow_forward(x, A, B, W, None, None, 0.5), args.iters)
            bwd = _time(lambda: ops.sow_backward(dy, x, h, A, B, W, None, 0.5, False, phases=_lib.BWD_DATA, dx=dx,
                                                 workspace=ws), args.iters)
            res[dt] = (fwd, bwd)
        (fb, bb), (ff, bf) = res[torch.bfloat16], res[torch.float16]
        print(f"{name:48s} T={T}  forward bf16 {fb:7.1f} us  f16 {ff:7.1f} us  ({ff / fb - 1:+.1%})   "
              f"data grad bf16 {bb:7.1f} us  f16 {bf:7.1f} us  ({bf / bb - 1:+.1%})", flush=True)


if __name__ == "__main__":
    main()
