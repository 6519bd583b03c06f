#!/usr/bin/env python3
"""Timing of bf16 layers with a 5461-wide side (llama_1b's MLP) at T = 32768: forward, data gradient and weight gradients
through the C ABI, each phase timed separately (CUDA events, median of --iters), for three cases:
  ragged   the fused ragged kernels (chain_wide / skinny_tn_wide with ragged rows),
  generic  the same layer with the NO_RAGGED switch (the generic kernels of the parent commit),
  aligned  the aligned neighbour (5464 instead of 5461) on its own kernels.
--block adds fwd + bwd of a llama_1b decoder block's seven projections through the module surface (SoWLinear, rank 200),
with and without NO_RAGGED.  Run it under `rocprofv3 --kernel-trace --stats` for per-kernel times (tools/kstats.py)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sow_amd import _lib  # noqa: E402

DEV = "cuda"


def bench(fn, iters):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def layer_times(T, d_in, d_out, r, iters):
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(0)
    bf = torch.bfloat16
    x = torch.randn(T, d_in, device=DEV, generator=g).to(bf)
    dy = torch.randn(T, d_out, device=DEV, generator=g).to(bf)
    A = (torch.randn(d_in, r, device=DEV, generator=g) * 0.03).to(bf)
    B = (torch.randn(r, d_out, device=DEV, generator=g) * 0.03).to(bf)
    bias = torch.zeros(d_out, device=DEV, dtype=bf)
    y, dx = torch.empty(T, d_out, device=DEV, dtype=bf), torch.empty(T, d_in, device=DEV, dtype=bf)
    h = torch.empty(lib.sow_h_save_elems(T, r), device=DEV, dtype=bf)
    dA, dB, db = torch.empty_like(A), torch.empty_like(B), torch.empty_like(bias)
    nws = lib.sow_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_NONE, _lib.BF16)
    ws = torch.empty(nws, device=DEV, dtype=torch.uint8)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def fwd():
        _lib.check(lib.sow_forward(p(x), p(A), p(B), None, None, p(bias), p(y), p(h), T, d_in, d_out, r, 0, _lib.ACC_NONE, 0.5,
                                   _lib.BF16, p(ws), nws, s), "sow_forward")

    def bwd(phases):
        _lib.check(lib.sow_backward_ex(p(dy), p(x), p(h), p(A), p(B), None, None, p(dx), p(dA), p(dB), p(db), T, d_in, d_out, r,
                                       0, _lib.ACC_NONE, 0.5, 0.0, _lib.BF16, p(ws), nws, phases, s), "sow_backward_ex")

    fwd()
    t_f = bench(fwd, iters)
    t_d = bench(lambda: bwd(_lib.BWD_DATA), iters)
    t_w = bench(lambda: bwd(_lib.BWD_WEIGHTS), iters)
    return t_f, t_d, t_w


def block_time(T, r, iters):
    from sow_amd import SoWLinear
    shapes = [(2048, 2048)] * 4 + [(2048, 5461), (2048, 5461), (5461, 2048)]
    layers = [SoWLinear(i, o, bias=False, rank=r, scale=0.5, init_method="normal", device=DEV, dtype=torch.bfloat16)
              for i, o in shapes]
    xs = [torch.randn(T, i, device=DEV, dtype=torch.bfloat16, requires_grad=True) for i, _ in shapes]
    dys = [torch.randn(T, o, device=DEV, dtype=torch.bfloat16) for _, o in shapes]

    def step():
        for m, x, dy in zip(layers, xs, dys):
            m(x).backward(dy)

    return bench(step, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=32768)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--block", action="store_true")
    a = ap.parse_args()
    print(f"T = {a.T}, bf16, bias, scale 0.5; median of {a.iters}; microseconds")
    print(f"{'layer':>16s} {'r':>4s} {'case':>8s} {'fwd':>9s} {'dgrad':>9s} {'wgrad':>9s} {'sum':>9s}")
    for d_in, d_out in ((2048, 5461), (5461, 2048)):
        for r in (200, 50):
            for case in ("ragged", "generic", "aligned"):
                di, do = (d_in, d_out) if case != "aligned" else (5464 if d_in == 5461 else d_in, 5464 if d_out == 5461 else d_out)
                with _lib.switch(NO_RAGGED=1 if case == "generic" else -1):
                    t = layer_times(a.T, di, do, r, a.iters)
                print(f"{f'{di}->{do}':>16s} {r:4d} {case:>8s} {t[0]:9.1f} {t[1]:9.1f} {t[2]:9.1f} {sum(t):9.1f}", flush=True)
    if a.block:
        for case in ("ragged", "generic"):
            with _lib.switch(NO_RAGGED=1 if case == "generic" else -1):
                t = block_time(a.T, 200, max(3, a.iters // 2))
            print(f"llama_1b block (7 SoWLinear, r = 200) fwd + bwd, {case}: {t:.1f} us", flush=True)


if __name__ == "__main__":
    main()
