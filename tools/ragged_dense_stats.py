#!/usr/bin/env python3
"""Timing of bf16 layers with a 5461-wide side (llama_1b's MLP) and a DENSE frozen accumulator at rank 200 -- the steady
state of the flagship configuration after the first accumulate().  Forward, data gradient and weight gradients through the
C ABI, each phase timed separately (CUDA events), for the variants
  new       gemm_rag + the ragged chain_wide / skinny_tn_wide,
  no_gemm   NO_RAGGED_GEMM = 1: the dense product on gemm_auto (generic kernel), the ragged chain and weight gradients kept,
  generic   NO_RAGGED = 1: the launches of the parent commit,
  aligned   the aligned neighbour (5464 instead of 5461) on gemm4 + chain_wide,
  parent    (--parent-lib PATH) a build of the parent commit loaded beside this one, default switches.
The variants are timed ALTERNATELY in one process, --rounds times; the table gives the median over the rounds and the
spread (min .. max) so that a difference can be held against the run-to-run noise.  --block adds fwd + bwd of a llama_1b
decoder block's seven projections through the module surface (SoWLinear, rank 200) after accumulate().  Run it under
`rocprofv3 --kernel-trace --stats` (with --rounds 1) for per-kernel times."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sow_amd import _lib  # noqa: E402

DEV = "cuda"
SWITCHES = {"new": {}, "no_gemm": dict(NO_RAGGED_GEMM=1), "generic": dict(NO_RAGGED=1), "aligned": {}, "parent": {}}


def load_other(path):
    """A second build of the library (the parent commit's) beside the package's own, with the same signatures."""
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def timed(fn, iters):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


class Layer:
    """The buffers and the three phase calls of one dense-accumulator layer on library `lib`."""

    def __init__(self, lib, T, d_in, d_out, r):
        self.lib, self.dims = lib, (T, d_in, d_out, r)
        g = torch.Generator(device=DEV).manual_seed(0)
        bf = torch.bfloat16
        rnd = lambda *s, std=1.0: (torch.randn(*s, device=DEV, generator=g) * std).to(bf)
        self.x, self.dy = rnd(T, d_in), rnd(T, d_out)
        self.A, self.B, self.W = rnd(d_in, r, std=0.03), rnd(r, d_out, std=0.03), rnd(d_in, d_out, std=0.02)
        self.bias = torch.zeros(d_out, device=DEV, dtype=bf)
        self.y, self.dx = torch.empty(T, d_out, device=DEV, dtype=bf), torch.empty(T, d_in, device=DEV, dtype=bf)
        self.h = torch.empty(lib.sow_h_save_elems(T, r), device=DEV, dtype=bf)
        self.dA, self.dB, self.db = torch.empty_like(self.A), torch.empty_like(self.B), torch.empty_like(self.bias)
        self.nws = lib.sow_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_DENSE, _lib.BF16)
        self.ws = torch.empty(self.nws, device=DEV, dtype=torch.uint8)

    def fwd(self):
        T, d_in, d_out, r = self.dims
        p = lambda t: t.data_ptr()
        rc = self.lib.sow_forward(p(self.x), p(self.A), p(self.B), p(self.W), None, p(self.bias), p(self.y), p(self.h), T, d_in,
                                  d_out, r, 0, _lib.ACC_DENSE, 0.5, _lib.BF16, p(self.ws), self.nws,
                                  torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def bwd(self, phases):
        T, d_in, d_out, r = self.dims
        p = lambda t: t.data_ptr()
        rc = self.lib.sow_backward_ex(p(self.dy), p(self.x), p(self.h), p(self.A), p(self.B), p(self.W), None, p(self.dx),
                                      p(self.dA), p(self.dB), p(self.db), T, d_in, d_out, r, 0, _lib.ACC_DENSE, 0.5, 0.0,
                                      _lib.BF16, p(self.ws), self.nws, phases, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def phases(self):
        return (self.fwd, lambda: self.bwd(_lib.BWD_DATA), lambda: self.bwd(_lib.BWD_WEIGHTS))


def set_switches(lib, values):
    old = {k: lib.sow_get_switch(k.encode()) for k in values}
    for k, v in values.items():
        assert lib.sow_set_switch(k.encode(), v) == 0, k
    return old


def layer_table(T, d_in, d_out, r, variants, libs, rounds, iters):
    """{variant: [(median, min, max) per phase]} with the variants alternating inside every round."""
    layers = {}
    for v in variants:
        di, do = (5464 if d_in == 5461 else d_in, 5464 if d_out == 5461 else d_out) if v == "aligned" else (d_in, d_out)
        layers[v] = Layer(libs[v], T, di, do, r)
    samples = {v: [[], [], []] for v in variants}
    for rnd in range(rounds + 1):            # round 0 warms every variant up
        for v in variants:
            old = set_switches(libs[v], SWITCHES[v])
            try:
                L = layers[v]
                L.fwd()
                for i, fn in enumerate(L.phases()):
                    fn()
                    t = timed(fn, iters)
                    if rnd:
                        samples[v][i].append(t)
            finally:
                set_switches(libs[v], old)
    # the variants compute the same layer: the kernels differ in summation order only
    if "new" in layers and "generic" in layers:
        a, b = layers["new"], layers["generic"]
        for name in ("y", "dx", "dA", "dB"):
            ta, tb = getattr(a, name).float(), getattr(b, name).float()
            print(f"    new vs generic {name}: max |diff| / max |ref| = {float((ta - tb).abs().max() / tb.abs().max()):.3g}")
    return {v: [(statistics.median(s), min(s), max(s)) for s in samples[v]] for v in variants}


def block_time(T, r, rounds, iters):
    from sow_amd import SoWLinear
    shapes = [(2048, 2048)] * 4 + [(2048, 5461), (2048, 5461), (5461, 2048)]
    layers = [SoWLinear(i, o, bias=False, rank=r, scale=0.5, init_method="normal", device=DEV, dtype=torch.bfloat16)
              for i, o in shapes]
    for m in layers:
        m.virtual_rank = min(m.in_features, m.out_features)     # what prepare_sow sets: the accumulator stays dense
        m.accumulate()
        torch.nn.init.normal_(m.upscale_weights[0], std=0.02)
    xs = [torch.randn(T, i, device=DEV, dtype=torch.bfloat16, requires_grad=True) for i, _ in shapes]
    dys = [torch.randn(T, o, device=DEV, dtype=torch.bfloat16) for _, o in shapes]

    def step():
        for m, x, dy in zip(layers, xs, dys):
            m(x).backward(dy)

    out = {"new": [], "generic": []}
    for rnd in range(rounds + 1):
        for case in out:
            with _lib.switch(**SWITCHES[case]):
                step()
                t = timed(step, iters)
            if rnd:
                out[case].append(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, nargs="+", default=[32768, 4096])
    ap.add_argument("--r", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--variants", nargs="+", default=["new", "no_gemm", "generic", "aligned"])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--block", action="store_true")
    a = ap.parse_args()
    lib = _lib.load()
    variants = list(a.variants)
    libs = {v: lib for v in variants}
    if a.parent_lib:
        libs["parent"] = load_other(a.parent_lib)
        if "parent" not in variants:
            variants.append("parent")
        print(f"parent build: version {libs['parent'].sow_version()}; this build: version {lib.sow_version()}")
    print(f"bf16, dense accumulator, r = {a.r}, bias, scale 0.5; {a.rounds} alternating rounds, median of {a.iters} calls each; "
          "microseconds: median (min .. max) over the rounds")
    for T in a.T:
        for d_in, d_out in ((2048, 5461), (5461, 2048)):
            print(f"T = {T}, {d_in} -> {d_out}", flush=True)
            tab = layer_table(T, d_in, d_out, a.r, variants, libs, a.rounds, a.iters)
            for v in variants:
                cells = "  ".join(f"{n} {m:9.1f} ({lo:9.1f} .. {hi:9.1f})" for n, (m, lo, hi) in zip(("fwd", "dgrad", "wgrad"), tab[v]))
                print(f"    {v:>8s}  {cells}", flush=True)
            for other in variants:
                if other != "new" and "new" in tab:
                    ratios = "  ".join(f"{n} {tab[other][i][0] / tab['new'][i][0]:6.2f}x" for i, n in enumerate(("fwd", "dgrad", "wgrad")))
                    print(f"    {other:>8s} / new  {ratios}", flush=True)
    if a.block:
        for T in a.T:
            out = block_time(T, a.r, a.rounds, a.iters)
            for case, ts in out.items():
                print(f"llama_1b block (7 SoWLinear, r = {a.r}, dense accumulators) fwd + bwd, T = {T}, {case}: "
                      f"{statistics.median(ts):.1f} us ({min(ts):.1f} .. {max(ts):.1f})", flush=True)


if __name__ == "__main__":
    main()
