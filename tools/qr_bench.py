#!/usr/bin/env python3
"""Timing of sow_qr_thin: the blocked route (qr_blocked.hip, more than 64 factored columns) against the one-workgroup
route (NO_BLOCKED_QR = 1), fp32 in and out, R requested.  CUDA events around single calls through the C ABI, one warm-up
call, the median of --reps (>= 5) timed calls and their spread.

  default      the table of shapes and a sweep of k at m = n = 1376 that locates the crossover;
  --prepare    prepare_sow(decompose='qr') on the projections of llama_60m (8 blocks of 4 x 512 x 512, 2 x 512 -> 1376,
               1376 -> 512), both routes;
  --parent-lib PATH   a build of the parent commit: its outputs against this build's under NO_BLOCKED_QR = 1, bit for bit;
  --one M N K  one warm-up and one call (run under `rocprofv3 --kernel-trace --stats -- python tools/qr_bench.py --one ..`).
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sow_amd import _lib  # noqa: E402

DEV = "cuda"
SHAPES = [(512, 512, 512), (768, 768, 300), (1376, 512, 512), (2048, 5461, 2048), (4096, 4096, 4096)]
SWEEP = [(1376, 1376, k) for k in (32, 64, 65, 96, 128, 256)]


class Call:
    def __init__(self, lib, m, n, k):
        self.lib, self.dims = lib, (m, n, k)
        self.W = torch.randn(m, n, generator=torch.Generator().manual_seed(m + n + k)).to(DEV)
        self.Q = torch.empty(m, k, device=DEV)
        self.R = torch.empty(k, n, device=DEV)
        self.nws = lib.sow_qr_workspace_bytes(m, n, k, _lib.F32, 1)
        self.ws = torch.empty(self.nws, device=DEV, dtype=torch.uint8)

    def __call__(self):
        m, n, k = self.dims
        rc = self.lib.sow_qr_thin(self.W.data_ptr(), n, m, n, _lib.F32, k, self.Q.data_ptr(), k, self.R.data_ptr(), n, _lib.F32,
                                  self.ws.data_ptr(), self.nws, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def table(lib, shapes, reps, new_only=False):
    print(f"{'m':>5} {'n':>5} {'k':>5} | {'blocked ms (min .. max)':>30} | {'one workgroup ms (min .. max)':>32} | ratio", flush=True)
    for m, n, k in shapes:
        call = Call(lib, m, n, k)
        new = timed(call, reps)
        if new_only:
            print(f"{m:5d} {n:5d} {k:5d} | {new[0]:10.3f} ({new[1]:.3f} .. {new[2]:.3f})", flush=True)
            continue
        with _lib.switch(NO_BLOCKED_QR=1):
            old = timed(call, reps)
        f = lambda t: f"{t[0]:10.3f} ({t[1]:.3f} .. {t[2]:.3f})"
        print(f"{m:5d} {n:5d} {k:5d} | {f(new):>30} | {f(old):>32} | {old[0] / new[0]:6.2f} x", flush=True)


def llama_60m():
    from torch import nn
    model = nn.Module()
    model.layers = nn.ModuleList()
    for _ in range(8):
        blk = nn.Module()
        for name in ("q_proj", "k_proj", "v_proj", "o_proj"):
            setattr(blk, name, nn.Linear(512, 512, bias=False))
        blk.gate_proj, blk.up_proj, blk.down_proj = (nn.Linear(512, 1376, bias=False), nn.Linear(512, 1376, bias=False),
                                                    nn.Linear(1376, 512, bias=False))
        model.layers.append(blk)
    return model


def prepare(rank):
    from sow_amd import SoWConfig, prepare_sow
    cfg = SoWConfig(target_modules=["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"], rank=rank,
                    init_method="normal_QR", decompose="qr", device=DEV)
    for tag, sw in (("warm-up", {}), ("blocked", {}), ("one workgroup", dict(NO_BLOCKED_QR=1)), ("blocked", {})):
        torch.manual_seed(0)
        model = llama_60m()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with _lib.switch(**sw):
            prepare_sow(model, cfg)
            torch.cuda.synchronize()
        print(f"prepare_sow(decompose='qr'), llama_60m projections (56 matrices), rank {rank}, {tag}: "
              f"{time.perf_counter() - t0:.3f} s", flush=True)


def against_parent(lib, path):
    other = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(other, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    for m, n, k in ((200, 200, 200), (1376, 512, 512)):
        mine, theirs = Call(lib, m, n, k), Call(other, m, n, k)
        with _lib.switch(NO_BLOCKED_QR=1):
            mine()
        theirs()
        torch.cuda.synchronize()
        same = torch.equal(mine.Q.view(torch.int32), theirs.Q.view(torch.int32)) and \
            torch.equal(mine.R.view(torch.int32), theirs.R.view(torch.int32))
        print(f"{m} x {n}, k = {k}: NO_BLOCKED_QR = 1 against the parent build: "
              f"{'Q and R bit-identical' if same else 'DIFFERENT'}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prepare", action="store_true")
    ap.add_argument("--rank", type=int, default=128)
    ap.add_argument("--parent-lib")
    ap.add_argument("--one", type=int, nargs=3, metavar=("M", "N", "K"))
    ap.add_argument("--skip-table", action="store_true")
    ap.add_argument("--new-only", action="store_true", help="time the blocked route only (A/B builds of the block width)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: a median of at least 5")
    lib = _lib.load()
    if a.one:
        call = Call(lib, *a.one)
        call()
        call()
        torch.cuda.synchronize()
        return
    print(f"# {torch.cuda.get_device_name(0)}, library version {lib.sow_version()}, {os.path.basename(_lib.LIB_PATH)}")
    if a.parent_lib:
        against_parent(lib, a.parent_lib)
    if not a.skip_table:
        table(lib, SHAPES, a.reps, a.new_only)
        print("# crossover sweep, m = n = 1376 (k <= 64 runs the one-workgroup kernel on both sides)")
        table(lib, SWEEP, a.reps, a.new_only)
    if a.prepare:
        prepare(a.rank)


if __name__ == "__main__":
    main()
