#!/usr/bin/env python3
"""Clipping the factor bucket's gradient: the device record inside FactorAdamW.step against torch's clip_grad_norm_.

Synthetic buckets of plain parameters in the factor layouts of the reference's models (no model, no data):
  llama_60m r=50      8 blocks x 7 layers (512 / 1376), A [d_in, 50] and B [50, d_out]: 112 tensors, 3.9 M elements
  roberta-base r=8    one encoder block, 6 layers (768 / 3072) with their biases: 18 tensors, 117 504 elements, TWO param
                      groups (factors with weight decay, biases without)
  llama-7b r=8        32 blocks x 7 layers (4096 / 11008): 448 tensors, 20.0 M elements
Timed per layout, HIP events around the call, Python included, the four variants alternating call by call in one process:
  step        opt.step()                                                          (no clipping: the floor)
  torch-clip  torch.nn.utils.clip_grad_norm_(bucket.params, 1.0); opt.step()     (multi-tensor norm over the views, a second
                                                                                  pass that scales and re-rounds the gradient)
  fused       opt.step(max_grad_norm=1.0, skip_nonfinite=True)                   (sow_grad_stats_flat + sow_adamw_flat_seg_stats)
  fused-skip  the same call with every skip counter at 1, as after one skipped step and before the next state_dict(): every
              workgroup forms its bias correction on the device (one lane: two double pow, a sqrt, a divide; LDS hands it on)
WARM warm-up calls, then REPEATS windows of TIMED calls each: the figure of a variant is the median of the window medians,
its spread the distance between the largest and the smallest window median.  Every variant has its own bucket and optimizer.

  python tools/grad_clip_bench.py [--out profiles/grad_clip.txt]
  python tools/grad_clip_bench.py --one LAYOUT VARIANT        (TRACE_STEPS calls, for rocprofv3 --kernel-trace)
  python tools/grad_clip_bench.py --summarize DIR             (launches per call from the trace under DIR)
"""
import argparse
import collections
import csv
import glob
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sow_amd import FactorAdamW, FactorBucket, _lib  # noqa: E402

DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
WARM, TIMED, REPEATS = 10, 48, 5
TRACE_STEPS = 23          # a prime: a kernel whose launch count is a multiple of it is taken as part of the step
VARIANTS = ("step", "torch-clip", "fused", "fused-skip")


def _llama(hidden, inter, blocks, r):
    shapes = []
    for _ in range(blocks):
        for i, o in ((hidden, hidden),) * 4 + ((hidden, inter),) * 2 + ((inter, hidden),):
            shapes += [(i, r), (r, o)]
    return shapes, 0


def _roberta_block(r):
    layers = ((768, 768),) * 4 + ((768, 3072), (3072, 768))
    shapes = []
    for i, o in layers:
        shapes += [(i, r), (r, o)]
    return shapes + [(o,) for _, o in layers], 6       # the last 6 tensors are the biases: a param group of their own


LAYOUTS = {
    "llama_60m-r50-bf16": (lambda: _llama(512, 1376, 8, 50), BF16),
    "roberta-base-r8-bias-bf16": (lambda: _roberta_block(8), BF16),
    "llama-7b-r8-bf16": (lambda: _llama(4096, 11008, 32, 8), BF16),
    "llama_60m-r50-f32": (lambda: _llama(512, 1376, 8, 50), F32),
}


class Setup:
    def __init__(self, name, variants=VARIANTS):
        mk, dtype = LAYOUTS[name]
        shapes, n_bias = mk()
        g = torch.Generator(device="cuda").manual_seed(1)
        self.bucket, self.opt = {}, {}
        for v in variants:
            ps = [nn.Parameter((torch.randn(s, device=DEV, generator=g) * 0.05).to(dtype)) for s in shapes]
            b = FactorBucket(ps)
            for p in ps:                                   # norm = 0.01 sqrt(numel): well above 1 at every layout
                p.grad.copy_((torch.randn(p.shape, device=DEV, generator=g) * 0.01).to(dtype))
            groups = None
            if n_bias:
                groups = [{"params": ps[:-n_bias], "lr": 1e-3, "weight_decay": 0.1},
                          {"params": ps[-n_bias:], "lr": 1e-4, "weight_decay": 0.0}]
            self.bucket[v], self.opt[v] = b, FactorAdamW(b, lr=1e-3, weight_decay=0.1, param_groups=groups)
            if v == "fused-skip":
                self.opt[v].skip_counters.fill_(1)
        self.numel, self.tensors, self.dtype, self.groups = b.padded_numel, len(shapes), dtype, 2 if n_bias else 1

    def call(self, v):
        if v == "step":
            self.opt[v].step()
        elif v == "torch-clip":
            torch.nn.utils.clip_grad_norm_(self.bucket[v].params, 1.0)
            self.opt[v].step()
        else:
            self.opt[v].step(max_grad_norm=1.0, skip_nonfinite=True)


def measure(S):
    for _ in range(WARM):
        for v in VARIANTS:
            S.call(v)
    torch.cuda.synchronize()
    meds = {v: [] for v in VARIANTS}
    for _ in range(REPEATS):
        times = {v: [] for v in VARIANTS}
        for _ in range(TIMED):
            for v in VARIANTS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                S.call(v)
                e1.record()
                e1.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1e3)
        for v in VARIANTS:
            meds[v].append(statistics.median(times[v]))
    return {v: (statistics.median(m), max(m) - min(m)) for v, m in meds.items()}


def sweep(out_path):
    lines = [f"# tools/grad_clip_bench.py on {torch.cuda.get_device_name(0)}; sow_version {_lib.load().sow_version()}",
             "# synthetic factor buckets (plain parameters, gradient norm well above max_norm = 1); us per call, HIP events, Python "
             f"included: median of {REPEATS} window medians ({TIMED} calls each, {WARM} warm-up), +- = spread of the window medians",
             "# step = opt.step(); torch-clip = torch.nn.utils.clip_grad_norm_(bucket.params, 1.0) + opt.step(); "
             "fused = opt.step(max_grad_norm=1.0, skip_nonfinite=True); fused-skip = fused with the skip counters at 1 (bias "
             "correction formed on the device)",
             "# margin = torch-clip - fused - (sum of their spreads): positive = the fused step is faster beyond the noise",
             f"{'layout':>26} {'elements':>9} {'tensors':>7} {'groups':>6} | {'step':>13} {'torch-clip':>13} {'fused':>13} {'fused-skip':>13} | "
             f"{'clip/fused':>10} {'fused-step':>10} {'margin':>7}"]
    print("\n".join(lines), flush=True)
    cell = lambda v: f"{v[0]:8.1f}+-{v[1]:<4.1f}"   # noqa: E731
    for name in LAYOUTS:
        S = Setup(name)
        m = measure(S)
        margin = m["torch-clip"][0] - m["fused"][0] - (m["torch-clip"][1] + m["fused"][1])
        line = (f"{name:>26} {S.numel:9d} {S.tensors:7d} {S.groups:6d} | {cell(m['step'])} {cell(m['torch-clip'])} {cell(m['fused'])} {cell(m['fused-skip'])} | "
                f"{m['torch-clip'][0] / m['fused'][0]:10.2f} {m['fused'][0] - m['step'][0]:10.1f} {margin:7.1f}")
        print(line, flush=True)
        lines.append(line)
        del S
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def one(name, variant):
    S = Setup(name, variants=(variant,))
    torch.cuda.synchronize()
    for _ in range(TRACE_STEPS):
        S.call(variant)
    torch.cuda.synchronize()


def summarize(d):
    f = glob.glob(d + "/**/*_kernel_trace.csv", recursive=True)[0]
    agg = collections.defaultdict(list)
    for r in csv.DictReader(open(f)):
        agg[r["Kernel_Name"]].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    per_call, busy = 0, 0.0
    for name, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
        in_step = len(v) % TRACE_STEPS == 0
        k = len(v) // TRACE_STEPS if in_step else 0
        per_call += k
        busy += sum(v) / TRACE_STEPS / 1e3 if in_step else 0.0
        print(f"{name[:96]:96s} n={len(v):5d} per call={k if in_step else '-':>3} med={statistics.median(v) / 1e3:7.1f}us")
    print(f"launches per call: {per_call}; kernel time per call: {busy:.1f} us (kernels launched a multiple of {TRACE_STEPS} times)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", nargs=2, metavar=("LAYOUT", "VARIANT"))
    ap.add_argument("--summarize", metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.one:
        one(*a.one)
    else:
        sweep(a.out)
