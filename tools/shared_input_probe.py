#!/usr/bin/env python3
"""Shared-input siblings against today's grouped path, llama_60m shapes (r = 50, T = 32768, bf16):
  q + k + v : 3 x 512 -> 512          gate + up : 2 x 512 -> 1376

  forward        grouped: sow_forward_group (each sibling streams x)      shared: sow_forward_shared (x read once)
  backward data  grouped: sow_backward_group(DATA) + n - 1 torch adds of the siblings' dX (what group.py does)
                 shared : sow_backward_shared(DATA) (one dX, summed in the kernel)

Timing: device events around `--reps` back-to-back launches of one variant, the variants alternating, `--rounds` rounds after
`--warmup` rounds; median / min / max of the per-launch time over the rounds.  Every time is printed next to its
algorithmic bytes (activations only: the factors are a few hundred KB) and as a fraction of the time those bytes take at
the copy rate measured in the same process (a 512 MiB device-to-device copy).

  python tools/shared_input_probe.py [--out DIR]                   timing table (+ DIR/shared_input_timing.json)
  rocprofv3 --kernel-trace --stats -f csv -d D -o run -- python tools/shared_input_probe.py --trace [--group ...]
                                                                   a few launches of each variant, for the kernel trace
                                                                   (one group per trace: the grouped launches of two
                                                                   groups share a kernel name)
  python tools/shared_input_probe.py --summarize D                 per-kernel table of that trace (all kernels, adds included)
  --group name:d_in:d_out,d_out,...  (repeatable) other sibling sets instead of the two llama_60m groups
"""
import argparse
import collections
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, R = 32768, 50
GROUPS = {"qkv": (512, [512, 512, 512]), "gateup": (512, [1376, 1376])}


def summarize(d):
    f = glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True)[0]
    agg = collections.defaultdict(list)
    for r in csv.DictReader(open(f)):
        agg[r["Kernel_Name"][:90]].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for k, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
        v = sorted(v)
        print(f"{k:92s} n={len(v):4d} med={v[len(v) // 2]:8.1f} us  min={v[0]:8.1f}  max={v[-1]:8.1f}")


def build(name):
    import torch
    from sow_amd import _lib, ops
    d_in, outs = GROUPS[name]
    g = torch.Generator(device="cuda").manual_seed(0)
    bf = torch.bfloat16
    x = torch.randn(T, d_in, device="cuda", generator=g).to(bf)
    layers = []
    for d_out in outs:
        A = (torch.randn(d_in, R, device="cuda", generator=g) * 0.04).to(bf)
        B = (torch.randn(R, d_out, device="cuda", generator=g) * 0.04).to(bf)
        dy = torch.randn(T, d_out, device="cuda", generator=g).to(bf)
        layers.append((A, B, dy))
    shared_dx = torch.empty_like(x)
    hs = [torch.empty(T * 64, dtype=bf, device="cuda") for _ in layers]   # one h per sibling: the backward reads it

    def calls(shared):
        cs = []
        for (A, B, dy), h in zip(layers, hs):
            out = (torch.empty_like(A), torch.empty_like(B), None)
            cs.append(ops.LayerCall(x, A, B, scale=0.5, h=h, dy2=dy, dx=shared_dx if shared else torch.empty_like(x),
                                    out=out, y=torch.empty(T, B.shape[1], dtype=bf, device="cuda")))
        return cs

    grouped, shared = ops.LayerGroup(calls(False)), ops.SharedInputGroup(calls(True))
    n = len(outs)

    def fwd_grouped():
        grouped.forward()

    def fwd_shared():
        assert shared.forward()

    def bwd_grouped():
        grouped.backward(_lib.BWD_DATA)
        dx = grouped.calls[-1].dx
        for c in reversed(grouped.calls[:-1]):   # group.py _input_grad
            dx = dx + c.dx
        return dx

    def bwd_shared():
        assert shared.backward(_lib.BWD_DATA)

    e = 2   # bytes per element
    sum_out = sum(outs)
    bytes_ = {
        "fwd_grouped": e * T * (n * d_in + sum_out + n * 64),
        "fwd_shared": e * T * (d_in + sum_out + n * 64),
        # dY_i in, dX_i out, dh_i out; then n - 1 adds of 3 [T, d_in] passes each
        "bwd_grouped": e * T * (sum_out + n * d_in + n * 64) + e * T * d_in * 3 * (n - 1),
        "bwd_shared": e * T * (sum_out + d_in + n * 64),
    }
    fwd_grouped()
    bwd_grouped()
    return dict(fwd_grouped=fwd_grouped, fwd_shared=fwd_shared, bwd_grouped=bwd_grouped, bwd_shared=bwd_shared), bytes_


def copy_rate(torch):
    a = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(10):
        s.record()
        b.copy_(a)
        t.record()
        t.synchronize()
        best = min(best, s.elapsed_time(t) / 1e3)
    return 2 * a.numel() / best   # bytes read + written per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="a few launches of each variant (run under rocprofv3)")
    ap.add_argument("--summarize", metavar="DIR")
    ap.add_argument("--out", metavar="DIR")
    ap.add_argument("--group", action="append", default=[])
    a = ap.parse_args()
    if a.group:
        GROUPS.clear()
        for g in a.group:
            name, d_in, outs = g.split(":")
            GROUPS[name] = (int(d_in), [int(v) for v in outs.split(",")])
    if a.summarize:
        summarize(a.summarize)
        return
    import torch
    if a.trace:
        for name in GROUPS:
            fns, _ = build(name)
            for _ in range(10):
                for k in ("fwd_grouped", "fwd_shared", "bwd_grouped", "bwd_shared"):
                    fns[k]()
            torch.cuda.synchronize()
        return
    bw = copy_rate(torch)
    print(f"copy rate {bw / 1e12:.2f} TB/s (512 MiB device-to-device, read + write)")
    res = {"copy_TBps": bw / 1e12, "T": T, "r": R, "groups": {}}
    for name in GROUPS:
        fns, bytes_ = build(name)
        times = {k: [] for k in fns}
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for rnd in range(a.warmup + a.rounds):
            for pair in (("fwd_grouped", "fwd_shared"), ("bwd_grouped", "bwd_shared")):
                order = pair if rnd % 2 == 0 else pair[::-1]   # alternate which variant goes first
                for k in order:
                    s.record()
                    for _ in range(a.reps):
                        fns[k]()
                    t.record()
                    t.synchronize()
                    if rnd >= a.warmup:
                        times[k].append(s.elapsed_time(t) * 1e3 / a.reps)
        res["groups"][name] = {}
        print(f"\n{name}: {GROUPS[name][1]} from {GROUPS[name][0]}, T = {T}, r = {R}, bf16")
        for k, v in times.items():
            med, lo, hi = statistics.median(v), min(v), max(v)
            floor_us = bytes_[k] / bw * 1e6
            res["groups"][name][k] = dict(median_us=med, min_us=lo, max_us=hi, bytes=bytes_[k], copy_rate_floor_us=floor_us,
                                          fraction_of_floor=floor_us / med)
            print(f"  {k:12s} median {med:7.1f} us  (min {lo:7.1f}, max {hi:7.1f})  bytes {bytes_[k] / 1e6:6.1f} MB  "
                  f"floor {floor_us:6.1f} us  -> {100 * floor_us / med:5.1f} % of the copy rate")
        for d in ("fwd", "bwd"):
            g, sh = res["groups"][name][d + "_grouped"]["median_us"], res["groups"][name][d + "_shared"]["median_us"]
            res["groups"][name][d + "_speedup"] = g / sh
            print(f"  {d}: shared / grouped = {sh / g:.3f} (bytes {bytes_[d + '_shared'] / bytes_[d + '_grouped']:.3f})")
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "shared_input_timing.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
