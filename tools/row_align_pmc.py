#!/usr/bin/env python3
"""Workload for the L2 request counters of the chain kernel's row alignment (profiles/row_align_ab.txt): the four 1376-wide
launches of the headline step, in a fixed order, twice (the second pass is the one to read):
  fwd gate+up 2x(512->1376), fwd down 1376->512, bwd gate+up, bwd down       (T = 32768, r = 50, bf16)
    rocprofv3 --pmc TCC_REQ_sum TCC_READ_sum TCC_WRITE_sum -f csv -d D -- python3 tools/row_align_pmc.py
    SOW_AMD_NO_ROW_ALIGN=1 rocprofv3 ... (same)
    python3 tools/row_align_pmc.py --summarize D"""
import collections
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LABELS = ["fwd gate+up", "fwd down", "bwd gate+up", "bwd down"]


def summarize(d):
    f = glob.glob(d + "/**/*counter_collection.csv", recursive=True)[0]
    per = collections.OrderedDict()
    for r in csv.DictReader(open(f)):
        if "chain2_kernel" in r["Kernel_Name"]:
            per.setdefault(int(r["Dispatch_Id"]), {})[r["Counter_Name"]] = float(r["Counter_Value"])
    last = [per[k] for k in sorted(per)][-4:]
    for label, c in zip(LABELS, last):
        print(f"{label:12s} " + " ".join(f"{k}={v:.0f}" for k, v in sorted(c.items())))


def main():
    import torch
    from sow_amd import _lib, ops
    T, r, dev = 32768, 50, "cuda"
    g = torch.Generator(device=dev).manual_seed(0)

    def layer(di, do):
        x = torch.randn(T, di, device=dev, generator=g).bfloat16()
        dy = torch.randn(T, do, device=dev, generator=g).bfloat16()
        A = (torch.randn(di, r, device=dev, generator=g) * 0.05).bfloat16()
        B = (torch.randn(r, do, device=dev, generator=g) * 0.05).bfloat16()
        return ops.LayerCall(x, A, B, scale=0.5, dy2=dy, dx=torch.empty_like(x), out=(torch.zeros_like(A), torch.zeros_like(B), None))
    gate_up = ops.LayerGroup([layer(512, 1376), layer(512, 1376)])
    down = ops.LayerGroup([layer(1376, 512)])
    for _ in range(2):
        gate_up.forward()
        down.forward()
        gate_up.backward(_lib.BWD_DATA)
        down.backward(_lib.BWD_DATA)
    torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        main()
