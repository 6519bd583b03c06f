"""Per-kernel summary of a `rocprofv3 --kernel-trace` database of tools/wide_rank_trace.py (T = 32768, d_in = d_out = 2048,
r = 200, bf16), with each new kernel's time against max(bytes / 8 TB/s, flops / 2.5 PF).

    python tools/wide_rank_stats.py out_wide/run_results.db out_generic/run_results.db
"""
import sqlite3
import statistics
import sys

T, D, R, RP = 32768, 2048, 200, 256
HBM, MFMA = 8e12, 2.5e15
# bytes and flops of one launch at the traced shape
BOUNDS = {
    # x (or dY) read, y (or dX) written, h (or dh) written; two products of 2 T D r flops
    "chain_wide_kernel": (2 * T * D * 2 + T * R * 2, 2 * 2 * T * D * R),
    # x, dY, h, dh read once; fp32 slab partials (8 slabs) written; MFMA work on r_pad = 256 columns
    "tnw_partial_kernel": (2 * T * D * 2 + 2 * T * R * 2 + 8 * 2 * D * RP * 4 + 8 * D * 4, 2 * T * 2 * D * RP),
    # partials read, dA / dB / dbias written
    "tnw_reduce_kernel": (8 * 2 * D * RP * 4 + 2 * D * R * 2, 0),
    # A and B read, packed copies written
    "wide_pack_kernel": (2 * D * R * 2 + 2 * D * RP * 2, 0),
}


def short(name):
    base = name.split("(")[0]
    for k in BOUNDS:
        if k in base:
            return k
    return base[:70]


def load(path):
    con = sqlite3.connect(path)
    rows = con.execute("select name, duration from kernels").fetchall()
    per = {}
    for name, dur in rows:
        per.setdefault(short(name), []).append(dur / 1000.0)
    return per


def report(title, per, steps):
    print(f"== {title}")
    print(f"{'kernel':72s} {'calls':>6s} {'median us':>10s} {'us/step':>9s}  bound")
    total = 0.0
    for k, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        if "sow" not in k and k not in BOUNDS:
            continue        # torch's own kernels (input generation, allocation)
        med = statistics.median(v)
        step = sum(v) / steps
        total += step
        b = ""
        if k in BOUNDS:
            nb, nf = BOUNDS[k]
            th, tf = nb / HBM * 1e6, nf / MFMA * 1e6
            which = "HBM" if th >= tf else "MFMA"
            b = f"{max(th, tf):6.1f} us ({which}: {nb / 1e6:.0f} MB, {nf / 1e9:.1f} GFLOP)  -> {max(th, tf) / med * 100:4.0f} %"
        print(f"{k:72s} {len(v):6d} {med:10.1f} {step:9.1f}  {b}")
    print(f"{'sum of the layer kernels per step':72s} {'':6s} {'':10s} {total:9.1f}")
    return total


if __name__ == "__main__":
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 23
    a = report("fused wide kernels (NO_WIDE_CHAIN=0)", load(sys.argv[1]), steps)
    b = report("generic composition (NO_WIDE_CHAIN=1)", load(sys.argv[2]), steps)
    print(f"forward + backward: {b:.1f} us -> {a:.1f} us per step ({b / a:.2f}x)")
