"""Per-kernel summary of `rocprofv3 --kernel-trace` databases of tools/autocast_bench.py (one per variant, --only <variant>;
T = 32768, r = 50, llama_60m stack): launches per step, median us per launch and us per step of every library kernel, side
by side.

    python tools/autocast_stats.py STEPS bf16=prof_bf16/run_results.db mixed=prof_mixed/run_results.db ...

STEPS = the steps_run figure the bench printed (every variant runs the same number of steps).
"""
import sqlite3
import statistics
import re
import sys



_TYPES = (("DF16b", "__bf16"), ("DF16_", "_Float16"), ("f", "float"))


def demangle(name):
    """sow::<kernel><type, ...> of a mangled kernel name (older c++filt versions do not know the __bf16 code DF16b)."""
    m = re.match(r"_ZN3sow(\d+)", name)
    if not m:
        return name
    n = int(m.group(1))
    rest = name[m.end():]
    base, rest = rest[:n], rest[n:]
    args = []
    if rest.startswith("I"):
        rest = rest[1:]
        while rest and rest[0] != "E":
            for code, ty in _TYPES:
                if rest.startswith(code):
                    args.append(ty)
                    rest = rest[len(code):]
                    break
            else:
                break
    return f"sow::{base}" + (f"<{', '.join(args)}>" if args else "")


def short(name):
    base = demangle(name).split("(")[0].replace("void ", "").strip()
    return base[:60]


def load(path):
    rows = sqlite3.connect(path).execute("select name, duration from kernels").fetchall()
    per = {}
    for name, dur in rows:
        name = demangle(name)
        if "sow::" in name:     # the library's kernels; torch's own (input generation, setup copies) are left out
            per.setdefault(short(name), []).append(dur / 1000.0)
    return per


def main():
    steps = int(sys.argv[1])
    variants = [a.split("=", 1)[0] for a in sys.argv[2:]]
    data = [load(a.split("=", 1)[1]) for a in sys.argv[2:]]
    names = sorted(set().union(*data), key=lambda k: -max(sum(d.get(k, [])) for d in data))
    head = f"{'kernel':60s}" + "".join(f" | {v + ': calls/step  med us  us/step':>34s}" for v in variants)
    print(head)
    print("-" * len(head))
    totals = [0.0] * len(data)
    for k in names:
        line = f"{k:60s}"
        for i, d in enumerate(data):
            v = d.get(k)
            if not v:
                line += f" | {'-':>34s}"
                continue
            per_step = sum(v) / steps
            totals[i] += per_step
            line += f" | {len(v) / steps:14.1f} {statistics.median(v):8.1f} {per_step:10.1f}"
        print(line)
    print("-" * len(head))
    print(f"{'sum of the library kernels per step (us)':60s}" + "".join(f" | {t:34.1f}" for t in totals))


if __name__ == "__main__":
    main()
