#!/usr/bin/env python3
"""Weight-gradient partial sums (skinny_tn.hip) in f16 on the LDS-DMA kernels against the generic kernel they replace and
against bf16 on the same kernels.

Per row, through the C ABI (no Python wrapper in the timed region), HIP events around every call of the PARTIAL phase alone
(sow_backward_ex / sow_backward_group with SOW_BWD_WEIGHTS_PARTIAL; h_save and the dh of the data phase are prepared once per
buffer copy, outside the timed region):
  f16      the streaming dispatch: tn_partial_dma_wide_kernel<f16> for a single layer, tn_partial_rows_kernel<f16> for the
           deferred group (SOW_BWD_GROUP_SLABS);
  f16_gen  the same call under NO_F16_TN=1: tn_partial_kernel<f16>, one launch per layer -- the launches before the f16 forms;
  bf16     the same shapes in bf16 (the plain symbols of the same kernels).
The variants alternate call by call in one process; WARM warm-up calls, then REPEATS windows of TIMED calls each: the figure
of a variant is the median of the window medians, its spread the distance between the largest and the smallest window median.
Every call takes the next copy of x / dY / h / workspace, rotating over more than 256 MiB, so that the token rows come from
HBM as they do in a training step.

  python tools/f16_tn_bench.py [--out profiles/f16_weight_gradients.txt] [--rows 3,4] [--bf16-first]
  python tools/f16_tn_bench.py --trace      (a short run of three rows for rocprofv3 --kernel-trace --stats)
"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from sow_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
BF16, F16 = torch.bfloat16, torch.float16
CODE = {BF16: _lib.BF16, F16: _lib.F16}
WARM, TIMED, REPEATS = 3, 24, 3
VARIANTS = (("f16", F16, 0), ("f16_gen", F16, 1), ("bf16", BF16, 0))     # (name, dtype, NO_F16_TN)
BLOCK = [(512, 512)] * 4 + [(512, 1376)] * 2 + [(1376, 512)]            # the seven projections of a llama_60m decoder block
# (label, T, [(d_in, d_out), ...], r): more than one layer = one deferred group
ROWS = ([("llama_60m block", 32768, BLOCK, 50)]
        + [(f"{di}->{do}", 32768, [(di, do)], 50) for di, do in ((512, 512), (512, 1376), (1376, 512), (768, 768))]
        + [("512->512", T, [(512, 512)], 50) for T in (1024, 4096, 8192)]
        + [(f"{di}->{do}", 1024, [(di, do)], 8) for di, do in ((4096, 4096), (4096, 11008))])


def _p(t):
    return None if t is None else t.data_ptr()


class Row:
    """The buffers of one row in one dtype: `copies` sets of (x, dY, h_save, workspace with dh) per layer."""

    def __init__(self, T, shapes, r, dtype):
        lib = _lib.load()
        self.T, self.shapes, self.r, self.dtype, self.dt = T, shapes, r, dtype, CODE[dtype]
        per_copy = sum(T * (di + do) * 2 for di, do in shapes)
        self.copies = max(2, -(-288 * 1024 * 1024 // per_copy))
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *s, std: (torch.randn(*s, device=DEV, dtype=torch.float32, generator=g) * std).to(dtype)   # noqa: E731
        st = torch.cuda.current_stream().cuda_stream
        self.layers = []
        for di, do in shapes:
            A, B = rnd(di, r, std=0.05), rnd(r, do, std=0.05)
            dA, dB = torch.empty(di, r, device=DEV, dtype=dtype), torch.empty(r, do, device=DEV, dtype=dtype)
            nws = lib.sow_workspace_bytes(T, di, do, r, 0, _lib.ACC_NONE, self.dt)
            nfw = lib.sow_forward_workspace_bytes(T, di, do, r, 0, _lib.ACC_NONE, self.dt)
            fws = torch.empty(nfw, device=DEV, dtype=torch.uint8) if nfw else None
            sets = []
            scratch_y = torch.empty(T, do, device=DEV, dtype=dtype)
            scratch_dx = torch.empty(T, di, device=DEV, dtype=dtype)
            for _ in range(self.copies):
                x, dy = rnd(T, di, std=1.0), rnd(T, do, std=1.0)
                h = torch.empty(T * 64, device=DEV, dtype=dtype)
                ws = torch.empty(nws, device=DEV, dtype=torch.uint8)
                _lib.check(lib.sow_forward(_p(x), _p(A), _p(B), None, None, None, _p(scratch_y), _p(h), T, di, do, r, 0,
                                           _lib.ACC_NONE, 0.5, self.dt, _p(fws), nfw, st), "sow_forward")
                _lib.check(lib.sow_backward_ex(_p(dy), _p(x), _p(h), _p(A), _p(B), None, None, _p(scratch_dx), _p(dA), _p(dB),
                                               None, T, di, do, r, 0, _lib.ACC_NONE, 0.5, 0.0, self.dt, _p(ws), nws,
                                               _lib.BWD_DATA, st), "sow_backward_ex(DATA)")
                sets.append((x, dy, h, ws))
            torch.cuda.synchronize()
            self.layers.append(dict(di=di, do=do, A=A, B=B, dA=dA, dB=dB, dx=scratch_dx, sets=sets, nws=nws))
        # the grouped call's argument arrays, one per copy
        self.args = []
        if len(shapes) > 1:
            for k in range(self.copies):
                arr = (_lib.LayerArgs * len(shapes))()
                for i, L in enumerate(self.layers):
                    x, dy, h, ws = L["sets"][k]
                    arr[i] = _lib.LayerArgs(x=_p(x), A=_p(L["A"]), B=_p(L["B"]), acc_down=None, acc_up=None, bias=None, y=_p(dy),
                                            h_save=_p(h), dy=_p(dy), dx=_p(x), dA=_p(L["dA"]), dB=_p(L["dB"]), dbias=None, T=T,
                                            d_in=L["di"], d_out=L["do"], r_live=r, r_acc=0, acc_kind=_lib.ACC_NONE, scale=0.5,
                                            grad_beta=0.0, workspace=_p(ws), workspace_bytes=L["nws"])
                self.args.append(arr)

    def call(self, j):
        lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
        k = j % self.copies
        if self.args:
            rc = lib.sow_backward_group(self.args[k], len(self.shapes), self.dt,
                                        _lib.BWD_WEIGHTS_PARTIAL | _lib.BWD_GROUP_SLABS, st)
            _lib.check(rc, "sow_backward_group(PARTIAL | GROUP_SLABS)")
            return
        L = self.layers[0]
        x, dy, h, ws = L["sets"][k]
        rc = lib.sow_backward_ex(_p(dy), _p(x), _p(h), _p(L["A"]), _p(L["B"]), None, None, _p(L["dx"]), _p(L["dA"]), _p(L["dB"]), None,
                                 self.T, L["di"], L["do"], self.r, 0, _lib.ACC_NONE, 0.5, 0.0, self.dt, _p(ws), L["nws"],
                                 _lib.BWD_WEIGHTS_PARTIAL, st)
        _lib.check(rc, "sow_backward_ex(PARTIAL)")

    def plan(self):
        """Row-owner plan of the grouped call under the current switches (single layers: 0)."""
        if not self.args:
            return 0
        return _lib.load().sow_backward_group_plan(self.args[0], len(self.shapes), self.dt,
                                                   _lib.BWD_WEIGHTS_PARTIAL | _lib.BWD_GROUP_SLABS, None)


def _set(off):
    _lib.check(_lib.load().sow_set_switch(b"NO_F16_TN", off), "sow_set_switch")


def measure(rows):
    """rows: {dtype: Row}.  {variant: (median of the window medians, spread of the window medians)} in us."""
    def call(v, j):
        name, dtype, off = v
        _set(off)
        rows[dtype].call(j)

    for j in range(WARM):
        for v in VARIANTS:
            call(v, j)
    torch.cuda.synchronize()
    meds = {v[0]: [] for v in VARIANTS}
    j = 0
    for _ in range(REPEATS):
        times = {v[0]: [] for v in VARIANTS}
        for _ in range(TIMED):
            for v in VARIANTS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(v, j)
                e1.record()
                e1.synchronize()
                times[v[0]].append(e0.elapsed_time(e1) * 1e3)
            j += 1
        for v in VARIANTS:
            meds[v[0]].append(statistics.median(times[v[0]]))
    _set(-1)
    return {k: (statistics.median(m), max(m) - min(m)) for k, m in meds.items()}


def sweep(out_path, only=None, bf16_first=False):
    lines = [f"# tools/f16_tn_bench.py on {torch.cuda.get_device_name(0)}; sow_version {_lib.load().sow_version()}",
             f"# us per call of the weight-gradient PARTIAL phase: median of {REPEATS} window medians ({TIMED} calls each, {WARM} "
             "warm-up), +- = spread of the window medians; x / dY / h / dh rotate over > 256 MiB",
             "# f16 = LDS-DMA kernels (single layer: tn_partial_dma_wide_kernel<f16>; block: tn_partial_rows_kernel<f16>, one "
             "launch); f16_gen = NO_F16_TN=1 (tn_partial_kernel<f16>, one launch per layer); bf16 = the same kernels in bf16",
             f"{'row':>16} {'T':>6} {'r':>3} | {'f16':>14} {'f16_gen':>14} {'bf16':>14} | {'gen/f16':>7} {'f16/bf16':>8}"]
    print("\n".join(lines), flush=True)
    if bf16_first:
        lines.append("# the bf16 buffers of every row allocated BEFORE the f16 ones (default: after)")
    for i, (label, T, shapes, r) in enumerate(ROWS):
        if only is not None and i not in only:
            continue
        rows = {dt: Row(T, shapes, r, dt) for dt in ((BF16, F16) if bf16_first else (F16, BF16))}
        if len(shapes) > 1:
            assert rows[F16].plan() == 1 and rows[BF16].plan() == 1
        m = measure(rows)
        cell = lambda v: f"{v[0]:8.1f}+-{v[1]:<4.1f}"   # noqa: E731
        line = (f"{label:>16} {T:6d} {r:3d} | {cell(m['f16'])} {cell(m['f16_gen'])} {cell(m['bf16'])} | "
                f"{m['f16_gen'][0] / m['f16'][0]:7.2f} {m['f16'][0] / m['bf16'][0]:8.3f}")
        print(line, flush=True)
        lines.append(line)
        del rows
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def trace():
    """20 calls of every variant of three rows, for rocprofv3 --kernel-trace --stats (kernel names tell the variants apart)."""
    for label, T, shapes, r in (ROWS[0], ROWS[1], ROWS[6]):
        rows = {dt: Row(T, shapes, r, dt) for dt in (F16, BF16)}
        for j in range(20):
            for name, dtype, off in VARIANTS:
                _set(off)
                rows[dtype].call(j)
        torch.cuda.synchronize()
        _set(-1)
        del rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--rows", default=None, help="comma-separated indices into ROWS (default: all)")
    ap.add_argument("--bf16-first", action="store_true", help="allocate the bf16 buffers of a row before the f16 ones")
    a = ap.parse_args()
    if a.trace:
        trace()
    else:
        sweep(a.out, None if a.rows is None else {int(v) for v in a.rows.split(",")}, a.bf16_first)
