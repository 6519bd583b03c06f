"""CPU table of the weight-gradient selector (skinny_tn.hip: tn_shape_kernel / pick_tn / tn_blocks / tn_pick_slabs; api.hip:
pick_tn_wide_rank and the grouped arms of backward_group_impl), through the debug export sow_debug_tn_pick, which is declared
here and nowhere else.  The export builds fake-pointer operands through the real plan_ws / tn_params / group_rows path and
launches nothing.

tests/golden/host_tn_pick.json.gz was recorded BEFORE the selector existed: from a scratch build of the commit before it, with
the same export written on top of that commit's own launch_tn / backward_impl / backward_group_impl conditions, in their order
(`python tests/test_host_tn_pick_cpu.py --record` with SOW_AMD_LIB pointing at such a build).  Every row is asserted; none is
skipped.  A row: kernel (TnKernel of kernels.hpp), blocks of work, ns and slab_len of the x operand and of the dY operand,
bytes of the plan's two partial regions, and whether the layer shares a grouped launch.

The second assertion is what the selector is for: the partials the chosen kernel writes fit the regions plan_ws reserved.  A
kernel's block b maps to (slab, first column group) with `groups` 64-column groups per block; one group of one slab is a
[64][64] fp32 tile.  The kernels skip groups past the operand's last one (ncg not a multiple of `groups`) and the quad kernel's
padding blocks (slab >= ns) leave before they touch memory, so an operand's footprint is ns x ncg tiles; the test recomputes
tn_blocks from (kernel, ns, ncg) with the padding counted, holds it equal to the export's figure, and holds the footprint
within the region.  Wide-rank rows: the three regions of tnw_partial_bytes within pw_bytes."""
import ctypes
import gzip
import itertools
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sow_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_tn_pick.json.gz")
KERNELS = ("none", "generic", "dma", "dma_wide", "rows", "f32_x3", "f32_exact", "f32_wide", "f32_quad", "wide_rank", "gemm_pair")
GROUPS = {"generic": 1, "dma": 1, "dma_wide": 2, "f32_x3": 1, "f32_exact": 1, "f32_wide": 2, "f32_quad": 4}
SLAB_MULT = {"generic": 1, "dma": 16, "dma_wide": 16, "rows": 32, "f32_x3": 8, "f32_exact": 8, "f32_wide": 8, "f32_quad": 32}
DTYPES = {"f32": _lib.F32, "bf16": _lib.BF16, "f16": _lib.F16}
TS = (0, 1, 511, 512, 1000, 1024, 4095, 4096, 32768)
WIDTHS = ((512, 512), (512, 1376), (1376, 512), (192, 192), (128, 192), (100, 36), (102, 36), (2048, 5461))
RANKS = (8, 50, 63, 64, 66, 200)
SINGLE = ("TN_NARROW", "F32_EXACT", "NO_TN_F32Q", "NO_F16_TN", "NO_TN_ROWS", "NO_GROUPED", "NO_WIDE_CHAIN", "NO_RAGGED")
SWITCH_SETS = [()] + [(s,) for s in SINGLE] + [("F32_EXACT", "TN_NARROW")]
BLOCK = [(512, 512)] * 4 + [(512, 1376)] * 2 + [(1376, 512)]    # the seven projections of a decoder block
PHASES = {"deferred": _lib.BWD_WEIGHTS_PARTIAL | _lib.BWD_GROUP_SLABS, "full": _lib.BWD_DATA | _lib.BWD_WEIGHTS,
          "partial": _lib.BWD_WEIGHTS_PARTIAL}
FAKE = 1 << 20
TILE = 64 * 64 * 4


def _pick():
    f = _lib.load().sow_debug_tn_pick
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                  ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
    return f


def _call(f, shapes, T, r, dbias, dt, phases, misalign):
    n = len(shapes)
    d_in, d_out = (ctypes.c_int * n)(*[s[0] for s in shapes]), (ctypes.c_int * n)(*[s[1] for s in shapes])
    out = (ctypes.c_int64 * (9 * n))()
    _lib.check(f(n, T, d_in, d_out, r, dbias, dt, phases, misalign, out), "sow_debug_tn_pick")
    return [list(out[9 * i:9 * i + 9]) for i in range(n)]


def _table():
    """{key: rows}: single layers over the whole grid under the defaults (every pointer misaligned in turn) and under every
    switch set (aligned), then the decoder block as a group."""
    f, table = _pick(), {}
    for sw in SWITCH_SETS:
        with _lib.switch(**{s: 1 for s in sw}):
            for (dn, dt), T, (d_in, d_out), r, dbias in itertools.product(DTYPES.items(), TS, WIDTHS, RANKS, (0, 1)):
                for mis in ((0, 1, 2, 4, 8) if not sw else (0,)):
                    key = f"{'+'.join(sw) or 'default'}|{dn}|{T}|{d_in}x{d_out}|r{r}|b{dbias}|m{mis}"
                    table[key] = _call(f, [(d_in, d_out)], T, r, dbias, dt, PHASES["full"], mis)
            for (dn, dt), T, (pn, ph), dbias in itertools.product(DTYPES.items(), TS, PHASES.items(), (0, 1)):
                key = f"{'+'.join(sw) or 'default'}|{dn}|{T}|block|{pn}|b{dbias}"
                table[key] = _call(f, BLOCK, T, 50, dbias, dt, ph, 0)
    return table


def _group_plan(dt, T, phases, dbias):
    """sow_backward_group_plan on the same block (its own fake layers, as tests/test_host_f16_tn_cpu.py)."""
    lib = _lib.load()
    arr = (_lib.LayerArgs * len(BLOCK))()
    for i, (d_in, d_out) in enumerate(BLOCK):
        ws = lib.sow_workspace_bytes(T, d_in, d_out, 50, 0, _lib.ACC_NONE, dt)
        arr[i] = _lib.LayerArgs(x=FAKE, A=FAKE, B=FAKE, y=FAKE, h_save=FAKE, dy=FAKE, dx=FAKE, dA=FAKE, dB=FAKE,
                                dbias=FAKE if dbias else None, T=T, d_in=d_in, d_out=d_out, r_live=50, r_acc=0,
                                acc_kind=_lib.ACC_NONE, scale=1.0, grad_beta=0.0, workspace=FAKE, workspace_bytes=ws + 256)
    slabs = (ctypes.c_int * (2 * len(BLOCK)))()
    return lib.sow_backward_group_plan(arr, len(BLOCK), dt, phases, slabs), list(slabs)


def _shapes(key):
    part = key.split("|")
    if part[3] == "block":
        return BLOCK, 50, int(part[5][1:])
    d_in, d_out = part[3].split("x")
    return [(int(d_in), int(d_out))], int(part[4][1:]), int(part[5][1:])


def _fits(key, T, shape, r, dbias, row):
    """The partials of the row's kernel lie inside the row's regions; the export's block count is tn_blocks of (kernel, ns, ncg)."""
    kernel, blocks, ns0, slab0, ns1, slab1, reg0, reg1, _ = row
    name = KERNELS[kernel]
    ncg = [(d + 63) // 64 for d in shape]
    if name == "none":
        assert T == 0 and row == [0] * 9, (key, row)
        return
    if name in ("wide_rank", "gemm_pair"):
        assert r > 64 and reg1 == 0, (key, row)
        if name == "gemm_pair":
            assert blocks == 0, (key, row)
            return
        r_pad, al = (r + 63) // 64 * 64, lambda b: (b + 255) // 256 * 256
        assert blocks == ns0 * sum(ncg) and ns0 == ns1 >= 1 and slab0 % 64 == 0 and ns0 * slab0 >= T, (key, row)
        need = sum(al(ns0 * c * 64 * r_pad * 4) for c in ncg) + al(ns0 * ncg[1] * 64 * 4)
        assert need <= reg0, (key, row, need)
        return
    assert r <= 64, (key, row)
    for ns, slab in ((ns0, slab0), (ns1, slab1)):
        assert ns >= 1 and slab % SLAB_MULT[name] == 0 and ns * slab >= T > (ns - 1) * slab, (key, row)
    if name == "rows":
        assert blocks == ns0 * ((ncg[0] + 15) // 16) + ns1 * ((ncg[1] + 15) // 16), (key, row)
    else:
        g, launched = GROUPS[name], (ns0 + 7) // 8 * 8 if name == "f32_quad" else ns0
        assert ns0 == ns1 and slab0 == slab1, (key, row)
        assert blocks == sum((c + g - 1) // g for c in ncg) * launched, (key, row)
    for ns, c, reg in ((ns0, ncg[0], reg0), (ns1, ncg[1], reg1)):
        assert ns * c * TILE <= reg, (key, row, ns * c * TILE)


def _golden():
    with gzip.open(FIXTURE, "rt") as fh:
        return json.load(fh)


def test_every_row_matches_the_recording_and_fits_its_plan():
    golden, got = _golden(), _table()
    assert sorted(got) == sorted(golden), "the grid of this test and the recorded grid differ"
    bad = [(k, golden[k], got[k]) for k in golden if got[k] != golden[k]]
    assert not bad, f"{len(bad)} of {len(golden)} rows differ; the first: {bad[:5]}"
    seen = set()
    for key, rows in got.items():
        shapes, r, dbias = _shapes(key)
        for shape, row in zip(shapes, rows):
            _fits(key, int(key.split("|")[2]), shape, r, dbias, row)
            seen.add(KERNELS[row[0]])
    assert seen == set(KERNELS), f"the grid reaches {sorted(seen)} only"


def test_the_recording_itself_fits_its_plan():
    """The soundness property held before the selector: the recorded rows (the commit before it) pass the same check."""
    for key, rows in _golden().items():
        shapes, r, dbias = _shapes(key)
        for shape, row in zip(shapes, rows):
            _fits(key, int(key.split("|")[2]), shape, r, dbias, row)


def test_block_rows_agree_with_the_group_plan():
    """sow_backward_group_plan on the seven-layer block: the rows flag and every slab count the export reports."""
    f = _pick()
    for sw in SWITCH_SETS:
        with _lib.switch(**{s: 1 for s in sw}):
            for dt, T, ph in itertools.product(DTYPES.values(), TS[1:], PHASES.values()):
                rows, slabs = _group_plan(dt, T, ph, 0)
                got = _call(f, BLOCK, T, 50, 0, dt, ph, 0)
                assert rows == int(all(KERNELS[g[0]] == "rows" for g in got)), (sw, dt, T, ph)
                assert rows == int(any(KERNELS[g[0]] == "rows" for g in got)), (sw, dt, T, ph)
                assert slabs == [v for g in got for v in (g[2], g[4])], (sw, dt, T, ph, slabs)


def test_switches_are_restored():
    lib = _lib.load()
    for s in SINGLE:
        if "SOW_AMD_" + s not in os.environ:
            assert lib.sow_get_switch(s.encode()) == -1


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: SOW_AMD_LIB=<a build with sow_debug_tn_pick> python tests/test_host_tn_pick_cpu.py --record")
    table = _table()
    with open(FIXTURE, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as fh:
        fh.write(json.dumps(table, separators=(",", ":"), sort_keys=True).encode())
    print(f"recorded {len(table)} keys, version {_lib.load().sow_version()}, {os.path.getsize(FIXTURE)} bytes -> {FIXTURE}")
