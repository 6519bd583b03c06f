"""CPU tests of the short-batch entry points on E4M3 / MXFP4 codes read in place (sow_forward_short_codes /
sow_backward_short_codes, include/sow_amd.h): the C-ABI surface, the two workspace queries, every host-side refusal -- decided
before anything is launched or dereferenced (fake pointers, as tests/test_host_short_rows_cpu.py) --, the per-format dispatch rule
against the table in its docstring, and the second opt-in (sow_amd.short_codes)."""
import ctypes
import os
import re

import pytest

from sow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = _lib.F32, _lib.BF16, _lib.F16
PF, NATIVE = _lib.PARAM_F32, _lib.ACC_NATIVE
NONE, LOWRANK, DENSE, FP8, FP4 = _lib.ACC_NONE, _lib.ACC_LOWRANK, _lib.ACC_DENSE, _lib.ACC_DENSE_FP8, _lib.ACC_DENSE_FP4
ERR_NULL, ERR_SHAPE, ERR_DTYPE, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -3, -5, -6
NAMES = ("sow_forward_short_codes_workspace_bytes", "sow_short_codes_workspace_bytes", "sow_forward_short_codes", "sow_backward_short_codes")
# d_in a multiple of 32 in every shape: both formats admit them
SHAPES = ((768, 768, 8), (768, 3072, 8), (3072, 768, 8), (4096, 4096, 50), (4096, 11008, 64), (11008, 4096, 2), (288, 520, 63), (512, 1376, 50))
TS = (1, 33, 64, 65, 100, 129, 1024)


def test_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "sow_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert len(re.findall(r"\b(?:size_t|int)\s+" + name + r"\s*\(", header)) == 1, name
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name), name
    for name in NAMES[:2]:
        assert _lib.SIGNATURES[name][0] is ctypes.c_size_t and len(_lib.SIGNATURES[name][1]) == 6
        assert re.search(name + r"\s*\(\s*int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype\s*\)", header), name
    for name in NAMES[2:]:
        assert _lib.SIGNATURES[name][0] is ctypes.c_int and _lib.SIGNATURES[name][1][0] is ctypes.POINTER(_lib.LayerArgs)
        assert re.search(name + r"\s*\(\s*const sow_layer_args\* layers, int n, int dtype, void\* stream\s*\)", header), name
    assert _lib.load().sow_version() >= 125


def test_queries_are_positive_inside_the_admitted_set():
    lib = _lib.load()
    fq, q = lib.sow_forward_short_codes_workspace_bytes, lib.sow_short_codes_workspace_bytes
    for kind in (FP8, FP4):
        for d_in, d_out, r in SHAPES:
            for T in TS:
                for dt in (BF16, F16):
                    fw, full = fq(T, d_in, d_out, r, kind, dt), q(T, d_in, d_out, r, kind, dt)
                    base = lib.sow_workspace_bytes(T, d_in, d_out, r, 0, DENSE, dt)
                    assert fw > 0 and full > 0, (T, d_in, d_out, r, kind, dt)
                    # one buffer serves the forward, the data phase and the unchanged weight phases called with SOW_ACC_DENSE
                    assert full >= base and full >= fw, (T, d_in, d_out, r, kind, dt, fw, full, base)
                assert fq(T, d_in, d_out, r, kind, BF16) == fq(T, d_in, d_out, r, kind, F16)
            # more rows never need less, from one measured row count to the next.  (Not at EVERY T: the plan counts the row blocks,
            # so 129 rows -- three blocks -- plan fewer slabs than 100, and 65 fewer than 64, as in sow_short_workspace_bytes.)
            sizes = [q(T, d_in, d_out, r, kind, BF16) for T in (65, 128, 256, 512, 1024)]
            assert sizes == sorted(sizes), (d_in, d_out, r, kind, sizes)
        # the partials hold at least one slab of fp32 y and of fp32 h
        assert fq(1024, 768, 768, 8, kind, BF16) >= 1024 * (768 + 64) * 4
    # E4M3 takes widths that are multiples of 8 where MXFP4 wants whole blocks of d_in
    assert q(100, 264, 520, 8, FP8, BF16) > 0 and q(100, 264, 520, 8, FP4, BF16) == 0


OUTSIDE = [(100, 768, 768, 8, DENSE, BF16), (100, 768, 768, 8, NONE, BF16), (100, 768, 768, 8, LOWRANK, F16), (100, 768, 768, 8, 5, BF16),
           (0, 768, 768, 8, FP8, BF16), (1025, 768, 768, 8, FP8, BF16), (0, 768, 768, 8, FP4, F16), (1025, 768, 768, 8, FP4, BF16),
           (-1, 768, 768, 8, FP8, BF16), (100, 768, 768, 0, FP8, BF16), (100, 768, 768, 66, FP8, BF16), (100, 768, 768, 0, FP4, BF16),
           (100, 768, 768, 66, FP4, F16), (100, 768, 768, 8, FP8, F32), (100, 768, 768, 8, FP4, F32), (100, 768, 768, 8, FP8, BF16 | PF),
           (100, 768, 768, 8, FP4, F16 | PF | NATIVE), (100, 768, 768, 8, FP8, BF16 | PF | NATIVE), (100, 100, 768, 8, FP8, BF16),
           (100, 264, 768, 8, FP4, BF16), (100, 768, 516, 8, FP8, F16), (100, 768, 516, 8, FP4, F16), (100, 768, 768, 8, FP8, 7)]


def test_queries_are_zero_outside_the_admitted_set_and_pure():
    lib = _lib.load()
    inside = [(T, d_in, d_out, r, kind, dt) for T in TS for d_in, d_out, r in SHAPES[:3] for kind in (FP8, FP4) for dt in (BF16, F16)]
    for q in (lib.sow_forward_short_codes_workspace_bytes, lib.sow_short_codes_workspace_bytes):
        for a in OUTSIDE:
            assert q(*a) == 0, a
        first = [q(*a) for a in inside + OUTSIDE]
        for sw in (dict(NO_SKINNY=1), dict(NO_SKINNY=0), {}):
            with _lib.switch(**sw):
                assert [q(*a) for a in inside + OUTSIDE] == first
    # the queries of sow_forward_short / sow_backward_short keep answering 0 for the code kinds
    for q in (lib.sow_forward_short_workspace_bytes, lib.sow_short_workspace_bytes):
        assert q(100, 768, 768, 8, DENSE, BF16) > 0
        for kind in (FP8, FP4):
            for dt in (BF16, F16):
                assert q(100, 768, 768, 8, kind, dt) == 0


def _fake_layers(n, T=100, d_in=512, d_out=768, r=50, kind=FP8):
    """Layer descriptors with dummy non-null, 16-byte-aligned pointers that are never dereferenced: every call below must
    return from the host checks (a launch on this machine, or a read of one of these addresses, would not return a code)."""
    arr = (_lib.LayerArgs * n)()
    for i in range(n):
        a = arr[i]
        base = 0x10000000 * (i + 1)
        a.x, a.A, a.B, a.acc_down, a.bias, a.y = 0x1000000, base + 0x1000, base + 0x2000, base + 0x3000, base + 0x4000, base + 0x5000
        a.acc_up, a.h_save, a.dy, a.dx = base + 0x6000, base + 0x7000, base + 0x8000, base + 0x9000
        a.workspace, a.workspace_bytes = base + 0x100000, 1 << 30
        a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, kind, 0.5
    return arr


REFUSALS = [
    ("T=1025", dict(T=1025), BF16, ERR_UNSUPPORTED),
    ("T=-1", dict(T=-1), BF16, ERR_SHAPE),
    ("dense", dict(kind=DENSE), BF16, ERR_UNSUPPORTED),
    ("none", dict(kind=NONE), BF16, ERR_UNSUPPORTED),
    ("lowrank", dict(kind=LOWRANK), F16, ERR_UNSUPPORTED),
    ("unknown_kind", dict(kind=5), BF16, ERR_SHAPE),
    ("r=0", dict(r=0), BF16, ERR_SHAPE),
    ("r=66", dict(r=66), BF16, ERR_UNSUPPORTED),
    ("d_in=100", dict(d_in=100), BF16, ERR_UNSUPPORTED),
    ("d_out=516", dict(d_out=516), F16, ERR_UNSUPPORTED),
    ("param_f32", {}, BF16 | PF, ERR_UNSUPPORTED),
    ("param_f32_native", {}, F16 | PF | NATIVE, ERR_UNSUPPORTED),
    ("fp32", {}, F32, ERR_DTYPE),
    ("fp32_param_f32", {}, F32 | PF, ERR_DTYPE),
    ("unknown_dtype", {}, 7, ERR_DTYPE),
]


@pytest.mark.parametrize("entry", ["sow_forward_short_codes", "sow_backward_short_codes"])
@pytest.mark.parametrize("name,kw,dtype,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_are_decided_on_the_host(name, kw, dtype, code, entry):
    fn = getattr(_lib.load(), entry)
    assert fn(_fake_layers(1, **kw), 1, dtype, None) == code
    # one bad layer refuses the whole call, wherever it sits: nothing is launched for the layers ahead of it
    arr = _fake_layers(3)
    bad = _fake_layers(1, **kw)[0]
    for f in ("T", "d_in", "d_out", "r_live", "acc_kind"):
        setattr(arr[2], f, getattr(bad, f))
    assert fn(arr, 3, dtype, None) == code


@pytest.mark.parametrize("entry", ["sow_forward_short_codes", "sow_backward_short_codes"])
def test_format_widths_and_one_kind_per_call(entry):
    fn = getattr(_lib.load(), entry)
    # MXFP4 wants whole blocks of d_in; E4M3 takes the same width
    assert fn(_fake_layers(1, d_in=264, kind=FP4), 1, BF16, None) == ERR_UNSUPPORTED
    # two layers of different code kinds in one call, in either order
    for first, second in ((FP8, FP4), (FP4, FP8)):
        arr = _fake_layers(2, kind=first)
        arr[1].acc_kind = second
        assert fn(arr, 2, BF16, None) == ERR_UNSUPPORTED
    assert fn(_fake_layers(17), 17, BF16, None) == ERR_UNSUPPORTED     # n > 16
    assert fn(_fake_layers(17, kind=FP4), 17, F16, None) == ERR_UNSUPPORTED
    # and the plain entry point of the same direction keeps refusing the code kinds
    plain = getattr(_lib.load(), entry.replace("_codes", ""))
    for kind in (FP8, FP4):
        assert plain(_fake_layers(1, kind=kind), 1, BF16, None) == ERR_UNSUPPORTED


def test_workspace_alignment_and_the_switch():
    lib = _lib.load()
    fwd, bwd = lib.sow_forward_short_codes, lib.sow_backward_short_codes
    for kind in (FP8, FP4):
        need_f = lib.sow_forward_short_codes_workspace_bytes(100, 512, 768, 50, kind, BF16)
        need = lib.sow_short_codes_workspace_bytes(100, 512, 768, 50, kind, BF16)
        for fn, n in ((fwd, need_f), (bwd, need)):
            arr = _fake_layers(2, kind=kind)
            arr[1].workspace_bytes = n - 1
            assert fn(arr, 2, BF16, None) == ERR_WORKSPACE
            arr = _fake_layers(1, kind=kind)
            arr[0].workspace = None
            assert fn(arr, 1, F16, None) == ERR_WORKSPACE
        # the operands of sow_forward_short 16-byte aligned; codes and scales as the kernels load them (E4M3 codes 16, the rest 8)
        for field in ("x", "y", "A", "B", "bias", "h_save", "acc_down", "acc_up"):
            arr = _fake_layers(2, kind=kind)
            setattr(arr[1], field, getattr(arr[1], field) + 2)
            assert fwd(arr, 2, BF16, None) == ERR_UNSUPPORTED, (kind, field)
        for field in ("dy", "dx", "A", "B", "acc_down", "acc_up"):
            arr = _fake_layers(2, kind=kind)
            setattr(arr[1], field, getattr(arr[1], field) + 2)
            assert bwd(arr, 2, BF16, None) == ERR_UNSUPPORTED, (kind, field)
        for fn, fields in ((fwd, ("x", "y", "A", "B", "acc_down", "acc_up")), (bwd, ("dy", "dx", "A", "B", "acc_down", "acc_up"))):
            for field in fields:
                arr = _fake_layers(1, kind=kind)
                setattr(arr[0], field, None)
                assert fn(arr, 1, BF16, None) == ERR_NULL, (kind, field)
            assert fn(None, 1, BF16, None) == ERR_NULL
            assert fn(_fake_layers(1, kind=kind), -1, BF16, None) == ERR_SHAPE
            # nothing to do: SOW_OK without a launch
            assert fn(_fake_layers(3, T=0, kind=kind), 3, BF16, None) == 0
            assert fn(_fake_layers(1, kind=kind), 0, F16, None) == 0
            with _lib.switch(NO_SKINNY=1):
                assert fn(_fake_layers(1, kind=kind), 1, BF16, None) == ERR_UNSUPPORTED
                assert fn(_fake_layers(3, T=0, kind=kind), 3, BF16, None) == ERR_UNSUPPORTED
                assert fn(_fake_layers(1, kind=kind), 1, F32, None) == ERR_DTYPE
    assert lib.sow_get_switch(b"NO_SKINNY") in (-1, 0)


def test_short_codes_switch_nests_restores_and_is_inert_outside_short_rows():
    import sow_amd
    import torch
    from sow_amd import ops
    assert ops.short_codes_enabled() is False, "the default is off"
    with sow_amd.short_codes():
        assert ops.short_codes_enabled() is True and ops.short_rows_enabled() is False
        with sow_amd.short_codes(False):
            assert ops.short_codes_enabled() is False
        assert ops.short_codes_enabled() is True
    assert ops.short_codes_enabled() is False
    assert sow_amd.set_short_codes(True) is False
    try:
        with pytest.raises(RuntimeError):
            with sow_amd.short_codes(False):
                raise RuntimeError("leave the block")
        assert ops.short_codes_enabled() is True
        # on, but outside short_rows: nothing is admitted, decided before a tensor is looked at
        assert ops.short_codes_admits(None, None, None, None, None, None) is False
    finally:
        assert sow_amd.set_short_codes(False) is True
    with pytest.raises(ValueError):
        sow_amd.set_short_codes(1)
    # inside short_rows alone the codes path stays off too; with both on the call is judged (a CPU tensor is no candidate)
    x = torch.zeros(100, 768, dtype=torch.bfloat16)
    with sow_amd.short_rows():
        assert ops.short_codes_admits(None, None, None, None, None, None) is False
        with sow_amd.short_codes():
            assert ops.short_codes_admits(x, x, x, None, None, None) is False
    assert ops.short_rows_enabled() is False and ops.short_codes_enabled() is False


@pytest.mark.parametrize("name", ["fp8_e4m3", "mxfp4"])
def test_pays_short_equals_the_table_in_its_docstring(name):
    """The docstring of a format's rule carries one line per measured shape, `d_in->d_out: T <= N` (N = 0: never).  The rule is exactly
    that table: true inside it, false at every other shape and row count, and the record's field is that function."""
    from sow_amd import acc_format
    fmt = acc_format.FORMATS[name]
    fn = {"fp8_e4m3": acc_format.short_fp8_pays, "mxfp4": acc_format.short_fp4_pays}[name]
    assert fmt.pays_short is fn and acc_format.AccFormat._fields[-1] == "pays_short"
    doc = fn.__doc__
    assert "profiles/short_codes.txt" in doc
    table = {(int(a), int(b)): int(n) for a, b, n in re.findall(r"^\s*(\d+)->(\d+): T <= (\d+)\s*$", doc, re.M)}
    assert len(table) == 8, "one line per measured shape"
    assert {k: v for k, v in table.items() if v} == acc_format.SHORT_CODES_TABLE[name]
    for (d_in, d_out), tmax in table.items():
        assert tmax in (0, 65, 128, 256, 512, 1024), "a measured row count"
        for T in (1, 64, 65, 128, 129, 256, 512, 1024, 1025):
            assert fn(T, d_in, d_out) == (64 < T <= tmax), (T, d_in, d_out)
    for d_in, d_out in ((264, 520), (288, 520), (1024, 1024), (4096, 768)):
        assert (d_in, d_out) not in table and not any(fn(T, d_in, d_out) for T in (65, 128, 1024))
    # the rule in the profile is the rule in the code
    prof = open(os.path.join(ROOT, "profiles", "short_codes.txt")).read()
    rule = {(int(a), int(b)): int(n) for a, b, n in re.findall(r"^#\s+" + name + r" (\d+)->(\d+): T <= (\d+)\s*$", prof, re.M)}
    assert rule == table
