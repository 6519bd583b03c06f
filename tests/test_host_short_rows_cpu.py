"""CPU tests of the short-batch entry points of dense-accumulator layers (sow_forward_short / sow_backward_short,
include/sow_amd.h): the C-ABI surface, the two workspace queries, every host-side refusal -- decided before anything is launched
or dereferenced (fake pointers, as tests/test_host_skinny_rows_cpu.py) -- and the Python switch with its dispatch rule."""
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
NAMES = ("sow_forward_short_workspace_bytes", "sow_short_workspace_bytes", "sow_forward_short", "sow_backward_short")
SHAPES = ((768, 768, 8), (768, 3072, 8), (3072, 768, 8), (4096, 4096, 50), (4096, 11008, 64), (11008, 4096, 2), (264, 520, 63), (512, 1376, 50))
TS = (1, 33, 64, 65, 100, 129, 1024)


def test_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "sow_amd.h")).read()
    assert re.search(r"^#define\s+SOW_SHORT_ROWS_MAX\s+1024\s*$", text, re.M)
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b(size_t|int)\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name), name
    for name in NAMES[:2]:
        assert _lib.SIGNATURES[name][0] is ctypes.c_size_t and len(_lib.SIGNATURES[name][1]) == 6
    for name in NAMES[2:]:
        assert _lib.SIGNATURES[name][1][0] is ctypes.POINTER(_lib.LayerArgs)
    assert _lib.load().sow_version() >= 123


def test_queries_are_positive_inside_the_admitted_set():
    lib = _lib.load()
    for T in TS:
        for d_in, d_out, r in SHAPES:
            for dt in (BF16, F16):
                fw = lib.sow_forward_short_workspace_bytes(T, d_in, d_out, r, DENSE, dt)
                full = lib.sow_short_workspace_bytes(T, d_in, d_out, r, DENSE, dt)
                base = lib.sow_workspace_bytes(T, d_in, d_out, r, 0, DENSE, dt)
                assert fw > 0 and full > 0, (T, d_in, d_out, r, dt)
                # one buffer serves the forward, the data phase and the unchanged weight phases
                assert full >= base and full >= fw, (T, d_in, d_out, r, dt, fw, full, base)
            # the slab plan is one for both compute dtypes (the plan of the weight phases is not: sow_workspace_bytes)
            assert (lib.sow_forward_short_workspace_bytes(T, d_in, d_out, r, DENSE, BF16)
                    == lib.sow_forward_short_workspace_bytes(T, d_in, d_out, r, DENSE, F16))
    # the partials hold at least one slab of fp32 y and of fp32 h
    assert lib.sow_forward_short_workspace_bytes(1024, 768, 768, 8, DENSE, BF16) >= 1024 * (768 + 64) * 4
    # more rows never need less
    q = lib.sow_short_workspace_bytes
    assert q(1024, 768, 768, 8, DENSE, BF16) >= q(512, 768, 768, 8, DENSE, BF16) >= q(65, 768, 768, 8, DENSE, BF16)


OUTSIDE = [(1025, 768, 768, 8, DENSE, BF16), (0, 768, 768, 8, DENSE, BF16), (-1, 768, 768, 8, DENSE, BF16),
           (100, 768, 768, 8, DENSE, F32), (100, 768, 768, 8, NONE, BF16), (100, 768, 768, 8, LOWRANK, BF16),
           (100, 768, 768, 8, FP8, BF16), (100, 768, 768, 8, FP4, F16), (100, 768, 768, 66, DENSE, BF16),
           (100, 768, 768, 0, DENSE, BF16), (100, 100, 768, 8, DENSE, BF16), (100, 768, 516, 8, DENSE, F16),
           (100, 768, 768, 8, DENSE, BF16 | PF), (100, 768, 768, 8, DENSE, F16 | PF | NATIVE), (100, 768, 768, 8, 5, BF16),
           (100, 768, 768, 8, DENSE, 7)]


def test_queries_are_zero_outside_the_admitted_set_and_pure():
    lib = _lib.load()
    inside = [(T, d_in, d_out, r, DENSE, dt) for T in TS for d_in, d_out, r in SHAPES[:3] for dt in (BF16, F16)]
    for q in (lib.sow_forward_short_workspace_bytes, lib.sow_short_workspace_bytes):
        for a in OUTSIDE:
            assert q(*a) == 0, a
        first = [q(*a) for a in inside + OUTSIDE]
        for sw in (dict(NO_SKINNY=1), dict(NO_SKINNY=0), {}):
            with _lib.switch(**sw):
                assert [q(*a) for a in inside + OUTSIDE] == first


def _fake_layers(n, T=100, d_in=512, d_out=768, r=50, kind=DENSE):
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
    ("none", dict(kind=NONE), BF16, ERR_UNSUPPORTED),
    ("lowrank", dict(kind=LOWRANK), F16, ERR_UNSUPPORTED),
    ("fp8", dict(kind=FP8), BF16, ERR_UNSUPPORTED),
    ("fp4", dict(kind=FP4), BF16, ERR_UNSUPPORTED),
    ("r=66", dict(r=66), BF16, ERR_UNSUPPORTED),
    ("d_in=100", dict(d_in=100), BF16, ERR_UNSUPPORTED),
    ("d_out=516", dict(d_out=516), F16, ERR_UNSUPPORTED),
    ("param_f32", {}, BF16 | PF, ERR_UNSUPPORTED),
    ("param_f32_native", {}, F16 | PF | NATIVE, ERR_UNSUPPORTED),
    ("fp32", {}, F32, ERR_DTYPE),
    ("fp32_param_f32", {}, F32 | PF, ERR_DTYPE),
    ("unknown_dtype", {}, 7, ERR_DTYPE),
]


@pytest.mark.parametrize("entry", ["sow_forward_short", "sow_backward_short"])
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


def test_workspace_alignment_layer_count_and_the_switch():
    lib = _lib.load()
    fwd, bwd = lib.sow_forward_short, lib.sow_backward_short
    need_f = lib.sow_forward_short_workspace_bytes(100, 512, 768, 50, DENSE, BF16)
    need = lib.sow_short_workspace_bytes(100, 512, 768, 50, DENSE, BF16)
    for fn, n in ((fwd, need_f), (bwd, need)):
        arr = _fake_layers(2)
        arr[1].workspace_bytes = n - 1
        assert fn(arr, 2, BF16, None) == ERR_WORKSPACE
        arr = _fake_layers(1)
        arr[0].workspace = None
        assert fn(arr, 1, F16, None) == ERR_WORKSPACE
    for field in ("x", "y", "acc_down", "A", "B", "bias", "h_save"):
        arr = _fake_layers(2)
        setattr(arr[1], field, getattr(arr[1], field) + 2)
        assert fwd(arr, 2, BF16, None) == ERR_UNSUPPORTED, field
    for field in ("dy", "dx", "acc_down", "A", "B"):
        arr = _fake_layers(2)
        setattr(arr[1], field, getattr(arr[1], field) + 2)
        assert bwd(arr, 2, BF16, None) == ERR_UNSUPPORTED, field
    for fn, fields in ((fwd, ("x", "y", "A", "B", "acc_down")), (bwd, ("dy", "dx", "A", "B", "acc_down"))):
        assert fn(_fake_layers(17), 17, BF16, None) == ERR_UNSUPPORTED     # n > 16
        for field in fields:
            arr = _fake_layers(1)
            setattr(arr[0], field, None)
            assert fn(arr, 1, BF16, None) == ERR_NULL, field
        assert fn(None, 1, BF16, None) == ERR_NULL
        assert fn(_fake_layers(1), -1, BF16, None) == ERR_SHAPE
        # nothing to do: SOW_OK without a launch
        assert fn(_fake_layers(3, T=0), 3, BF16, None) == 0
        assert fn(_fake_layers(1), 0, F16, None) == 0
        with _lib.switch(NO_SKINNY=1):
            assert fn(_fake_layers(1), 1, BF16, None) == ERR_UNSUPPORTED
            assert fn(_fake_layers(3, T=0), 3, BF16, None) == ERR_UNSUPPORTED
            assert fn(_fake_layers(1), 1, F32, None) == ERR_DTYPE
    assert lib.sow_get_switch(b"NO_SKINNY") in (-1, 0)


def test_short_rows_switch_restores_the_earlier_value():
    import sow_amd
    from sow_amd import ops
    assert ops.short_rows_enabled() is False, "the default is off"
    with sow_amd.short_rows():
        assert ops.short_rows_enabled() is True
        with sow_amd.short_rows(False):
            assert ops.short_rows_enabled() is False
        assert ops.short_rows_enabled() is True
    assert ops.short_rows_enabled() is False
    assert sow_amd.set_short_rows(True) is False
    try:
        with pytest.raises(RuntimeError):
            with sow_amd.short_rows(False):
                raise RuntimeError("leave the block")
        assert ops.short_rows_enabled() is True
    finally:
        assert sow_amd.set_short_rows(False) is True
    with pytest.raises(ValueError):
        sow_amd.set_short_rows(1)


def test_short_rows_pays_equals_the_table_in_its_docstring():
    """The docstring carries one line per measured shape class: `d_in->d_out: T <= N` (N = 0: never).  The rule is exactly that
    table: true inside it, false at every other shape and row count."""
    from sow_amd import ops
    doc = ops.short_rows_pays.__doc__
    table = {(int(a), int(b)): int(n) for a, b, n in re.findall(r"^\s*(\d+)->(\d+): T <= (\d+)\s*$", doc, re.M)}
    assert table, "the docstring holds the table"
    assert table == ops.SHORT_ROWS_TABLE
    for (d_in, d_out), tmax in table.items():
        for T in (1, 64, 65, 128, 256, 512, 1024, 1025):
            assert ops.short_rows_pays(T, d_in, d_out) == (64 < T <= tmax), (T, d_in, d_out)
    for d_in, d_out in ((264, 520), (1024, 1024), (4096, 768)):
        if (d_in, d_out) not in table:
            assert not any(ops.short_rows_pays(T, d_in, d_out) for T in (65, 128, 1024))
