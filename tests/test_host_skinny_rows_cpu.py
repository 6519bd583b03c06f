"""CPU tests of the generation-sized forward for up to 64 rows (sow_forward_skinny_rows, include/sow_amd.h): the C-ABI surface,
the one workspace query of all four accumulator kinds and the host-side refusals, every one of which is decided before anything
is launched or dereferenced (fake pointers, as tests/test_host_skinny_cpu.py)."""
import ctypes
import os
import re

import pytest

from sow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = _lib.F32, _lib.BF16, _lib.F16
PF, NATIVE = _lib.PARAM_F32, _lib.ACC_NATIVE
NONE, LOWRANK, DENSE, FP8, FP4 = _lib.ACC_NONE, _lib.ACC_LOWRANK, _lib.ACC_DENSE, _lib.ACC_DENSE_FP8, _lib.ACC_DENSE_FP4
KINDS = (NONE, DENSE, FP8, FP4)
ERR_NULL, ERR_SHAPE, ERR_DTYPE, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -3, -5, -6


def _old_query(T, d_in, d_out, r, kind, dtype):
    """The query of sow_forward_skinny that matches `kind`."""
    lib = _lib.load()
    if kind == FP8:
        return lib.sow_forward_skinny_fp8_workspace_bytes(T, d_in, d_out, r, dtype)
    if kind == FP4:
        return lib.sow_forward_skinny_fp4_workspace_bytes(T, d_in, d_out, r, dtype)
    return lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, kind, dtype)


def test_rows_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "sow_amd.h")).read()
    assert re.search(r"^#define\s+SOW_SKINNY_ROWS_MAX\s+64\s*$", text, re.M)
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bsize_t\s+sow_forward_skinny_rows_workspace_bytes\s*\(", header)
    assert re.search(r"\bint\s+sow_forward_skinny_rows\s*\(", header)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sow_forward_skinny_rows_workspace_bytes", "sow_forward_skinny_rows"):
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name), name
    assert _lib.SIGNATURES["sow_forward_skinny_rows"][1][0] is ctypes.POINTER(_lib.LayerArgs)
    assert _lib.SIGNATURES["sow_forward_skinny_rows_workspace_bytes"][0] is ctypes.c_size_t
    assert len(_lib.SIGNATURES["sow_forward_skinny_rows_workspace_bytes"][1]) == 6
    assert _lib.load().sow_version() >= 122


@pytest.mark.parametrize("kind", KINDS)
def test_query_is_positive_past_32_rows_for_every_kind_and_dtype(kind):
    q = _lib.load().sow_forward_skinny_rows_workspace_bytes
    for T in (33, 48, 64):
        for dtype in (BF16, F16, BF16 | PF | NATIVE, F16 | PF | NATIVE):
            for d_in, d_out, r in ((4096, 4096, 8), (288, 520, 50), (11008, 4096, 64)):
                assert q(T, d_in, d_out, r, kind, dtype) > 0, (T, d_in, d_out, r, kind, dtype)
        # fp32 factors need no workspace of their own, and the compute dtypes share the plan
        assert q(T, 4096, 4096, 8, kind, BF16) == q(T, 4096, 4096, 8, kind, F16) == q(T, 4096, 4096, 8, kind, BF16 | PF | NATIVE)
    # more rows never need less; an accumulator needs the partials of y on top of those of x . A
    assert q(64, 4096, 4096, 8, kind, BF16) >= q(48, 4096, 4096, 8, kind, BF16) >= q(33, 4096, 4096, 8, kind, BF16)
    if kind != NONE:
        assert q(64, 4096, 4096, 8, kind, BF16) > q(64, 4096, 4096, 8, NONE, BF16)


OUTSIDE = [(65, 4096, 4096, 8, DENSE, BF16), (0, 4096, 4096, 8, DENSE, BF16), (-1, 512, 512, 8, DENSE, BF16),
           (64, 4096, 4096, 8, DENSE, F32), (64, 4096, 4096, 8, LOWRANK, BF16), (64, 4096, 4096, 65, DENSE, BF16),
           (64, 4096, 516, 8, DENSE, BF16), (64, 264, 4096, 8, FP4, BF16), (48, 4096, 4096, 8, FP8, BF16 | PF),
           (48, 4096, 4096, 8, NONE, F16 | PF), (64, 4096, 4096, 8, 5, BF16), (64, 4096, 4096, 0, DENSE, BF16),
           (65, 4096, 4096, 8, FP8, F16), (65, 4096, 4096, 8, FP4, F16), (65, 4096, 4096, 8, NONE, F16)]


def test_query_is_zero_outside_the_admitted_set_and_pure():
    q = _lib.load().sow_forward_skinny_rows_workspace_bytes
    for a in OUTSIDE:
        assert q(*a) == 0, a
    inside = [(T, 520, 264, 50, kind, dt) for T in (1, 33, 64) for kind in KINDS for dt in (BF16, F16) if kind != FP4] + \
             [(T, 544, 264, 50, FP4, BF16) for T in (1, 33, 64)]
    first = [q(*a) for a in inside + OUTSIDE]
    assert all(v > 0 for v in first[:len(inside)])
    for sw in (dict(NO_SKINNY=1), dict(NO_SKINNY=0), {}):
        with _lib.switch(**sw):
            assert [q(*a) for a in inside + OUTSIDE] == first


@pytest.mark.parametrize("T", [1, 17, 32])
def test_up_to_32_rows_the_query_is_the_existing_one(T):
    q = _lib.load().sow_forward_skinny_rows_workspace_bytes
    for kind in KINDS:
        for dtype in (BF16, F16, BF16 | PF | NATIVE):
            for d_in, d_out, r in ((4096, 4096, 8), (4096, 11008, 50), (11008, 4096, 64), (288, 520, 2), (8224, 128, 8)):
                want = _old_query(T, d_in, d_out, r, kind, dtype)
                assert want > 0
                assert q(T, d_in, d_out, r, kind, dtype) == want, (T, d_in, d_out, r, kind, dtype)


def _fake_layers(n, T=64, d_in=512, d_out=512, r=50, kind=DENSE):
    """Layer descriptors with dummy non-null, 16-byte-aligned pointers that are never dereferenced: every call below must
    return from the host checks (a launch on this machine, or a read of one of these addresses, would not return a code)."""
    arr = (_lib.LayerArgs * n)()
    for i in range(n):
        a = arr[i]
        base = 0x10000000 * (i + 1)
        a.x, a.A, a.B, a.acc_down, a.bias, a.y = 0x1000000, base + 0x1000, base + 0x2000, base + 0x3000, base + 0x4000, base + 0x5000
        a.acc_up = base + 0x6000
        a.workspace, a.workspace_bytes = base + 0x100000, 1 << 30
        a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, kind, 0.5
    return arr


REFUSALS = [
    ("T=65", dict(T=65), BF16, ERR_UNSUPPORTED),
    ("T=-1", dict(T=-1), BF16, ERR_SHAPE),
    ("lowrank", dict(kind=LOWRANK), BF16, ERR_UNSUPPORTED),
    ("r=65", dict(r=65), BF16, ERR_UNSUPPORTED),
    ("d_out=516", dict(d_out=516), BF16, ERR_UNSUPPORTED),
    ("d_in=516", dict(d_in=516), F16, ERR_UNSUPPORTED),
    ("fp4_d_in=264", dict(d_in=264, kind=FP4), BF16, ERR_UNSUPPORTED),
    ("param_f32_bf16", {}, BF16 | PF, ERR_UNSUPPORTED),
    ("param_f32_f16", dict(kind=FP8), F16 | PF, ERR_UNSUPPORTED),
    ("fp32", {}, F32, ERR_DTYPE),
    ("fp32_param_f32", {}, F32 | PF, ERR_DTYPE),
    ("unknown_dtype", {}, 7, ERR_DTYPE),
]


@pytest.mark.parametrize("name,kw,dtype,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_are_decided_on_the_host(name, kw, dtype, code):
    lib = _lib.load()
    assert lib.sow_forward_skinny_rows(_fake_layers(1, **kw), 1, dtype, None) == code
    # one bad layer refuses the whole call, wherever it sits: nothing is launched for the layers ahead of it
    arr = _fake_layers(3, kind=kw.get("kind", DENSE) if kw.get("kind") in (FP8, FP4) else DENSE)
    bad = _fake_layers(1, **kw)[0]
    for f in ("T", "d_in", "d_out", "r_live", "acc_kind"):
        setattr(arr[2], f, getattr(bad, f))
    assert lib.sow_forward_skinny_rows(arr, 3, dtype, None) == code
    # ... also behind a layer of at most 32 rows
    arr[0].T = 17
    assert lib.sow_forward_skinny_rows(arr, 3, dtype, None) == code


@pytest.mark.parametrize("kinds", [(DENSE, FP8), (FP8, FP4), (FP4, DENSE)])
def test_dense_kinds_do_not_mix(kinds):
    lib = _lib.load()
    arr = _fake_layers(3, d_in=544)
    arr[0].acc_kind, arr[1].acc_kind, arr[2].acc_kind = kinds[0], NONE, kinds[1]
    arr[2].T = 17
    assert lib.sow_forward_skinny_rows(arr, 3, BF16, None) == ERR_UNSUPPORTED
    assert lib.sow_forward_skinny_rows(arr, 3, F16 | PF | NATIVE, None) == ERR_UNSUPPORTED


def test_workspace_alignment_layer_count_and_the_switch():
    lib = _lib.load()
    for kind in KINDS:
        need = lib.sow_forward_skinny_rows_workspace_bytes(64, 544, 512, 50, kind, BF16)
        arr = _fake_layers(2, d_in=544, kind=kind)
        arr[1].workspace_bytes = need - 1
        assert lib.sow_forward_skinny_rows(arr, 2, BF16, None) == ERR_WORKSPACE, kind
    arr = _fake_layers(1)
    arr[0].workspace = None
    assert lib.sow_forward_skinny_rows(arr, 1, F16, None) == ERR_WORKSPACE
    for field in ("x", "y", "acc_down", "A", "B", "bias"):
        arr = _fake_layers(2)
        setattr(arr[1], field, getattr(arr[1], field) + 2)
        assert lib.sow_forward_skinny_rows(arr, 2, BF16, None) == ERR_UNSUPPORTED, field
    assert lib.sow_forward_skinny_rows(_fake_layers(17), 17, BF16, None) == ERR_UNSUPPORTED     # n > 16
    arr = _fake_layers(1)
    arr[0].A = None
    assert lib.sow_forward_skinny_rows(arr, 1, BF16, None) == ERR_NULL
    arr = _fake_layers(1, kind=FP8)
    arr[0].acc_up = None
    assert lib.sow_forward_skinny_rows(arr, 1, BF16, None) == ERR_NULL
    assert lib.sow_forward_skinny_rows(None, 1, BF16, None) == ERR_NULL
    assert lib.sow_forward_skinny_rows(_fake_layers(1), -1, BF16, None) == ERR_SHAPE
    # nothing to do: SOW_OK without a launch
    assert lib.sow_forward_skinny_rows(_fake_layers(3, T=0), 3, BF16, None) == 0
    assert lib.sow_forward_skinny_rows(_fake_layers(1), 0, F16, None) == 0
    with _lib.switch(NO_SKINNY=1):
        assert lib.sow_forward_skinny_rows(_fake_layers(1), 1, BF16, None) == ERR_UNSUPPORTED
        assert lib.sow_forward_skinny_rows(_fake_layers(1, T=4), 1, BF16, None) == ERR_UNSUPPORTED
        assert lib.sow_forward_skinny_rows(_fake_layers(3, T=0), 3, BF16, None) == ERR_UNSUPPORTED
        assert lib.sow_forward_skinny_rows(_fake_layers(1), 1, F32, None) == ERR_DTYPE
    assert lib.sow_get_switch(b"NO_SKINNY") in (-1, 0)
    # the existing entry keeps refusing 33 rows
    assert lib.sow_forward_skinny(_fake_layers(1, T=33), 1, BF16, None) == ERR_UNSUPPORTED
    assert lib.sow_forward_skinny_workspace_bytes(33, 512, 512, 50, DENSE, BF16) == 0
