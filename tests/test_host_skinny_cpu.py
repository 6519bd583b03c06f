"""CPU tests of the generation-sized forward (sow_forward_skinny, include/sow_amd.h): the C-ABI surface, the workspace
query and the host-side refusals, every one of which is decided before anything is launched or dereferenced."""
import ctypes
import os
import re

import pytest

from sow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = _lib.F32, _lib.BF16, _lib.F16
NONE, LOWRANK, DENSE = _lib.ACC_NONE, _lib.ACC_LOWRANK, _lib.ACC_DENSE
ERR_SHAPE, ERR_DTYPE, ERR_WORKSPACE, ERR_UNSUPPORTED = -2, -3, -5, -6


def test_skinny_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sow_amd.h")).read(), flags=re.S)
    assert re.search(r"\bsize_t\s+sow_forward_skinny_workspace_bytes\s*\(", header)
    assert re.search(r"\bint\s+sow_forward_skinny\s*\(", header)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sow_forward_skinny_workspace_bytes", "sow_forward_skinny"):
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name), name
    assert _lib.SIGNATURES["sow_forward_skinny"][1][0] is ctypes.POINTER(_lib.LayerArgs)
    assert _lib.SIGNATURES["sow_forward_skinny_workspace_bytes"][0] is ctypes.c_size_t
    assert len(_lib.SIGNATURES["sow_forward_skinny_workspace_bytes"][1]) == 6
    assert _lib.load().sow_get_switch(b"NO_SKINNY") in (-1, 0, 1)   # a known switch name (unknown: SOW_ERR_UNSUPPORTED)
    assert _lib.load().sow_version() >= 118


INSIDE = [(1, 4096, 4096, 8, DENSE, BF16), (32, 4096, 11008, 50, DENSE, BF16), (4, 11008, 4096, 64, DENSE, F16),
          (3, 264, 520, 2, NONE, BF16), (17, 1032, 72, 1, NONE, F16), (16, 8, 8, 64, DENSE, BF16)]
OUTSIDE = [(33, 4096, 4096, 8, DENSE, BF16), (0, 4096, 4096, 8, DENSE, BF16), (-1, 512, 512, 8, DENSE, BF16),
           (4, 4096, 4096, 8, LOWRANK, BF16), (4, 4096, 4096, 66, DENSE, BF16), (4, 4096, 4096, 0, DENSE, BF16),
           (4, 4096, 523, 8, DENSE, BF16), (4, 516, 4096, 8, NONE, F16), (4, 4096, 4096, 8, DENSE, F32),
           (4, 4096, 4096, 8, DENSE, BF16 | _lib.PARAM_F32), (4, 4096, 4096, 8, DENSE, F16 | _lib.PARAM_F32),
           (4, 4096, 4096, 8, 3, BF16), (4, 4096, 4096, 8, DENSE, 7), (4, 0, 4096, 8, DENSE, BF16)]


def test_workspace_query_is_zero_outside_the_admitted_set_and_positive_inside():
    q = _lib.load().sow_forward_skinny_workspace_bytes
    for a in INSIDE:
        assert q(*a) > 0, a
    for a in OUTSIDE:
        assert q(*a) == 0, a
    # a dense accumulator needs the slab partials of y on top of those of x . A; more tokens never need less
    assert q(4, 4096, 4096, 8, DENSE, BF16) > q(4, 4096, 4096, 8, NONE, BF16)
    assert q(32, 4096, 4096, 8, DENSE, BF16) > q(4, 4096, 4096, 8, DENSE, BF16)
    # bf16 and f16 share the plan (fp32 partials either way); the rank does not enter (the partials of x . A hold 64 columns)
    assert q(4, 4096, 4096, 8, DENSE, BF16) == q(4, 4096, 4096, 8, DENSE, F16) == q(4, 4096, 4096, 50, DENSE, BF16)
    # far below the weight it streams: the K-slab count is planned, not one slab per k-step
    assert q(32, 4096, 4096, 50, DENSE, BF16) < 4096 * 4096 * 2 // 4


def test_workspace_query_is_a_pure_function_of_the_shape():
    q = _lib.load().sow_forward_skinny_workspace_bytes
    first = [q(*a) for a in INSIDE + OUTSIDE]
    assert [q(*a) for a in INSIDE + OUTSIDE] == first
    with _lib.switch(NO_SKINNY=1):
        assert [q(*a) for a in INSIDE + OUTSIDE] == first
    with _lib.switch(NO_SKINNY=0):
        assert [q(*a) for a in INSIDE + OUTSIDE] == first


def _fake_layers(n, T=4, d_in=512, d_out=512, r=50, kind=DENSE):
    """Layer descriptors with dummy non-null, 16-byte-aligned pointers that are never dereferenced: every call below must
    return from the host checks (a launch on this machine, or a read of one of these addresses, would not return a code)."""
    arr = (_lib.LayerArgs * n)()
    for i in range(n):
        a = arr[i]
        base = 0x10000000 * (i + 1)
        a.x, a.A, a.B, a.acc_down, a.bias, a.y = 0x1000000, base + 0x1000, base + 0x2000, base + 0x3000, base + 0x4000, base + 0x5000
        a.workspace, a.workspace_bytes = base + 0x100000, 1 << 30
        a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, kind, 0.5
    return arr


REFUSALS = [
    ("T=33", dict(T=33), BF16, ERR_UNSUPPORTED),
    ("lowrank", dict(kind=LOWRANK), BF16, ERR_UNSUPPORTED),
    ("r=65", dict(r=65), BF16, ERR_UNSUPPORTED),
    ("r=66", dict(r=66), BF16, ERR_UNSUPPORTED),
    ("d_out=523", dict(d_out=523), BF16, ERR_UNSUPPORTED),
    ("d_in=516", dict(d_in=516), F16, ERR_UNSUPPORTED),
    ("param_f32_bf16", {}, BF16 | _lib.PARAM_F32, ERR_UNSUPPORTED),
    ("param_f32_f16", {}, F16 | _lib.PARAM_F32, ERR_UNSUPPORTED),
    ("fp32", {}, F32, ERR_DTYPE),
    ("fp32_param_f32", {}, F32 | _lib.PARAM_F32, ERR_DTYPE),
    ("unknown_dtype", {}, 7, ERR_DTYPE),
]


@pytest.mark.parametrize("name,kw,dtype,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_are_decided_on_the_host(name, kw, dtype, code):
    lib = _lib.load()
    assert lib.sow_forward_skinny(_fake_layers(1, **kw), 1, dtype, None) == code
    # one bad layer refuses the whole call, wherever it sits: nothing is launched for the layers ahead of it
    arr = _fake_layers(3)
    bad = _fake_layers(1, **kw)[0]
    for f in ("T", "d_in", "d_out", "r_live", "acc_kind"):
        setattr(arr[2], f, getattr(bad, f))
    assert lib.sow_forward_skinny(arr, 3, dtype, None) == code


def test_misaligned_bases_workspace_and_layer_count():
    lib = _lib.load()
    for field in ("x", "y", "acc_down", "A", "B", "bias"):
        arr = _fake_layers(2)
        setattr(arr[1], field, getattr(arr[1], field) + 2)
        assert lib.sow_forward_skinny(arr, 2, BF16, None) == ERR_UNSUPPORTED, field
    need = lib.sow_forward_skinny_workspace_bytes(4, 512, 512, 50, DENSE, BF16)
    arr = _fake_layers(2)
    arr[1].workspace_bytes = need - 1
    assert lib.sow_forward_skinny(arr, 2, BF16, None) == ERR_WORKSPACE
    arr = _fake_layers(1)
    arr[0].workspace = None
    assert lib.sow_forward_skinny(arr, 1, F16, None) == ERR_WORKSPACE
    assert lib.sow_forward_skinny(_fake_layers(17), 17, BF16, None) == ERR_UNSUPPORTED          # n > 16
    arr = _fake_layers(1)
    arr[0].A = None
    assert lib.sow_forward_skinny(arr, 1, BF16, None) == -1                                     # SOW_ERR_NULL
    assert lib.sow_forward_skinny(None, 1, BF16, None) == -1
    assert lib.sow_forward_skinny(_fake_layers(1), -1, BF16, None) == ERR_SHAPE
    assert lib.sow_forward_skinny(_fake_layers(1, d_in=0), 1, BF16, None) == ERR_SHAPE


def test_empty_calls_and_the_switch():
    lib = _lib.load()
    assert lib.sow_forward_skinny(_fake_layers(3, T=0), 3, BF16, None) == 0       # T = 0: nothing to do, SOW_OK
    assert lib.sow_forward_skinny(_fake_layers(1), 0, F16, None) == 0
    with _lib.switch(NO_SKINNY=1):
        assert lib.sow_forward_skinny(_fake_layers(1), 1, BF16, None) == ERR_UNSUPPORTED
        assert lib.sow_forward_skinny(_fake_layers(3, T=0), 3, BF16, None) == ERR_UNSUPPORTED
        assert lib.sow_forward_skinny(_fake_layers(1), 1, F32, None) == ERR_DTYPE
    assert lib.sow_get_switch(b"NO_SKINNY") in (-1, 0)
