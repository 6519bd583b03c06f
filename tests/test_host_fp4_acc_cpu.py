"""CPU tests of the C-ABI surface of MXFP4 dense accumulators (include/sow_amd.h: SOW_ACC_DENSE_FP4): the workspace query, and
the refusals, every one of which is decided on the host before anything is launched or dereferenced (the pointers below are
fakes: a launch, or a read of one of them, would not return a code)."""
import ctypes
import os
import re

import pytest

from sow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F16, F32 = _lib.BF16, _lib.F16, _lib.F32
FP4 = getattr(_lib, "ACC_DENSE_FP4", None)
FP8, DENSE, LOWRANK, NONE = _lib.ACC_DENSE_FP8, _lib.ACC_DENSE, _lib.ACC_LOWRANK, _lib.ACC_NONE
ERR_NULL, ERR_SHAPE, ERR_DTYPE, ERR_ALIGN, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -3, -4, -5, -6


def test_kind_and_entry_points_are_declared():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sow_amd.h")).read(), flags=re.S)
    assert re.search(r"#define\s+SOW_ACC_DENSE_FP4\s+4\b", header) and FP4 == 4
    assert re.search(r"\bint\s+sow_acc_dequantize_fp4\s*\(", header)
    assert re.search(r"\bsize_t\s+sow_forward_skinny_fp4_workspace_bytes\s*\(", header)
    assert "sow_acc_dequantize_fp4" in _lib.SIGNATURES and "sow_forward_skinny_fp4_workspace_bytes" in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, "sow_acc_dequantize_fp4") and hasattr(lib, "sow_forward_skinny_fp4_workspace_bytes")


def test_workspace_query():
    lib = _lib.load()
    q, qd, q8 = (lib.sow_forward_skinny_fp4_workspace_bytes, lib.sow_forward_skinny_workspace_bytes,
                 lib.sow_forward_skinny_fp8_workspace_bytes)
    for a in [(1, 4096, 4096, 8, BF16), (32, 4096, 11008, 50, BF16), (4, 11008, 4096, 64, F16), (16, 32, 8, 64, BF16)]:
        assert q(*a) > 0, a
    for a in [(33, 4096, 4096, 8, BF16), (0, 4096, 4096, 8, BF16), (4, 4096, 4096, 66, BF16), (4, 4096, 523, 8, BF16),
              (4, 4096, 524, 8, BF16), (4, 520, 4096, 8, F16), (4, 4104, 4096, 8, BF16), (4, 4096, 4096, 8, F32),
              (4, 4096, 4096, 8, BF16 | _lib.PARAM_F32)]:
        assert q(*a) == 0, a
    # the slab plan of the E4M3 kind: 128-column ranges, 4096 x 4096 plans 16 slabs; the partials of y and of x . A per slab
    assert q(4, 4096, 4096, 8, BF16) == 256 + 16 * 4 * (4096 + 64) * 4 == q8(4, 4096, 4096, 8, BF16)
    assert q(4, 4096, 4096, 8, BF16) == q(4, 4096, 4096, 50, F16)
    # the older queries keep their answer for the value 4
    assert qd(4, 4096, 4096, 8, FP4, BF16) == 0
    assert lib.sow_workspace_bytes(4, 512, 512, 50, 0, FP4, BF16) == 0
    assert lib.sow_forward_workspace_bytes(4, 512, 512, 50, 0, FP4, BF16) == 0
    # a pure function of the shape: the switches do not enter
    with _lib.switch(NO_SKINNY=1):
        assert q(4, 4096, 4096, 8, BF16) == 256 + 16 * 4 * (4096 + 64) * 4


def _fake_layers(n, T=4, d_in=512, d_out=512, r=50, kind=FP4):
    arr = (_lib.LayerArgs * n)()
    for i in range(n):
        a = arr[i]
        base = 0x10000000 * (i + 1)
        a.x, a.A, a.B, a.acc_down, a.acc_up, a.bias, a.y = (0x1000000, base + 0x1000, base + 0x2000, base + 0x3000, base + 0x3800,
                                                           base + 0x4000, base + 0x5000)
        a.h_save, a.dy, a.dx, a.dA, a.dB = base + 0x6000, base + 0x7000, 0x2000000, base + 0x9000, base + 0xa000
        a.workspace, a.workspace_bytes = base + 0x100000, 1 << 30
        a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, kind, 0.5
    return arr


def test_other_entry_points_refuse_the_kind_on_the_host():
    lib = _lib.load()
    both = _lib.BWD_DATA | _lib.BWD_WEIGHTS
    out = (ctypes.c_int * 8)()
    for n, bad in ((1, 0), (3, 0), (3, 1), (3, 2)):       # one bad layer refuses the whole call, wherever it sits
        arr = _fake_layers(n, kind=DENSE)
        arr[bad].acc_kind = FP4
        assert lib.sow_forward_group(arr, n, BF16, None) == ERR_UNSUPPORTED
        assert lib.sow_backward_group(arr, n, BF16, both, None) == ERR_UNSUPPORTED
        assert lib.sow_forward_shared(arr, n, BF16, None) == ERR_UNSUPPORTED
        assert lib.sow_backward_shared(arr, n, BF16, both, None) == ERR_UNSUPPORTED
        assert lib.sow_backward_group_plan(arr, n, BF16, both, out) == ERR_UNSUPPORTED
        assert lib.sow_backward_group_reduce_desc(arr, n, BF16, both, 0x5000000, out) == ERR_UNSUPPORTED
    a = _fake_layers(1)[0]
    assert lib.sow_forward(a.x, a.A, a.B, a.acc_down, a.acc_up, None, a.y, a.h_save, 4, 512, 512, 50, 0, FP4, 0.5, BF16, a.workspace,
                           a.workspace_bytes, None) == ERR_UNSUPPORTED
    assert lib.sow_backward_ex(a.dy, a.x, a.h_save, a.A, a.B, a.acc_down, a.acc_up, a.dx, a.dA, a.dB, None, 4, 512, 512, 50, 0, FP4, 0.5,
                               0.0, BF16, a.workspace, a.workspace_bytes, both, None) == ERR_UNSUPPORTED
    assert lib.sow_backward_reduce_desc(a.dA, a.dB, None, 64, 512, 512, 50, 0, FP4, 0.0, BF16, a.workspace, a.workspace_bytes,
                                        0x5000000, 0x6000000) == ERR_UNSUPPORTED
    # before every other check: a dtype that those entry points refuse otherwise
    assert lib.sow_forward_group(_fake_layers(1), 1, 7, None) == ERR_UNSUPPORTED
    assert lib.sow_forward(a.x, a.A, a.B, a.acc_down, a.acc_up, None, a.y, a.h_save, 4, 512, 512, 50, 0, FP4, 0.5, 7, a.workspace,
                           a.workspace_bytes, None) == ERR_UNSUPPORTED


SKINNY = [("T=33", dict(T=33), BF16, ERR_UNSUPPORTED), ("r=66", dict(r=66), BF16, ERR_UNSUPPORTED),
          ("d_in=520", dict(d_in=520), BF16, ERR_UNSUPPORTED), ("d_out=524", dict(d_out=524), BF16, ERR_UNSUPPORTED),
          ("param_f32", {}, BF16 | _lib.PARAM_F32, ERR_UNSUPPORTED), ("fp32", {}, F32, ERR_DTYPE)]


@pytest.mark.parametrize("name,kw,dtype,code", SKINNY, ids=[r[0] for r in SKINNY])
def test_skinny_refusals_are_decided_on_the_host(name, kw, dtype, code):
    lib = _lib.load()
    assert FP4 == 4
    assert lib.sow_forward_skinny(_fake_layers(1, **kw), 1, dtype, None) == code
    arr = _fake_layers(3)
    bad = _fake_layers(1, **kw)[0]
    for f in ("T", "d_in", "d_out", "r_live"):
        setattr(arr[2], f, getattr(bad, f))
    assert lib.sow_forward_skinny(arr, 3, dtype, None) == code


def test_d_in_520_is_admitted_by_the_other_dense_kinds():
    """520 is a multiple of 8: only the MXFP4 kind (whole blocks of 32) refuses it -- the refusal above is the kind's own."""
    lib = _lib.load()
    assert lib.sow_forward_skinny_workspace_bytes(4, 520, 512, 50, DENSE, BF16) > 0
    assert lib.sow_forward_skinny_fp8_workspace_bytes(4, 520, 512, 50, BF16) > 0
    assert lib.sow_forward_skinny_fp4_workspace_bytes(4, 520, 512, 50, BF16) == 0
    assert lib.sow_forward_skinny_fp4_workspace_bytes(4, 544, 512, 50, BF16) > 0


def test_skinny_operands_of_the_kind():
    lib = _lib.load()
    arr = _fake_layers(2)
    arr[1].acc_up = None                                    # the block scales are an operand
    assert lib.sow_forward_skinny(arr, 2, BF16, None) == ERR_NULL
    for field in ("acc_down", "acc_up"):                    # 8-byte-aligned codes and scales
        arr = _fake_layers(2)
        setattr(arr[1], field, getattr(arr[1], field) + 4)
        assert lib.sow_forward_skinny(arr, 2, BF16, None) == ERR_UNSUPPORTED
    for other in (FP8, DENSE):                              # one kind of dense accumulator per call
        for pos in (0, 1):
            arr = _fake_layers(2)
            arr[pos].acc_kind = other
            assert lib.sow_forward_skinny(arr, 2, BF16, None) == ERR_UNSUPPORTED
    arr = _fake_layers(2)
    arr[0].acc_kind = LOWRANK                               # 1 + 4
    assert lib.sow_forward_skinny(arr, 2, BF16, None) == ERR_UNSUPPORTED
    arr = _fake_layers(1)
    arr[0].workspace_bytes = lib.sow_forward_skinny_fp4_workspace_bytes(4, 512, 512, 50, BF16) - 1
    assert lib.sow_forward_skinny(arr, 1, BF16, None) == ERR_WORKSPACE
    arr = _fake_layers(1, d_in=4096, d_out=4096)
    arr[0].workspace_bytes = lib.sow_forward_skinny_workspace_bytes(4, 4096, 4096, 50, DENSE, BF16)  # the bf16 plan: half the slabs
    assert lib.sow_forward_skinny(arr, 1, BF16, None) == ERR_WORKSPACE
    assert lib.sow_forward_skinny(_fake_layers(3, T=0), 3, F16, None) == 0
    with _lib.switch(NO_SKINNY=1):
        assert lib.sow_forward_skinny(_fake_layers(1), 1, BF16, None) == ERR_UNSUPPORTED


def test_dequantize_argument_checks():
    f = _lib.load().sow_acc_dequantize_fp4
    q, e, dst = 0x1000000, 0x2000000, 0x3000000
    assert f(q, e, 0, 64, dst, 64, BF16, None) == 0 and f(q, e, 64, 0, dst, 0, F16, None) == 0      # nothing to do
    assert f(q, e, 64, 64, dst, 56, BF16, None) == ERR_SHAPE and f(q, e, -1, 64, dst, 64, BF16, None) == ERR_SHAPE
    assert f(q, e, 64, 64, dst, 64, F32, None) == ERR_DTYPE
    assert f(None, e, 64, 64, dst, 64, BF16, None) == ERR_NULL and f(q, None, 64, 64, dst, 64, BF16, None) == ERR_NULL
    assert f(q, e, 64, 60, dst, 64, BF16, None) == ERR_UNSUPPORTED and f(q, e, 64, 56, dst, 60, BF16, None) == ERR_UNSUPPORTED
    assert f(q, e, 72, 64, dst, 64, BF16, None) == ERR_UNSUPPORTED                                 # whole blocks of 32 rows
    assert f(q + 4, e, 64, 64, dst, 64, BF16, None) == ERR_ALIGN and f(q, e + 4, 64, 64, dst, 64, BF16, None) == ERR_ALIGN
    assert f(q, e, 64, 64, dst + 8, 64, BF16, None) == ERR_ALIGN
