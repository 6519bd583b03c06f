"""CPU tests of the SOW_ACC_NATIVE surface of the C ABI (include/sow_amd.h: fp32 master factors over an accumulator that is
already of the compute dtype; no GPU compute, fake pointers): the bit's value, the workspace queries without the accumulator's
packs, the dtype refusals, and the skinny forward that admits fp32 factors only next to the bit."""
import ctypes
import os
import re

import pytest

from sow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(0x10000)     # never dereferenced: every call below returns before a launch
PF, NATIVE = _lib.PARAM_F32, _lib.ACC_NATIVE
ERR_DTYPE, ERR_WORKSPACE, ERR_UNSUPPORTED = -3, -5, -6
DTS = [_lib.BF16, _lib.F16]


def al256(n: int) -> int:
    return (n + 255) // 256 * 256


def test_version_and_bit():
    """Declared in the header with the value the binding uses, disjoint from the dtype codes and from every other flag."""
    assert _lib.load().sow_version() >= 121
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sow_amd.h")).read(), flags=re.S)
    m = re.search(r"#define\s+SOW_ACC_NATIVE\s+(0x[0-9a-fA-F]+)", header)
    assert m and int(m.group(1), 16) == NATIVE == 0x800
    others = [_lib.F32, _lib.BF16, _lib.F16, _lib.PARAM_F32, _lib.FUSE_ACC, _lib.FUSE_ACC_DEEP]
    assert all(NATIVE & v == 0 for v in others)
    assert bin(NATIVE).count("1") == 1


SHAPES = [  # (T, d_in, d_out, r, r_acc, kind)
    (64, 512, 512, 50, 0, _lib.ACC_DENSE),
    (8193, 512, 1376, 8, 0, _lib.ACC_DENSE),
    (256, 768, 768, 100, 0, _lib.ACC_DENSE),
    (32768, 768, 776, 200, 0, _lib.ACC_DENSE),
    (256, 512, 512, 50, 100, _lib.ACC_LOWRANK),
    (32768, 512, 520, 50, 200, _lib.ACC_LOWRANK),
    (1000, 520, 264, 63, 96, _lib.ACC_LOWRANK),
]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_flagged_queries_leave_out_the_accumulator_packs(shape, dt):
    """ws(PF | NATIVE) = ws(PF) - the 256-aligned packs of the accumulator tensors (2 bytes per element), for both queries; the
    flagged forward query is never 0; and it is the unflagged plan plus the packs of A, B and bias."""
    lib = _lib.load()
    T, d_in, d_out, r, r_acc, kind = shape
    acc_pack = (al256(2 * d_in * d_out) if kind == _lib.ACC_DENSE else al256(2 * d_in * r_acc) + al256(2 * r_acc * d_out))
    abb = al256(2 * d_in * r) + al256(2 * r * d_out) + al256(2 * d_out)
    for q in (lib.sow_workspace_bytes, lib.sow_forward_workspace_bytes):
        pf, both = q(T, d_in, d_out, r, r_acc, kind, dt | PF), q(T, d_in, d_out, r, r_acc, kind, dt | PF | NATIVE)
        assert both == pf - acc_pack, (q.__name__, pf, both, acc_pack)
        assert both > 0
    assert (lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt | PF | NATIVE)
            == lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt) + abb)
    own = lib.sow_forward_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt)
    assert lib.sow_forward_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt | PF | NATIVE) == (own + abb if own else abb + 256)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("r", [50, 200])
def test_without_accumulator_the_bit_changes_nothing(r, dt):
    lib = _lib.load()
    for T in (1000, 32768):
        for q in (lib.sow_workspace_bytes, lib.sow_forward_workspace_bytes):
            assert q(T, 768, 768, r, 0, _lib.ACC_NONE, dt | PF | NATIVE) == q(T, 768, 768, r, 0, _lib.ACC_NONE, dt | PF) > 0


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", SHAPES + [(1000, 768, 768, 50, 0, _lib.ACC_NONE)])
def test_the_bit_alone_is_ignored(shape, dt):
    """NATIVE without PARAM_F32: the accumulator is native already -- the unflagged answers, permissions included."""
    lib = _lib.load()
    T, d_in, d_out, r, r_acc, kind = shape
    for q in (lib.sow_workspace_bytes, lib.sow_forward_workspace_bytes):
        for perm in (0, _lib.FUSE_ACC, _lib.FUSE_ACC_DEEP):
            assert q(T, d_in, d_out, r, r_acc, kind, dt | NATIVE | perm) == q(T, d_in, d_out, r, r_acc, kind, dt | perm)
    # the permissions stay ignored next to PARAM_F32, with or without the bit
    for perm in (_lib.FUSE_ACC, _lib.FUSE_ACC_DEEP):
        assert (lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt | PF | NATIVE | perm)
                == lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt | PF | NATIVE))


def test_f32_compute_with_the_bit_is_a_dtype_error():
    """SOW_DTYPE_F32 takes neither flag: SOW_ERR_DTYPE from the layer entry points, 0 from the queries."""
    lib = _lib.load()
    arr = (_lib.LayerArgs * 1)()
    for code in (_lib.F32 | PF | NATIVE, _lib.F32 | NATIVE, _lib.F32 | PF):
        assert lib.sow_workspace_bytes(4096, 768, 768, 50, 0, _lib.ACC_DENSE, code) == 0
        assert lib.sow_forward_workspace_bytes(4096, 768, 768, 50, 0, _lib.ACC_DENSE, code) == 0
        assert lib.sow_forward(FAKE, FAKE, FAKE, FAKE, None, None, FAKE, FAKE, 64, 64, 64, 8, 0, _lib.ACC_DENSE, 1.0, code, FAKE,
                               1 << 20, None) == ERR_DTYPE
        assert lib.sow_backward(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE, None, 64, 64, 64, 8, 0, _lib.ACC_DENSE,
                                1.0, 0.0, code, FAKE, 1 << 20, None) == ERR_DTYPE
        assert lib.sow_forward_group(arr, 1, code, None) == ERR_DTYPE
        assert lib.sow_backward_group(arr, 1, code, _lib.BWD_DATA, None) == ERR_DTYPE
        assert lib.sow_reduce_batch(FAKE, FAKE, 1, 4, code, None) == ERR_DTYPE
        assert lib.sow_backward_group_plan(arr, 1, code, _lib.BWD_WEIGHTS, None) == ERR_DTYPE
        assert lib.sow_forward_skinny(arr, 1, code, None) == ERR_DTYPE


@pytest.mark.parametrize("dt", DTS)
def test_entry_points_that_refuse_param_f32_give_the_bit_the_same_code(dt):
    lib = _lib.load()
    arr = (_lib.LayerArgs * 2)()
    for i in range(2):
        arr[i].x, arr[i].A, arr[i].B, arr[i].y, arr[i].h_save = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
        arr[i].T, arr[i].d_in, arr[i].d_out, arr[i].r_live, arr[i].scale = 16384, 512, 512, 8, 1.0
    for code in (dt | PF, dt | PF | NATIVE, dt | NATIVE):
        assert lib.sow_forward_shared(arr, 2, code, None) == ERR_UNSUPPORTED
        assert lib.sow_backward_shared(arr, 2, code, _lib.BWD_DATA, None) == ERR_UNSUPPORTED
        assert lib.sow_gemm(FAKE, 64, 0, FAKE, 64, 0, FAKE, 64, None, 64, 64, 64, 1.0, 0.0, code, None) == ERR_DTYPE
        assert lib.sow_qr_thin(FAKE, 64, 64, 32, code, 8, FAKE, 8, None, 0, _lib.F32, FAKE, 1 << 20, None) == ERR_DTYPE
        assert lib.sow_axpby(FAKE, FAKE, 1024, 1.0, 1.0, code, None) == ERR_DTYPE
        assert lib.sow_cast_copy(FAKE, 64, code, FAKE, 64, code, 16, 64, None) == ERR_DTYPE
        assert lib.sow_accumulate_batch(None, 1, code, None) == ERR_DTYPE


@pytest.mark.parametrize("dt", DTS)
def test_reduce_descriptor_and_plan_ignore_the_bit(dt):
    """The weight-gradient phases read no accumulator: descriptor, block count and slab plan are those of PARAM_F32."""
    lib = _lib.load()
    T, d_in, d_out, r = 8192, 768, 776, 50
    nws = lib.sow_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_DENSE, dt | PF)
    got = []
    for code in (dt | PF, dt | PF | NATIVE, dt | NATIVE, dt):
        desc = ctypes.create_string_buffer(lib.sow_reduce_desc_bytes())
        blocks = ctypes.c_int(-1)
        rc = lib.sow_backward_reduce_desc(FAKE, FAKE, None, T, d_in, d_out, r, 0, _lib.ACC_DENSE, 1.0, code, FAKE, nws, desc,
                                          ctypes.byref(blocks))
        assert rc == 0, lib.sow_error_string(rc)
        got.append((blocks.value, desc.raw))
    assert got[0] == got[1] == got[2] == got[3]
    assert lib.sow_reduce_batch(FAKE, FAKE, 0, 0, dt | PF | NATIVE, None) == 0
    assert lib.sow_reduce_batch(FAKE, FAKE, 0, 0, dt | NATIVE, None) == 0


@pytest.mark.parametrize("dt", DTS)
def test_flagged_calls_check_before_launching(dt):
    """T = 0 is a no-op; a workspace of the unflagged plan cannot hold the packed factors: refused before the pack launch."""
    lib = _lib.load()
    code = dt | PF | NATIVE
    args = (64, 64, 64, 8, 0, _lib.ACC_DENSE)
    assert lib.sow_forward(FAKE, FAKE, FAKE, FAKE, None, None, FAKE, None, 0, *args[1:], 1.0, code, None, 0, None) == 0
    assert lib.sow_forward(FAKE, FAKE, FAKE, FAKE, None, None, FAKE, FAKE, *args, 1.0, code, None, 0, None) == -1
    small = lib.sow_workspace_bytes(*args, dt)
    assert lib.sow_forward(FAKE, FAKE, FAKE, FAKE, None, None, FAKE, FAKE, *args, 1.0, code, FAKE, small, None) == ERR_WORKSPACE
    assert lib.sow_backward(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE, None, *args, 1.0, 0.0, code, FAKE, small,
                            None) == ERR_WORKSPACE


SKINNY = [(4, 512, 512, 8), (17, 160, 136, 50), (32, 4096, 4096, 50), (1, 1024, 264, 64)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", SKINNY)
def test_skinny_queries_answer_for_the_pair_what_they_answer_for_the_compute_dtype(shape, dt):
    lib = _lib.load()
    T, d_in, d_out, r = shape
    for kind in (_lib.ACC_NONE, _lib.ACC_DENSE):
        plain = lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, kind, dt)
        assert plain > 0
        assert lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, kind, dt | PF | NATIVE) == plain
        assert lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, kind, dt | NATIVE) == plain
        assert lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, kind, dt | PF) == 0
    for q in (lib.sow_forward_skinny_fp8_workspace_bytes, lib.sow_forward_skinny_fp4_workspace_bytes):
        plain = q(T, d_in, d_out, r, dt)
        assert plain > 0
        assert q(T, d_in, d_out, r, dt | PF | NATIVE) == plain == q(T, d_in, d_out, r, dt | NATIVE)
        assert q(T, d_in, d_out, r, dt | PF) == 0
    # outside the admitted set the pair answers 0 as well
    assert lib.sow_forward_skinny_workspace_bytes(33, d_in, d_out, r, _lib.ACC_DENSE, dt | PF | NATIVE) == 0
    assert lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, _lib.ACC_LOWRANK, dt | PF | NATIVE) == 0


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", [_lib.ACC_NONE, _lib.ACC_DENSE, _lib.ACC_DENSE_FP8, _lib.ACC_DENSE_FP4])
def test_skinny_forward_admits_fp32_factors_next_to_the_bit_only(kind, dt):
    """PF | NATIVE gets past the refusal -- a deliberately short workspace is SOW_ERR_WORKSPACE, decided on the host before any
    launch or dereference --; PF alone is still SOW_ERR_UNSUPPORTED."""
    lib = _lib.load()
    arr = (_lib.LayerArgs * 1)()
    a = arr[0]
    a.x, a.A, a.B, a.y, a.bias = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    if kind != _lib.ACC_NONE:
        a.acc_down = 0x60000
    if kind in (_lib.ACC_DENSE_FP8, _lib.ACC_DENSE_FP4):
        a.acc_up = 0x70000
    a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = 4, 512, 512, 8, kind, 1.0
    a.workspace, a.workspace_bytes = 0x80000, 256
    assert lib.sow_forward_skinny(arr, 1, dt | PF | NATIVE, None) == ERR_WORKSPACE
    assert lib.sow_forward_skinny(arr, 1, dt | NATIVE, None) == ERR_WORKSPACE
    assert lib.sow_forward_skinny(arr, 1, dt, None) == ERR_WORKSPACE
    assert lib.sow_forward_skinny(arr, 1, dt | PF, None) == ERR_UNSUPPORTED
    # the other conditions are unchanged: a low-rank accumulator stays outside the set
    a.acc_kind, a.acc_up, a.r_acc = _lib.ACC_LOWRANK, 0x70000, 16
    assert lib.sow_forward_skinny(arr, 1, dt | PF | NATIVE, None) == ERR_UNSUPPORTED
