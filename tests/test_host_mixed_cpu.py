"""CPU tests of the SOW_PARAM_F32 surface of the C ABI (fp32 parameters with bf16 / f16 compute, as under torch.autocast; no
GPU compute): version, the flag's value, the workspace it needs, the deferred-reduction descriptor and the entry points that
refuse it on the host."""
import ctypes

import pytest

from sow_amd import _lib

FAKE = ctypes.c_void_p(0x10000)     # never dereferenced: every call below returns before a launch


def test_version_and_flag():
    lib = _lib.load()
    assert lib.sow_version() >= 114
    assert _lib.PARAM_F32 == 0x100


@pytest.mark.parametrize("r", [50, 200])
@pytest.mark.parametrize("dt", [_lib.BF16, _lib.F16])
@pytest.mark.parametrize("acc", [(_lib.ACC_NONE, 0), (_lib.ACC_DENSE, 0), (_lib.ACC_LOWRANK, 96)])
def test_flagged_workspace_holds_the_packed_parameters(r, dt, acc):
    lib = _lib.load()
    kind, r_acc = acc
    for T in (32768, 1000):
        plain = lib.sow_workspace_bytes(T, 768, 768, r, r_acc, kind, dt)
        mixed = lib.sow_workspace_bytes(T, 768, 768, r, r_acc, kind, dt | _lib.PARAM_F32)
        # A, B and bias in the compute dtype at least (2 bytes per element)
        assert mixed >= plain + 2 * (768 * r + r * 768 + 768)
        assert lib.sow_forward_workspace_bytes(T, 768, 768, r, r_acc, kind, dt | _lib.PARAM_F32) > 0
    assert lib.sow_workspace_bytes(4096, 768, 768, r, 0, _lib.ACC_NONE, _lib.F32 | _lib.PARAM_F32) == 0
    assert lib.sow_forward_workspace_bytes(4096, 768, 768, r, 0, _lib.ACC_NONE, _lib.F32 | _lib.PARAM_F32) == 0


@pytest.mark.parametrize("dt", [_lib.BF16, _lib.F16])
def test_flagged_forward_workspace_is_its_own_scratch_plus_the_packed_parameters(dt):
    """The flagged forward query adds the packed parameters to the unflagged forward figure; a forward that needs no scratch of
    its own (chain2 at long T) asks for the packed parameters only, far less than the backward workspace."""
    lib = _lib.load()
    flag = dt | _lib.PARAM_F32
    T, d = 32768, 768
    assert lib.sow_forward_workspace_bytes(T, d, d, 50, 0, _lib.ACC_NONE, dt) == 0
    lean = lib.sow_forward_workspace_bytes(T, d, d, 50, 0, _lib.ACC_NONE, flag)
    assert 2 * (d * 50 * 2 + d) <= lean <= 2 * (d * 50 * 2 + d) + 3 * 256 + 256
    assert lean < lib.sow_workspace_bytes(T, d, d, 50, 0, _lib.ACC_NONE, flag) // 10
    for shape in ((1000, d, d, 50, 0, _lib.ACC_NONE), (T, d, d, 200, 0, _lib.ACC_NONE), (T, 512, 520, 50, 200, _lib.ACC_LOWRANK)):
        own = lib.sow_forward_workspace_bytes(*shape, dt)
        assert own > 0
        assert lib.sow_forward_workspace_bytes(*shape, flag) > own


@pytest.mark.parametrize("r", [50, 63, 200])
@pytest.mark.parametrize("dt", [_lib.BF16, _lib.F16])
def test_reduce_descriptor_with_the_flag(r, dt):
    """Same block count as without the flag (r <= 64; the descriptor does not depend on the gradient dtype), 0 blocks for a
    wide layer, SOW_ERR_DTYPE for F32 | PARAM_F32."""
    lib = _lib.load()
    T, d_in, d_out = 8192, 768, 776
    nws = lib.sow_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_NONE, dt | _lib.PARAM_F32)
    counts = []
    for code in (dt, dt | _lib.PARAM_F32):
        desc = ctypes.create_string_buffer(lib.sow_reduce_desc_bytes())
        blocks = ctypes.c_int(-1)
        rc = lib.sow_backward_reduce_desc(FAKE, FAKE, None, T, d_in, d_out, r, 0, _lib.ACC_NONE, 1.0, code, FAKE, nws, desc,
                                          ctypes.byref(blocks))
        assert rc == 0, lib.sow_error_string(rc)
        counts.append((blocks.value, desc.raw))
    assert counts[0] == counts[1]
    assert counts[1][0] == (0 if r > 64 else (d_in + 3) // 4 + (d_out + 3) // 4)
    desc = ctypes.create_string_buffer(lib.sow_reduce_desc_bytes())
    blocks = ctypes.c_int(-1)
    assert lib.sow_backward_reduce_desc(FAKE, FAKE, None, T, d_in, d_out, r, 0, _lib.ACC_NONE, 1.0, _lib.F32 | _lib.PARAM_F32,
                                        FAKE, nws, desc, ctypes.byref(blocks)) == -3


@pytest.mark.parametrize("dt", [_lib.BF16, _lib.F16, _lib.F32])
def test_other_entry_points_refuse_the_flag(dt):
    lib = _lib.load()
    flagged = dt | _lib.PARAM_F32
    ERR_DTYPE = -3
    assert lib.sow_gemm(FAKE, 64, 0, FAKE, 64, 0, FAKE, 64, None, 64, 64, 64, 1.0, 0.0, flagged, None) == ERR_DTYPE
    assert lib.sow_gemm_ex(FAKE, 64, 0, FAKE, 64, 0, FAKE, 64, None, 64, 64, 64, 1.0, 0.0, flagged, None, 0, None) == ERR_DTYPE
    assert lib.sow_qr_thin(FAKE, 64, 64, 32, flagged, 8, FAKE, 8, None, 0, _lib.F32, FAKE, 1 << 20, None) == ERR_DTYPE
    assert lib.sow_qr_thin(FAKE, 64, 64, 32, _lib.F32, 8, FAKE, 8, None, 0, flagged, FAKE, 1 << 20, None) == ERR_DTYPE
    assert lib.sow_adamw_flat(FAKE, FAKE, FAKE, FAKE, 1024, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, flagged, _lib.F32,
                              None) == ERR_DTYPE
    assert lib.sow_adamw_flat(FAKE, FAKE, FAKE, FAKE, 1024, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, _lib.F32,
                              _lib.F32 | _lib.PARAM_F32, None) == ERR_DTYPE
    f32f = _lib.F32 | _lib.PARAM_F32
    assert lib.sow_cast_copy(FAKE, 64, f32f, FAKE, 64, f32f, 16, 64, None) == ERR_DTYPE
    assert lib.sow_axpby(FAKE, FAKE, 1024, 1.0, 1.0, flagged, None) == ERR_DTYPE
    assert lib.sow_accumulate_batch(None, 1, flagged, None) == ERR_DTYPE


def test_layer_entry_points_refuse_f32_compute():
    lib = _lib.load()
    f32f = _lib.F32 | _lib.PARAM_F32
    assert lib.sow_forward(FAKE, FAKE, FAKE, None, None, None, FAKE, FAKE, 64, 64, 64, 8, 0, 0, 1.0, f32f, FAKE, 1 << 20,
                           None) == -3
    assert lib.sow_backward(FAKE, FAKE, FAKE, FAKE, FAKE, None, None, FAKE, FAKE, FAKE, None, 64, 64, 64, 8, 0, 0, 1.0, 0.0, f32f,
                            FAKE, 1 << 20, None) == -3
    arr = (_lib.LayerArgs * 1)()
    assert lib.sow_forward_group(arr, 1, f32f, None) == -3
    assert lib.sow_backward_group(arr, 1, f32f, _lib.BWD_DATA, None) == -3
    assert lib.sow_reduce_batch(FAKE, FAKE, 1, 4, f32f, None) == -3


def test_flagged_calls_check_before_launching():
    """T = 0 is a no-op forward; a flagged forward without workspace is refused before the pack launch."""
    lib = _lib.load()
    code = _lib.BF16 | _lib.PARAM_F32
    assert lib.sow_forward(FAKE, FAKE, FAKE, None, None, None, FAKE, None, 0, 64, 64, 8, 0, 0, 1.0, code, None, 0, None) == 0
    assert lib.sow_forward(FAKE, FAKE, FAKE, None, None, None, FAKE, None, 64, 64, 64, 8, 0, 0, 1.0, code, None, 0, None) == -1
    small = lib.sow_workspace_bytes(64, 64, 64, 8, 0, 0, _lib.BF16)
    assert lib.sow_forward(FAKE, FAKE, FAKE, None, None, None, FAKE, None, 64, 64, 64, 8, 0, 0, 1.0, code, FAKE, small,
                           None) == -5
