"""CPU tests of the wide-rank surface of the C ABI (64 < r <= 256; no GPU compute): version, the NO_WIDE_CHAIN switch, the
empty deferred-reduction descriptor and the forward workspace a wide layer needs."""
import ctypes

import pytest

from sow_amd import _lib


def test_version_and_switch():
    lib = _lib.load()
    assert lib.sow_version() >= 113
    assert lib.sow_get_switch(b"NO_WIDE_CHAIN") in (-1, 0, 1)     # SOW_ERR_UNSUPPORTED (-6) for an unknown name
    saved = lib.sow_get_switch(b"NO_WIDE_CHAIN")
    try:
        assert lib.sow_set_switch(b"NO_WIDE_CHAIN", 1) == 0
        assert lib.sow_get_switch(b"NO_WIDE_CHAIN") == 1
    finally:
        lib.sow_set_switch(b"NO_WIDE_CHAIN", saved)


@pytest.mark.parametrize("r", [65, 96, 200, 256, 300])
@pytest.mark.parametrize("dtype", [_lib.BF16, _lib.F16, _lib.F32])
def test_wide_reduce_descriptor_is_empty(r, dtype):
    """PARTIAL finishes a wide layer's gradients: its deferred reduction is a valid descriptor with no blocks."""
    lib = _lib.load()
    T, d_in, d_out = 4096, 512, 520
    nws = lib.sow_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_NONE, dtype)
    assert nws > 0
    fake = ctypes.c_void_p(0x10000)      # never dereferenced: the descriptor is built on the host
    desc = ctypes.create_string_buffer(lib.sow_reduce_desc_bytes())
    blocks = ctypes.c_int(-1)
    for dbias in (None, fake):
        rc = lib.sow_backward_reduce_desc(fake, fake, dbias, T, d_in, d_out, r, 0, _lib.ACC_NONE, 0.0, dtype, fake, nws, desc,
                                          ctypes.byref(blocks))
        assert rc == 0 and blocks.value == 0


def test_wide_forward_needs_workspace():
    lib = _lib.load()
    # generic path (fp32): the projection goes to the workspace when the caller passes no h_save
    assert lib.sow_forward_workspace_bytes(4096, 512, 264, 96, 0, _lib.ACC_NONE, _lib.F32) > 0
    # fused chain: the packed factors
    for dt in (_lib.BF16, _lib.F16):
        assert lib.sow_forward_workspace_bytes(32768, 2048, 2048, 200, 0, _lib.ACC_NONE, dt) > 0
    # nothing changes at r <= 64
    assert lib.sow_forward_workspace_bytes(32768, 2048, 2048, 50, 0, _lib.ACC_NONE, _lib.BF16) == 0
