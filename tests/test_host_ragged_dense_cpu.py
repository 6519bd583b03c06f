"""CPU tests of the host side of the ragged dense-accumulator route (api.hip: rag_layer admits SOW_ACC_DENSE): the library
version, the NO_RAGGED_GEMM switch, and the workspace plan of 2048 <-> 5461 layers with a dense accumulator -- it holds the
factor pack of chain_wide and the slab partials of skinny_tn_wide, so it is at least the plan of the aligned neighbour
5456, and it is a pure function of the shape: the same under every combination of NO_RAGGED and NO_RAGGED_GEMM.  No GPU
work is attempted."""
import itertools

import pytest

from sow_amd import _lib


def test_version_is_at_least_116():
    assert _lib.load().sow_version() >= 116


def test_no_ragged_gemm_switch_can_be_set_read_and_restored():
    lib = _lib.load()
    old = lib.sow_get_switch(b"NO_RAGGED_GEMM")
    assert old in (-1, 0, 1), "the switch table has no NO_RAGGED_GEMM"
    try:
        assert lib.sow_set_switch(b"NO_RAGGED_GEMM", 1) == 0 and lib.sow_get_switch(b"NO_RAGGED_GEMM") == 1
        assert lib.sow_set_switch(b"NO_RAGGED_GEMM", 0) == 0 and lib.sow_get_switch(b"NO_RAGGED_GEMM") == 0
        assert lib.sow_set_switch(b"NO_RAGGED_GEMM", -1) == 0 and lib.sow_get_switch(b"NO_RAGGED_GEMM") == -1
        with _lib.switch(NO_RAGGED_GEMM=1):
            assert lib.sow_get_switch(b"NO_RAGGED_GEMM") == 1
        assert lib.sow_get_switch(b"NO_RAGGED_GEMM") == -1
        # a switch of its own: setting it leaves NO_RAGGED alone
        before = lib.sow_get_switch(b"NO_RAGGED")
        with _lib.switch(NO_RAGGED_GEMM=1):
            assert lib.sow_get_switch(b"NO_RAGGED") == before
    finally:
        lib.sow_set_switch(b"NO_RAGGED_GEMM", old)
    assert lib.sow_get_switch(b"NO_RAGGED_GEMM") == old


DTYPES = [_lib.BF16, _lib.F16, _lib.BF16 | _lib.PARAM_F32, _lib.F16 | _lib.PARAM_F32]


@pytest.mark.parametrize("T", [1, 1000, 4096, 32768])
@pytest.mark.parametrize("r", [66, 200, 256])
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16", "bf16_param_f32", "f16_param_f32"])
def test_workspace_plan_of_ragged_dense_layers(T, r, dt):
    """sow_workspace_bytes / sow_forward_workspace_bytes of 2048 <-> 5461 with ACC_DENSE >= those of 2048 <-> 5456, and
    identical under every combination of the two switches."""
    lib = _lib.load()
    for d_in, d_out, a_in, a_out in ((2048, 5461, 2048, 5456), (5461, 2048, 5456, 2048)):
        seen = set()
        for nr, ng in itertools.product((-1, 1), (-1, 1)):
            with _lib.switch(NO_RAGGED=nr, NO_RAGGED_GEMM=ng):
                full = lib.sow_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_DENSE, dt)
                fwd = lib.sow_forward_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_DENSE, dt)
                full_al = lib.sow_workspace_bytes(T, a_in, a_out, r, 0, _lib.ACC_DENSE, dt)
                fwd_al = lib.sow_forward_workspace_bytes(T, a_in, a_out, r, 0, _lib.ACC_DENSE, dt)
            assert full >= full_al > 0, (d_in, d_out, nr, ng, full, full_al)
            assert fwd >= fwd_al > 0, (d_in, d_out, nr, ng, fwd, fwd_al)
            seen.add((full, fwd))
        assert len(seen) == 1, f"the plan of {d_in} x {d_out} depends on a switch: {sorted(seen)}"
