"""CPU tests of the ragged-width surface of the C ABI (bf16 / f16 layers with d_in or d_out not a multiple of 8 and
64 < r <= 256; no GPU compute): the NO_RAGGED switch, the workspace the fused ragged kernels need, and the plans of a
llama_1b decoder block (hidden 2048, intermediate 5461)."""
import ctypes

import pytest

from sow_amd import _lib

FAKE = 0x10000          # never dereferenced: plans and descriptors are built on the host


def test_version_and_no_ragged_switch():
    lib = _lib.load()
    assert lib.sow_version() >= 115
    saved = lib.sow_get_switch(b"NO_RAGGED")
    assert saved in (-1, 0, 1)            # an unknown name returns SOW_ERR_UNSUPPORTED
    try:
        assert lib.sow_set_switch(b"NO_RAGGED", 1) == 0
        assert lib.sow_get_switch(b"NO_RAGGED") == 1
        assert lib.sow_set_switch(b"NO_RAGGED", 0) == 0
        assert lib.sow_get_switch(b"NO_RAGGED") == 0
    finally:
        lib.sow_set_switch(b"NO_RAGGED", saved)
    assert lib.sow_get_switch(b"NO_RAGGED") == saved
    with _lib.switch(NO_RAGGED=1):
        assert lib.sow_get_switch(b"NO_RAGGED") == 1
    assert lib.sow_get_switch(b"NO_RAGGED") == saved


@pytest.mark.parametrize("dtype", [_lib.BF16, _lib.F16, _lib.BF16 | _lib.PARAM_F32, _lib.F16 | _lib.PARAM_F32])
@pytest.mark.parametrize("r", [66, 200, 256])
@pytest.mark.parametrize("direction", ["up", "down"])
def test_workspace_covers_the_ragged_kernels(dtype, r, direction):
    """A 5461-wide layer plans at least what its aligned neighbour 5456 plans (the factor pack and the weight-gradient slab
    partials), whatever the NO_RAGGED switch says."""
    lib = _lib.load()
    T = 32768

    def shape(d):
        return (2048, d) if direction == "up" else (d, 2048)

    for no_ragged in (0, 1):
        with _lib.switch(NO_RAGGED=no_ragged):
            rag = lib.sow_workspace_bytes(T, *shape(5461), r, 0, _lib.ACC_NONE, dtype)
            ali = lib.sow_workspace_bytes(T, *shape(5456), r, 0, _lib.ACC_NONE, dtype)
            assert rag >= ali > 0
            frag = lib.sow_forward_workspace_bytes(T, *shape(5461), r, 0, _lib.ACC_NONE, dtype)
            fali = lib.sow_forward_workspace_bytes(T, *shape(5456), r, 0, _lib.ACC_NONE, dtype)
            assert frag >= fali
            assert frag > 0            # the factor pack of the fused chain
            assert frag <= rag
            plans = (rag, frag)
        if no_ragged == 0:
            first = plans
        else:
            assert plans == first       # the plan does not depend on the switch


def test_workspace_of_a_ragged_lowrank_accumulator():
    lib = _lib.load()
    for r_acc in (32, 200, 256):
        rag = lib.sow_forward_workspace_bytes(32768, 2048, 5461, 200, r_acc, _lib.ACC_LOWRANK, _lib.BF16)
        ali = lib.sow_forward_workspace_bytes(32768, 2048, 5456, 200, r_acc, _lib.ACC_LOWRANK, _lib.BF16)
        assert rag >= ali > 0
        assert lib.sow_workspace_bytes(32768, 2048, 5461, 200, r_acc, _lib.ACC_LOWRANK, _lib.BF16) >= rag


def test_aligned_and_unadmitted_layers_keep_their_plans():
    lib = _lib.load()
    # r <= 64 is not admitted (measured slower than the generic kernels): no forward scratch, as before
    for d_out in (2048, 5461):
        assert lib.sow_forward_workspace_bytes(32768, 2048, d_out, 50, 0, _lib.ACC_NONE, _lib.BF16) == 0
        assert lib.sow_forward_workspace_bytes(32768, 2048, d_out, 50, 32, _lib.ACC_LOWRANK, _lib.BF16) == 0


def _block(T, r, ws_bytes):
    """The seven SoW layers of a llama_1b decoder block (q, k, v, o: 2048 -> 2048; gate, up: 2048 -> 5461; down: 5461 ->
    2048), without bias, as a sow_layer_args array."""
    shapes = [(2048, 2048)] * 4 + [(2048, 5461), (2048, 5461), (5461, 2048)]
    arr = (_lib.LayerArgs * len(shapes))()
    for a, (d_in, d_out) in zip(arr, shapes):
        for f in ("x", "A", "B", "y", "h_save", "dy", "dx", "dA", "dB", "workspace"):
            setattr(a, f, FAKE)
        a.T, a.d_in, a.d_out, a.r_live, a.r_acc, a.acc_kind = T, d_in, d_out, r, 0, _lib.ACC_NONE
        a.scale, a.grad_beta = 0.5, 1.0
        a.workspace_bytes = ws_bytes(T, d_in, d_out, r)
    return arr, shapes


@pytest.mark.parametrize("r", [50, 200])
def test_llama_1b_block_plans(r):
    lib = _lib.load()
    T = 32768

    def ws(T, d_in, d_out, r):
        return lib.sow_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_NONE, _lib.BF16) + 256

    arr, shapes = _block(T, r, ws)
    n = len(shapes)
    phases = _lib.BWD_WEIGHTS_PARTIAL | _lib.BWD_GROUP_SLABS
    results = []
    for _ in range(2):
        slabs = (ctypes.c_int * (2 * n))()
        rc = lib.sow_backward_group_plan(arr, n, _lib.BF16, phases, slabs)
        assert rc in (0, 1)
        descs = ctypes.create_string_buffer(n * lib.sow_reduce_desc_bytes())
        blocks = (ctypes.c_int * n)()
        assert lib.sow_backward_group_reduce_desc(arr, n, _lib.BF16, phases, descs, blocks) == 0
        results.append((rc, list(slabs), descs.raw, list(blocks)))
    assert results[0] == results[1]             # a pure function of the layer list
    blocks = results[0][3]
    for b in blocks:
        assert (b == 0) == (r > 64)             # PARTIAL finishes a wide layer, ragged or not: an empty descriptor
