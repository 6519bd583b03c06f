"""CPU tests of the host side of the f16 weight-gradient dispatch (no launch: sow_backward_group_plan,
sow_backward_group_reduce_desc and sow_workspace_bytes are host logic only).

f16 takes the bf16 plans -- the row-owner plan of a decoder block, the slab capacity of the workspace, the reduction
descriptors -- with one deliberate asymmetry: the row-owner plan needs SOW_BWD_GROUP_SLABS (a deferred reduction); a call that
runs both weight phases itself keeps the column-owner kernel, whose grouped results are pinned bit-identical to single calls
(tests/test_gpu_f16.py).  NO_F16_TN switches all of it off.  The last test shows that the coverage checks of the fuzz and
value sweeps stay satisfiable once the aligned f16 cases leave the generic weight-gradient kernel."""
import ctypes
import os

import fuzz_plan as FP
import value_plan as V
from sow_amd import _lib

FAKE = 1 << 20    # the plans look at alignment and sizes only; nothing is dereferenced
T = 32768
BLOCK = [(512, 512)] * 4 + [(512, 1376)] * 2 + [(1376, 512)]    # the seven projections of a llama_60m decoder block
DEFERRED = _lib.BWD_WEIGHTS_PARTIAL | _lib.BWD_GROUP_SLABS


def _layers(dt, shapes=BLOCK, T=T, r=50):
    lib = _lib.load()
    arr = (_lib.LayerArgs * len(shapes))()
    for i, (d_in, d_out) in enumerate(shapes):
        ws = lib.sow_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_NONE, dt)
        arr[i] = _lib.LayerArgs(x=FAKE, A=FAKE, B=FAKE, y=FAKE, h_save=FAKE, dy=FAKE, dx=FAKE, dA=FAKE, dB=FAKE, T=T, d_in=d_in,
                                d_out=d_out, r_live=r, r_acc=0, acc_kind=_lib.ACC_NONE, scale=1.0, grad_beta=0.0,
                                workspace=FAKE, workspace_bytes=ws + 256)
    return arr


def _plan(dt, phases, shapes=BLOCK):
    arr = _layers(dt, shapes)
    slabs = (ctypes.c_int * (2 * len(shapes)))()
    return _lib.load().sow_backward_group_plan(arr, len(shapes), dt, phases, slabs), list(slabs)


def test_f16_block_takes_the_row_owner_plan_only_with_a_deferred_reduction():
    """The bf16 plan for SOW_BWD_GROUP_SLABS; none for one call with DATA | WEIGHTS -- the asymmetry with bf16, which plans
    the row-owner kernel there too."""
    rows, slabs = _plan(_lib.BF16, DEFERRED)
    assert rows == 1 and slabs == [13] * 9 + [18, 13, 18, 18, 13]
    assert _plan(_lib.F16, DEFERRED) == (1, slabs)
    assert _plan(_lib.F16 | _lib.PARAM_F32, DEFERRED) == (1, slabs)
    assert _plan(_lib.F16, _lib.BWD_WEIGHTS_REDUCE | _lib.BWD_GROUP_SLABS) == (1, slabs)
    full = _lib.BWD_DATA | _lib.BWD_WEIGHTS
    single = [32] * 8 + [16] * 6
    assert _plan(_lib.BF16, full)[0] == 1
    assert _plan(_lib.F16, full) == (0, single)
    assert _plan(_lib.F16, _lib.BWD_WEIGHTS) == (0, single)
    assert _plan(_lib.F16, _lib.BWD_WEIGHTS_PARTIAL) == (0, single)


def test_switches_send_f16_back():
    lib = _lib.load()
    with _lib.switch(NO_F16_TN=1):
        assert _plan(_lib.F16, DEFERRED)[0] == 0
        assert _plan(_lib.BF16, DEFERRED)[0] == 1      # bf16 does not look at the switch
        # the workspace query does not shrink under the switch: the plan of the workspace is a function of shape and dtype
        assert (lib.sow_workspace_bytes(T, 512, 512, 50, 0, _lib.ACC_NONE, _lib.F16)
                == lib.sow_workspace_bytes(T, 512, 512, 50, 0, _lib.ACC_NONE, _lib.BF16))
    with _lib.switch(NO_TN_ROWS=1):
        assert _plan(_lib.F16, DEFERRED)[0] == 0
    assert _plan(_lib.F16, DEFERRED)[0] == 1


def test_reduce_descriptors_of_an_f16_block_have_the_bf16_block_counts():
    lib = _lib.load()
    size = lib.sow_reduce_desc_bytes()
    out = {}
    for dt in (_lib.BF16, _lib.F16):
        arr = _layers(dt)
        raw = ctypes.create_string_buffer(size * len(BLOCK))
        blocks = (ctypes.c_int * len(BLOCK))()
        _lib.check(lib.sow_backward_group_reduce_desc(arr, len(BLOCK), dt, DEFERRED, raw, blocks), "reduce_desc")
        out[dt] = (list(blocks), raw.raw)
    assert out[_lib.F16][0] == out[_lib.BF16][0] and all(b > 0 for b in out[_lib.F16][0])
    # same pointers, same workspace offsets, same group-planned slab counts: the descriptors themselves agree
    assert out[_lib.F16][1] == out[_lib.BF16][1]


def test_f16_workspace_has_the_bf16_slab_capacity():
    lib = _lib.load()
    shapes = [(32768, 512, 512, 50), (32768, 512, 1376, 50), (32768, 1376, 512, 50), (8193, 256, 264, 50), (1024, 4096, 4096, 8),
              (1024, 4096, 11008, 8), (4096, 768, 768, 64), (2048, 512, 264, 63)]
    for Tt, d_in, d_out, r in shapes:
        for kind, r_acc in ((_lib.ACC_NONE, 0), (_lib.ACC_LOWRANK, 32), (_lib.ACC_LOWRANK, 96)):
            f16 = lib.sow_workspace_bytes(Tt, d_in, d_out, r, r_acc, kind, _lib.F16)
            bf16 = lib.sow_workspace_bytes(Tt, d_in, d_out, r, r_acc, kind, _lib.BF16)
            assert f16 == bf16, (Tt, d_in, d_out, r, kind, r_acc, f16, bf16)


def test_no_f16_tn_switch_exists_and_is_unset_by_default():
    lib = _lib.load()
    assert lib.sow_version() >= 120
    if "SOW_AMD_NO_F16_TN" not in os.environ:
        assert lib.sow_get_switch(b"NO_F16_TN") == -1
    with _lib.switch(NO_F16_TN=1):
        assert lib.sow_get_switch(b"NO_F16_TN") == 1
    assert lib.sow_get_switch(b"NO_F16_TN") in (-1, 0, 1)


def _reaches_generic_tn(c):
    """launch_tn of skinny_tn.hip for a layer of the sweep with r <= 64: the LDS-DMA kernels want 16-byte-aligned views and
    widths that are multiples of 8 elements (fp32: of 4); everything else runs tn_partial_kernel, in every dtype."""
    if c.r > 64 or not c.save_h:
        return False
    mult = 4 if c.dtype == "f32" else 8
    return bool(c.misalign or c.d_in % mult or c.d_out % mult)


def test_generic_weight_gradient_kernel_keeps_its_coverage():
    """test_zz_fuzz_coverage wants >= 3 cases per family, test_zz_value_coverage an exact case: the ragged and misaligned
    layers of the plan keep tn_partial_kernel when aligned f16 layers move to the LDS-DMA kernels."""
    generic = [c for c in FP.plan().layers if _reaches_generic_tn(c)]
    assert len(generic) >= 3, [c.name for c in generic]
    assert {c.dtype for c in generic} == {"bf16", "f16", "f32"}
    taken = [c for c in V.cases().layers if _reaches_generic_tn(c)]
    assert taken and all((c.dtype, c.edges[0]) in V.GENERIC for c in taken if c.stratum == "generic"), [c.name for c in taken]
