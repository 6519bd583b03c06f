"""-m gpu: float16 weight gradients on the LDS-DMA kernels of skinny_tn.hip -- the column-owner kernels
(tn_partial_dma_wide_kernel<f16>, tn_partial_dma_kernel<f16> under TN_NARROW) for single layers and small groups, the
row-owner kernel (tn_partial_rows_kernel<f16>) for a group with a deferred reduction (SOW_BWD_GROUP_SLABS) -- through the
element-wise harness of tests/test_gpu_elementwise.py: NaN-neighboured inputs, sentinel guards, three runs (poisoned,
zeroed, poisoned) that must be bit-identical, every stage against float64.  The trace of the third run must hold the named
f16 kernel and must not hold the generic tn_partial_kernel (ragged widths, misaligned views and the NO_F16_TN switch: the
other way round).

Exact operands (tests/value_plan.py, family A: every stored intermediate representable, every sum below 2^24 units --
proved on the CPU before the run) with fp32 gradients (SOW_PARAM_F32) make dA, dB and dbias equal RNE(ref64) bit for bit: one
dropped token of 32769 fails.  One NaN in dY at the last token of the last slab must reach exactly the elements the
float64 reference says and leave everything else, the other members of a group included, bit-identical.
"""
import ctypes
import dataclasses
import functools

import pytest
import torch
from torch import nn

import fuzz_plan as FP
import test_gpu_autocast as AC
import test_gpu_elementwise as E
import test_gpu_fuzz_elementwise as Z
import value_plan as V
from numerics import UNIT_ROUNDOFF, accumulation_term, bound, check_bound, check_rounded, fp32_floor, rne, to64
from sow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, F32 = torch.float16, torch.float32
WIDE, NARROW, ROWS, GENERIC = ("tn_partial_dma_wide_kernel", "tn_partial_dma_kernel", "tn_partial_rows_kernel",
                               "tn_partial_kernel")
FULL = _lib.BWD_DATA | _lib.BWD_WEIGHTS
DEFERRED = _lib.BWD_DATA | _lib.BWD_WEIGHTS_PARTIAL | _lib.BWD_GROUP_SLABS
KEYS = ("y", "h", "dx", "dA", "dB", "dbias")


def _f16_form(seq, kernel):
    """Launches of the f16 instantiation of `kernel` in a trace: the template of that name ("sow::name<_Float16>" demangled,
    "<len>nameIDF16_" mangled); the plain name is the bf16 kernel."""
    return [n for n in seq if f"sow::{kernel}<" in n or f"{len(kernel)}{kernel}I" in n]


def _expect(seq, kernel, name):
    """The trace holds `kernel` (its f16 form where it has two) and no other weight-gradient partial kernel."""
    names = sorted(set(seq))
    if kernel == GENERIC:
        assert Z._has(seq, GENERIC), f"{name}: expected the generic tn_partial_kernel, the trace holds {names}"
        for k in (WIDE, NARROW, ROWS):
            assert not Z._has(seq, k), f"{name}: {k} ran where the generic kernel is expected: {names}"
        return
    assert _f16_form(seq, kernel), f"{name}: expected the f16 form of {kernel}, the trace holds {names}"
    assert not Z._has(seq, GENERIC), f"{name}: the generic tn_partial_kernel ran: {names}"
    for k in (WIDE, NARROW, ROWS):
        if k != kernel:
            assert not Z._has(seq, k), f"{name}: {k} ran beside {kernel}: {names}"


# ------------------------------------------------------------------------------------------------------------ single layers
# (case, kernel the weight gradients must run on)
LAYERS = [
    # one-token last slab (T = 16 * 512 + 1), 8-column last column group (264 = 4 * 64 + 8)
    (E.Case("f16_wide_T8193", F16, 8193, 512, 264, 50, s=0.5), WIDE),
    (E.Case("f16_wide_T32769_r64_colsum", F16, 32769, 256, 520, 64), WIDE),              # r = 64: dbias by colsum_kernel
    (E.Case("f16_wide_T4097_r63_ones", F16, 4097, 512, 264, 63), WIDE),                  # the ones column is the last free one
    (E.Case("f16_wide_T32769_grad_beta", F16, 32769, 256, 264, 50, grad_beta=1.0), WIDE),
    (E.Case("f16_wide_short_T65", F16, 65, 1024, 1032, 50), WIDE),
    (E.Case("f16_wide_T1", F16, 1, 64, 72, 4), WIDE),                                    # 63 of 64 tokens from the zero page
    (E.Case("f16_narrow_T8193", F16, 8193, 512, 264, 50, s=0.5, switches=dict(TN_NARROW=1)), NARROW),
    (E.Case("f16_misaligned_T8193", F16, 8193, 512, 264, 50, s=0.5, misalign=1), GENERIC),
    (E.Case("f16_ragged_T1485", F16, 1485, 343, 280, 48), GENERIC),
    (E.Case("f16_switch_off_T8193", F16, 8193, 512, 264, 50, s=0.5, switches=dict(NO_F16_TN=1)), GENERIC),
]


@functools.lru_cache(maxsize=None)
def _gauss(c_key):
    """Gaussian operands of a case (test_gpu_elementwise._inputs), drawn once per case and never modified."""
    return E._inputs(_CASE_OF[c_key])


_CASE_OF = {}


def _data(c):
    _CASE_OF[c.name] = c
    return _gauss(c.name)


@pytest.mark.parametrize("c,kernel", LAYERS, ids=[c.name for c, _ in LAYERS])
def test_f16_layer_kernel_and_values(c, kernel):
    d = _data(c)
    trace = {}
    out = E._run_single(c, d, trace)
    _expect(trace["bwd"], kernel, c.name)
    if c.name.endswith("colsum"):
        assert Z._has(trace["bwd"], "colsum_kernel"), sorted(set(trace["bwd"]))
    E._check(c, d, out)


# ------------------------------------------------------------------------------------------------------------------ groups
def _L(name, T, d_in, d_out, r, bias=True, s=1.0):
    return FP.Layer(name, "f16", T, d_in, d_out, r, bias=bias, s=s, stratum="chain2")


COLUMN_GROUP = [_L("g0", 8193, 256, 264, 50, s=0.5), _L("g1", 8193, 256, 512, 16, bias=False), _L("g2", 8193, 256, 136, 8)]
# one column group per wave (every operand has at most 8 groups of 64 columns)
ROWS_GROUP_1 = [_L("g0", 32769, 256, 264, 50), _L("g1", 32769, 256, 256, 16, bias=False, s=0.5), _L("g2", 32769, 256, 264, 8),
                _L("g3", 32769, 256, 256, 62)]
# two column groups per wave: the 1032-wide operands have 17 column groups in two ranges of 9
ROWS_GROUP_2 = [_L("g0", 32769, 256, 264, 50), _L("g1", 32769, 256, 1032, 16, bias=False, s=0.5),
                _L("g2", 32769, 1032, 256, 8), _L("g3", 32769, 264, 256, 62)]


def _group(name, members, deferred, rows):
    ms = [dataclasses.replace(c, name=f"{name}.{c.name}", seed=i) for i, c in enumerate(members)]
    return FP.Group(name, ms, deferred=deferred, rows=rows), [Z._to_case(c, "once", "once") for c in ms]


def _c_plan(members, dt, phases):
    """sow_backward_group_plan on the shapes alone (host logic: nothing is dereferenced)."""
    lib = _lib.load()
    fake = 1 << 20
    arr = (_lib.LayerArgs * len(members))()
    for i, c in enumerate(members):
        ws = lib.sow_workspace_bytes(c.T, c.d_in, c.d_out, c.r, 0, _lib.ACC_NONE, dt)
        arr[i] = _lib.LayerArgs(x=fake, A=fake, B=fake, y=fake, h_save=fake, dy=fake, dx=fake, dA=fake, dB=fake,
                                dbias=fake if c.bias else None, T=c.T, d_in=c.d_in, d_out=c.d_out, r_live=c.r, r_acc=0,
                                acc_kind=_lib.ACC_NONE, scale=c.s, grad_beta=0.0, workspace=fake, workspace_bytes=ws + 256)
    slabs = (ctypes.c_int * (2 * len(members)))()
    return lib.sow_backward_group_plan(arr, len(members), dt, phases, slabs), list(slabs)


def _py_rows_plan(members):
    return FP.tn_rows_plan([m.T for m in members for _ in range(2)], [v for m in members for v in (m.d_in, m.d_out)])


_GROUP_DATA = {}


def _group_data(name, layers):
    """Gaussian operands of a group's members, drawn once per group and shared by the tests that run it."""
    if name not in _GROUP_DATA:
        _GROUP_DATA[name] = [E._inputs(c) for c in layers]
    return _GROUP_DATA[name]


def _same_as_single_calls(layers, data, outs, keys=KEYS):
    for c, d, out in zip(layers, data, outs):
        single = E._run_single(c, d)
        for k in keys:
            if out.get(k) is not None:
                assert torch.equal(E._bits(out[k]), E._bits(single[k])), f"{c.name}: {k} of the grouped call differs from the single call"


def test_f16_column_owner_group_is_one_launch_and_bit_identical_to_single_calls():
    gp, layers = _group("f16_group3_T8193", COLUMN_GROUP, deferred=False, rows=False)
    assert _c_plan(COLUMN_GROUP, _lib.F16, FULL)[0] == 0
    data = _group_data(gp.name, layers)
    outs, seq = Z.run_group(gp, layers, data)
    _expect(seq, WIDE, gp.name)
    assert len(_f16_form(seq, WIDE)) == 1, f"{gp.name}: one grouped column-owner launch expected: {_f16_form(seq, WIDE)}"
    for c, d, out in zip(layers, data, outs):
        E._check(c, d, out)
    _same_as_single_calls(layers, data, outs)


@pytest.mark.parametrize("members", [ROWS_GROUP_1, ROWS_GROUP_2], ids=["one_group_per_wave", "two_groups_per_wave"])
def test_f16_row_owner_group_with_a_deferred_reduction(members):
    name = "f16_rows_cgw1" if members is ROWS_GROUP_1 else "f16_rows_cgw2"
    assert _py_rows_plan(members)
    rows, slabs = _c_plan(members, _lib.F16, DEFERRED)
    assert (rows, slabs) == _c_plan(members, _lib.BF16, DEFERRED) and rows == 1
    if members is ROWS_GROUP_2:   # an operand past 16 column groups: two ranges, two groups per wave
        assert any((d + 63) // 64 > 16 for c in members for d in (c.d_in, c.d_out))
    gp, layers = _group(name, members, deferred=True, rows=True)
    data = _group_data(name, layers)
    outs, seq = Z.run_group(gp, layers, data)
    _expect(seq, ROWS, name)
    for c, d, out in zip(layers, data, outs):
        E._check(c, d, out)


def test_f16_default_phases_keep_the_column_owner_kernel_and_single_call_bits():
    """The asymmetry with bf16: DATA | WEIGHTS on a set the row-owner plan accepts keeps the column-owner kernel in f16, and
    the gradients stay bit-identical to single calls."""
    members = ROWS_GROUP_2
    assert _c_plan(members, _lib.F16, FULL)[0] == 0 and _c_plan(members, _lib.BF16, FULL)[0] == 1
    gp, layers = _group("f16_rows_cgw2", members, deferred=False, rows=False)    # the name keys the shared operands
    data = _group_data(gp.name, layers)
    outs, seq = Z.run_group(gp, layers, data)
    _expect(seq, WIDE, gp.name + " (default phases)")
    _same_as_single_calls(layers, data, outs, keys=("dA", "dB", "dbias"))


# ---------------------------------------------------------------------------------------- exact operands, fp32 gradients
def _exact(out, ref, dtype, name):
    """Bit equality with rne(ref64, dtype) (zeros compared as zeros)."""
    check_rounded(out, ref, dtype, max_ulp=0, max_inexact=0, min_count=0, name=name)
    want = rne(ref, dtype).to(dtype)
    assert torch.equal(E._bits(out.cpu() + 0), E._bits(want + 0)), f"{name}: bits differ from rne(ref64)"


def _h_full(c, f):
    h = torch.zeros(c.T, 64, dtype=torch.float64)
    h[:, :c.r] = f["h"]
    if c.r <= 63:
        h[:, 63] = 1.0
    return h


def _proved(c):
    """Family-A operands and references; V.exact_layer_proved raises NotExact unless every stored intermediate is
    representable in f16 and every sum stays below 2^24 units -- and, for these long-T chain2 cases, unless dA, dB and dbias
    are representable in fp32 (value_plan.check_density)."""
    assert V.f32_gradients(c)
    d, f = V.exact_layer_proved(c)
    assert {"h", "dh", "dA", "dB", "dx", "y"} <= set(f["_sums"])   # (the proof ran: every sum of the layer is recorded)
    return d, f


def test_exact_f16_layer_with_fp32_gradients():
    c = _L("f16_exact_T8193", 8193, 512, 264, 50, s=0.5)
    d, f = _proved(c)
    da = dict(x=d["x"], A=d["A"], B=d["B"], bias=d.get("bias"), dy=d["dy"], acc_down=None, acc_up=None, dA0=None, dB0=None,
              dbias0=None)
    res = {}
    seq = E._kernel_seq(lambda: res.update(AC._run(da, F16, c.T, c.d_in, c.d_out, c.r, None, 0, c.s, True)))
    _expect(seq, WIDE, c.name)
    for k in ("dA", "dB", "dbias"):
        assert res[k].dtype == F32
        _exact(res[k].cpu(), f[k], F32, f"{c.name}: {k}")
    _exact(res["h"].cpu(), _h_full(c, f), F16, f"{c.name}: h_save")
    _exact(res["y"].cpu(), f["y"], F16, f"{c.name}: y")
    _exact(res["dx"].cpu(), f["dx"], F16, f"{c.name}: dx")


def _run_group_param_f32(members, data):
    """sow_forward_group + sow_backward_group(DATA | PARTIAL | GROUP_SLABS) + sow_reduce_batch with SOW_DTYPE_F16 |
    SOW_PARAM_F32: f16 activations, fp32 factors and gradients.  Two runs (poisoned, zeroed) that must be bit-identical,
    guards intact; returns (outputs of the first per member, kernel names of the second)."""
    lib = _lib.load()
    code = _lib.F16 | _lib.PARAM_F32
    n = len(members)
    ar = AC.Arena()
    arr = (_lib.LayerArgs * n)()
    bufs = []
    for i, (c, d) in enumerate(zip(members, data)):
        b = dict(x=ar.input(d["x"], F16), A=ar.input(d["A"], F32), B=ar.input(d["B"], F32), bias=ar.input(d.get("bias"), F32),
                 dy=ar.input(d["dy"], F16), y=ar.output((c.T, c.d_out), F16), h=ar.output((c.T, 64), F16),
                 dx=ar.output((c.T, c.d_in), F16), dA=ar.output((c.d_in, c.r), F32), dB=ar.output((c.r, c.d_out), F32),
                 dbias=ar.output((c.d_out,), F32) if c.bias else None)
        b["ws"] = ar.workspace(lib.sow_workspace_bytes(c.T, c.d_in, c.d_out, c.r, 0, _lib.ACC_NONE, code))
        bufs.append(b)
        p = AC._p
        arr[i] = _lib.LayerArgs(x=p(b["x"]), A=p(b["A"]), B=p(b["B"]), acc_down=None, acc_up=None, bias=p(b["bias"]), y=p(b["y"]),
                                h_save=p(b["h"]), dy=p(b["dy"]), dx=p(b["dx"]), dA=p(b["dA"]), dB=p(b["dB"]), dbias=p(b["dbias"]),
                                T=c.T, d_in=c.d_in, d_out=c.d_out, r_live=c.r, r_acc=0, acc_kind=_lib.ACC_NONE, scale=c.s,
                                grad_beta=0.0, workspace=p(b["ws"]), workspace_bytes=b["ws"].numel())
    assert lib.sow_backward_group_plan(arr, n, code, DEFERRED, None) == 1
    raw = ctypes.create_string_buffer(lib.sow_reduce_desc_bytes() * n)
    blocks = (ctypes.c_int * n)()
    _lib.check(lib.sow_backward_group_reduce_desc(arr, n, code, DEFERRED, raw, blocks), "sow_backward_group_reduce_desc")
    descs = torch.frombuffer(bytearray(raw.raw), dtype=torch.uint8).to(DEV)
    st, total = [], 0
    for k in range(n):
        st.append(total)
        total += blocks[k]
    starts = torch.tensor(st, dtype=torch.int32, device=DEV)

    def step():
        _lib.check(lib.sow_forward_group(arr, n, code, E._stream()), "sow_forward_group")
        _lib.check(lib.sow_backward_group(arr, n, code, DEFERRED, E._stream()), "sow_backward_group")
        _lib.check(lib.sow_reduce_batch(E._ptr(descs), E._ptr(starts), n, total, code, E._stream()), "sow_reduce_batch")

    runs, seq = [], []
    for byte in (0xFF, 0x00):
        ar.fill(byte)
        if runs:
            seq = E._kernel_seq(step)
        else:
            step()
        ar.check_guards(f"fp32-gradient group, run {len(runs)}")
        runs.append([{k: (None if b[k] is None else b[k].clone()) for k in KEYS} for b in bufs])
    for i, c in enumerate(members):
        for k in KEYS:
            if runs[0][i][k] is not None:
                assert torch.equal(AC._bits(runs[0][i][k]), AC._bits(runs[1][i][k])), f"{c.name}: {k} differs on zeroed memory"
    return runs[0], seq


def test_exact_f16_row_owner_group_with_fp32_gradients():
    members = [dataclasses.replace(c, name=f"f16_exact_rows.{c.name}", seed=i) for i, c in enumerate(ROWS_GROUP_1)]
    proved = [_proved(c) for c in members]
    outs, seq = _run_group_param_f32(members, [d for d, _ in proved])
    _expect(seq, ROWS, "f16_exact_rows")
    for c, (d, f), out in zip(members, proved, outs):
        for k in ("dA", "dB", "dbias"):
            if out[k] is not None:
                assert out[k].dtype == F32
                _exact(out[k].cpu(), f[k], F32, f"{c.name}: {k}")
        _exact(out["h"].cpu(), _h_full(c, f), F16, f"{c.name}: h_save")
        _exact(out["y"].cpu(), f["y"], F16, f"{c.name}: y")
        _exact(out["dx"].cpu(), f["dx"], F16, f"{c.name}: dx")


# ------------------------------------------------------------------------------------------------------- non-finite values
def _check_poisoned(c, f, out, clean, name):
    """The non-finite set of every output equals the float64 reference's; everything else is bit-identical to the clean
    run."""
    for k in KEYS:
        if out.get(k) is None:
            continue
        ref = _h_full(c, f) if k == "h" else f[k]
        o, cl = out[k].cpu(), clean[k].cpu()
        bad_ref, bad = ~torch.isfinite(ref), ~torch.isfinite(o.float())
        assert torch.equal(bad, bad_ref), (f"{name}: {k}: {int(bad.sum())} non-finite elements, the float64 reference has "
                                           f"{int(bad_ref.sum())}")
        same = E._bits(o)[~bad] == E._bits(cl)[~bad]
        assert bool(same.all()), f"{name}: {k}: {int((~same).sum())} finite elements differ from the clean run"


def _layer_of(c):
    """The fuzz_plan.Layer of a test_gpu_elementwise.Case (value_plan.layer_refs reads shapes and settings from it)."""
    return FP.Layer(c.name, "f16", c.T, c.d_in, c.d_out, c.r, bias=c.bias, s=c.s, grad_beta=c.grad_beta)


def test_nan_in_the_last_token_of_dy_wide_kernel():
    c = LAYERS[0][0]
    d = {k: (None if v is None else to64(v)) for k, v in _data(c).items()}
    clean = E._run_single(c, d)
    dp = V.poison(d, "dy", [(c.T - 1, c.d_out - 1)], float("nan"))
    trace = {}
    out = E._run_single(c, dp, trace)
    _expect(trace["bwd"], WIDE, c.name)
    f = V.layer_refs(_layer_of(c), dp)
    assert not torch.isfinite(f["dB"]).all() and torch.isfinite(f["dB"]).any()
    _check_poisoned(c, f, out, clean, f"{c.name} NaN in dY[T - 1]")


def test_nan_in_the_last_token_of_dy_row_owner_group_member():
    gp, layers = _group("f16_rows_cgw1", ROWS_GROUP_1, deferred=True, rows=True)
    data = [{k: (None if v is None else to64(v)) for k, v in d.items()} for d in _group_data(gp.name, layers)]
    clean, _ = Z.run_group(gp, layers, data)
    pd = list(data)
    victim = 2
    cv = layers[victim]
    pd[victim] = V.poison(data[victim], "dy", [(cv.T - 1, cv.d_out - 1)], float("nan"))
    outs, seq = Z.run_group(gp, layers, pd)
    _expect(seq, ROWS, gp.name)
    for i, (c, dp, out, cl) in enumerate(zip(layers, pd, outs, clean)):
        f = V.layer_refs(_layer_of(c), dp)
        assert bool(torch.isfinite(f["dA"]).all()) == (i != victim)
        _check_poisoned(c, f, out, cl, f"{c.name} NaN in dY[T - 1] of member {victim}")


# ----------------------------------------------------------------------------------------------------------- module surface
class _Stack(nn.Module):
    """One decoder-block-like container of four SoWLinear layers on one input (FactorBucket groups them by block)."""

    def __init__(self, dtype):
        super().__init__()
        from sow_amd import SoWLinear
        torch.manual_seed(11)
        self.proj = nn.ModuleList([SoWLinear(256, 256, bias=False, rank=16, init_method="normal", device=DEV) for _ in range(4)])
        self.to(dtype)

    def forward(self, x):
        return [p(x) for p in self.proj]


def _factor_gradient_bounds(x, dy, A, B, s, gdt, cdt):
    """float64 references and bounds of one layer's factor gradients.  dA = x^T dh and dB = h^T dY are fp32 sums over T of
    products with a hidden intermediate rounded to the compute dtype (dh = rn(s dY B^T), h = rn(s x A)): one output ulp of
    the gradient dtype, the accumulated rounding of the hidden intermediate, the fp32 noise of a T-term sum and, in f16, the
    subnormal floor of the hidden rounding (test_gpu_elementwise._check's dA bound, applied to both)."""
    x, dy, A, B = to64(x), to64(dy), to64(A), to64(B)
    T = x.shape[0]
    h, dh = s * (x @ A), s * (dy @ B.t())
    u = UNIT_ROUNDOFF[cdt]
    dA_sq, dB_sq = (x * x).t() @ (dh * dh), (h * h).t() @ (dy * dy)
    sub_a = E._sub_term((x * x).sum(0)[:, None].expand(-1, A.shape[1]), cdt)
    sub_b = E._sub_term((dy * dy).sum(0)[None, :].expand(B.shape[0], -1), cdt)
    dA_ref, dB_ref = x.t() @ dh, h.t() @ dy
    return ((dA_ref, bound(dA_ref, gdt, accumulation_term(dA_sq, u), fp32_floor(dA_sq, T), sub_a)),
            (dB_ref, bound(dB_ref, gdt, accumulation_term(dB_sq, u), fp32_floor(dB_sq, T), sub_b)))


@pytest.mark.parametrize("autocast", [False, True], ids=["f16_model", "autocast_fp32_factors"])
def test_factor_bucket_block_reaches_the_f16_row_owner_kernel(autocast):
    from sow_amd.dp import FactorBucket, factor_parameters
    T = 32769
    net = _Stack(F32 if autocast else F16)
    bucket = FactorBucket(factor_parameters(net))
    assert bucket.attach(net) == 4
    gdt = F32 if autocast else F16
    assert bucket.flat_grad.dtype == gdt
    g = torch.Generator().manual_seed(12)
    x = torch.randn(T, 256, generator=g).to(F16).to(DEV).requires_grad_()
    dys = [(torch.randn(T, 256, generator=g) * 0.25).to(F16).to(DEV) for _ in range(4)]

    def step():
        bucket.zero_grad()
        x.grad = None
        with torch.autocast("cuda", dtype=F16, enabled=autocast):
            ys = net(x)
        torch.autograd.backward(ys, dys)
        bucket.finalize()

    step()
    seq = E._kernel_seq(step)
    _expect(seq, ROWS, "FactorBucket block")
    assert len(_f16_form(seq, ROWS)) == 1
    for p, dy in zip(net.proj, dys):
        pA, pB = p.downscale_weights[0], p.upscale_weights[0]
        assert pA.grad.dtype == gdt and pB.grad.dtype == gdt
        # autocast rounds the fp32 factors to f16 for the kernels: the references use what the kernels multiplied
        A, B = pA.detach().to(F16).cpu(), pB.detach().to(F16).cpu()
        (dA_ref, dA_bnd), (dB_ref, dB_bnd) = _factor_gradient_bounds(x.detach().cpu(), dy.cpu(), A, B, float(p.scale), gdt, F16)
        check_bound(pA.grad.cpu(), dA_ref, dA_bnd, name="FactorBucket dA")
        check_bound(pB.grad.cpu(), dB_ref, dB_bnd, name="FactorBucket dB")
