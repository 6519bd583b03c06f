"""-m gpu: bf16 / f16 layers of even rank 64 < r <= 256 with a DENSE frozen accumulator whose d_in or d_out is not a
multiple of 8 (llama_1b's 5461-wide MLP at rank 200 after accumulate()): the dense product on gemm_rag.hip, the live term
on the ragged chain_wide (beta = 1) and the weight gradients on skinny_tn_wide.

1. layers, element by element against float64 with the harnesses of tests/test_gpu_elementwise.py (bf16: NaN-neighboured
   inputs, sentinel guards, a 0xFF workspace, poisoned / zeroed / repeated runs bit-identical) and tests/test_gpu_f16.py;
   the same cases under NO_RAGGED_GEMM and NO_RAGGED within the same bounds;
2. the product alone (B = 0, no bias: the state right after accumulate()): y = rn(x W_acc) and dX = rn(dY W_acc^T), each
   rounded once, held with check_rounded(acc = fp32_floor) against float64;
3. exact operands (small integers and half-integers: every fp32 sum exact), bit for bit against RNE(ref64);
4. one NaN / one +Inf in x, dY and W_acc (the element after a row's end, the last element of a row, the interior): the
   non-finite elements of y and dX are those of the float64 reference, every other one equals the clean run bit for bit;
5. the kernels that run (torch profiler), under the default switches, NO_RAGGED_GEMM and NO_RAGGED;
6. grouped calls, SOW_PARAM_F32, HIP-graph capture and the module surface around accumulate()."""
import dataclasses

import pytest
import torch

import test_gpu_elementwise as E
import test_gpu_f16 as F
from conftest import rel_err
from numerics import check_rounded, fp32_floor, rne, to64
from oracle import sow_oracle as O
from sow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16

Case = E.Case


def D(name, T, d_in, d_out, r, **kw):
    kw.setdefault("y_rounds", "twice")      # gemm_rag writes rn(x W_acc), the chain adds the live term with beta = 1
    return Case(name, BF16, T, d_in, d_out, r, acc="dense", **kw)


# every row residue 1 .. 7 (mod 8) on d_in and on d_out: 1001 = 1, 258 = 2, 259 = 3, 100 = 4 (below one tile), 5461 = 261 =
# 5, 262 = 6, 263 = 7; T in {1, 63, 65, 4097, 32769}; with and without bias; grad_beta = 1; h_save = NULL
BASE = [
    D("rd_2048x5461_r200_T4097", 4097, 2048, 5461, 200, s=0.5),
    D("rd_5461x2048_r200_T4097", 4097, 5461, 2048, 200, s=0.5),
    D("rd_1001x264_r66_T65", 65, 1001, 264, 66),
    D("rd_258x264_r128_T63_nobias", 63, 258, 264, 128, bias=False, s=0.75),
    D("rd_259x520_r200_T1", 1, 259, 520, 200),
    D("rd_100x264_r66_T4097", 4097, 100, 264, 66, s=0.5),
    D("rd_261x264_r256_T65_nobias", 65, 261, 264, 256, bias=False),
    D("rd_262x264_r66_T32769", 32769, 262, 264, 66, s=0.5),
    D("rd_263x264_r128_T63", 63, 263, 264, 128),
    D("rd_264x1001_r66_T63_nobias", 63, 264, 1001, 66, bias=False),
    D("rd_264x258_r128_T65", 65, 264, 258, 128, s=0.5),
    D("rd_520x259_r200_T4097_grad_beta", 4097, 520, 259, 200, grad_beta=1.0),
    D("rd_264x100_r66_T1", 1, 264, 100, 66),
    D("rd_264x261_r256_T4097", 4097, 264, 261, 256, s=0.75),
    D("rd_264x262_r66_T65_grad_beta_nobias", 65, 264, 262, 66, bias=False, grad_beta=1.0),
    D("rd_264x263_r128_T32769", 32769, 264, 263, 128),
    D("rd_263x262_r200_T4097", 4097, 263, 262, 200, s=0.5),
    D("rd_100x50_r66_T65", 65, 100, 50, 66),                       # K and N below one tile
    D("rd_2049x264_r66_T4097_noh", 4097, 2049, 264, 66, save_h=False),
    D("rd_264x2049_r200_T65_noh_nobias", 65, 264, 2049, 200, save_h=False, bias=False, s=0.5),
]
SWITCHED = [dataclasses.replace(c, name=f"{c.name}_{tag}", switches=sw)
            for tag, sw in (("no_ragged_gemm", dict(NO_RAGGED_GEMM=1)), ("no_ragged", dict(NO_RAGGED=1))) for c in BASE]


@pytest.mark.parametrize("c", BASE + SWITCHED, ids=lambda c: c.name)
def test_ragged_dense_layer_bf16(c):
    d = E._inputs(c)
    out = E._run_single(c, d)
    E._check(c, d, out)


F16_CASES = [
    # (T, d_in, d_out, r, bias)
    (4097, 2048, 5461, 200, True),
    (4097, 5461, 2048, 200, True),
    (63, 259, 262, 66, False),
    (1, 100, 263, 256, True),
    (65, 1001, 264, 128, True),
    (4097, 264, 1001, 96, False),
]


@pytest.mark.parametrize("sw", [{}, dict(NO_RAGGED_GEMM=1), dict(NO_RAGGED=1)], ids=["default", "no_ragged_gemm", "no_ragged"])
@pytest.mark.parametrize("case", F16_CASES, ids=lambda v: f"T{v[0]}_{v[1]}x{v[2]}_r{v[3]}")
def test_ragged_dense_layer_f16(case, sw):
    T, d_in, d_out, r, bias = case
    with _lib.switch(**sw):
        data, out = F._run_layer(T, d_in, d_out, r, "dense", 0, bias, scale=0.75)
        F._check_layer(data, out, r, "dense", 0.75, bwd=True, y_once=False)
        _, again = F._run_layer(T, d_in, d_out, r, "dense", 0, bias, scale=0.75)
    for k in ("y", "h", "dx", "dA", "dB", "db"):
        if out[k] is not None:
            assert torch.equal(out[k].view(torch.int16), again[k].view(torch.int16)), f"{k} differs on a repeat"


# ---- 2. the product alone ------------------------------------------------------------------------------------------------
def _product_case(dtype, T, d_in, d_out, r=66, **kw):
    return Case(f"prod_{'bf16' if dtype == BF16 else 'f16'}_{d_in}x{d_out}_T{T}", dtype, T, d_in, d_out, r, acc="dense",
                bias=False, y_rounds="twice", **kw)


def _product_inputs(c):
    """B = 0 and no bias: y = rn(x W_acc) and dX = rn(dY W_acc^T) survive the chain's beta = 1 pass unchanged."""
    d = E._inputs(c)
    d["B"] = torch.zeros_like(d["B"])
    if c.dtype == F16:      # keep the sums well inside f16's range
        d["W"] = (d["W"].float() * 0.5).to(F16)
    return d


def _held(out, ref, dt, acc, name):
    """check_rounded(acc = fp32_floor) at the default MAX_INEXACT, for bf16 and f16 alike; the share is printed first."""
    print(f"{name}: {100 * float((to64(out) != rne(ref, dt)).double().mean()):.4f} % not bit-equal to RNE(ref64)")
    st = check_rounded(out, ref, dt, acc=acc, name=name)
    print(f"{name}: worst err / limit {st['worst']:.3f}")


def _check_product(c, d, out):
    x, W, dy = to64(d["x"]), to64(d["W"]), to64(d["dy"])
    _held(out["y"], x @ W, c.dtype, fp32_floor((x * x) @ (W * W), c.d_in), f"{c.name}: y")
    _held(out["dx"], dy @ W.t(), c.dtype, fp32_floor((dy * dy) @ (W * W).t(), c.d_out), f"{c.name}: dx")


PRODUCTS = [
    # the two llama_1b shapes; every residue on either side; K < 64 (d_in = 50 forward, d_out = 50 backward); N < one tile
    _product_case(BF16, 4097, 2048, 5461, 200),
    _product_case(BF16, 4097, 5461, 2048, 200),
    _product_case(BF16, 300, 1001, 264), _product_case(BF16, 300, 264, 1001),
    _product_case(BF16, 129, 258, 264), _product_case(BF16, 129, 264, 258),
    _product_case(BF16, 65, 259, 520), _product_case(BF16, 65, 520, 259),
    _product_case(BF16, 1, 100, 264), _product_case(BF16, 63, 264, 100),
    _product_case(BF16, 200, 261, 264), _product_case(BF16, 200, 264, 261),
    _product_case(BF16, 128, 262, 264), _product_case(BF16, 128, 264, 262),
    _product_case(BF16, 127, 263, 264), _product_case(BF16, 127, 264, 263),
    _product_case(BF16, 300, 50, 263), _product_case(BF16, 300, 263, 50), _product_case(BF16, 65, 21, 70),
    _product_case(F16, 4097, 2048, 5461, 200), _product_case(F16, 4097, 5461, 2048, 200),
    _product_case(F16, 300, 263, 1001), _product_case(F16, 65, 50, 262), _product_case(F16, 65, 262, 50),
]


@pytest.mark.parametrize("c", PRODUCTS, ids=lambda c: c.name)
def test_product_alone_rounds_once(c):
    d = _product_inputs(c)
    out = E._run_single(c, d)
    _check_product(c, d, out)
    again = E._run_single(dataclasses.replace(c, switches=dict(NO_RAGGED_GEMM=1)), d)
    _check_product(dataclasses.replace(c, name=c.name + "_no_ragged_gemm"), d, again)


# ---- 3. exact operands ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("d_in,d_out", [(2048, 5461), (5461, 2048), (263, 100)])
def test_exact_operands_are_bit_exact(d_in, d_out, dtype):
    """x and dY half-integers in [-2, 2], W_acc integers in [-3, 3], all dense: every partial sum is a multiple of 1/2 below
    2^15, exact in fp32 in any order, so y and dX must equal RNE(ref64) bit for bit (|sum| stays far below f16's 65504)."""
    T = 300
    c = Case(f"exact_{d_in}x{d_out}", dtype, T, d_in, d_out, 66, acc="dense", bias=False, y_rounds="twice")
    g = torch.Generator().manual_seed(d_in + 7 * d_out)
    d = E._inputs(c)
    d["x"] = (torch.randint(-4, 5, (T, d_in), generator=g).double() / 2).to(dtype)
    d["dy"] = (torch.randint(-4, 5, (T, d_out), generator=g).double() / 2).to(dtype)
    d["W"] = torch.randint(-3, 4, (d_in, d_out), generator=g).double().to(dtype)
    d["B"] = torch.zeros_like(d["B"])
    out = E._run_single(c, d)
    x, W, dy = to64(d["x"]), to64(d["W"]), to64(d["dy"])
    for name, got, ref in (("y", out["y"], x @ W), ("dx", out["dx"], dy @ W.t())):
        check_rounded(got, ref, dtype, max_ulp=0, max_inexact=0, min_count=0, name=f"{c.name}: {name}")


# ---- 4. non-finite values ------------------------------------------------------------------------------------------------
def _poison_spots(rows, cols):
    m = min(5, rows - 2)
    return {"after_row_end": (m + 1, 0), "row_last": (m, cols - 1), "interior": (rows // 2, cols // 2)}


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("operand", ["x", "dy", "W"])
@pytest.mark.parametrize("d_in,d_out", [(264, 1001), (1001, 264), (263, 261)])
def test_one_non_finite_value(d_in, d_out, operand, value):
    T = 131
    c = Case(f"poison_{d_in}x{d_out}", BF16, T, d_in, d_out, 66, acc="dense", bias=False, y_rounds="twice")
    d = E._inputs(c)
    clean = E._run_single(c, d)
    for where, (i, j) in _poison_spots(*d[operand].shape).items():
        p = dict(d)
        p[operand] = d[operand].clone()
        p[operand][i, j] = value
        out = E._run_single(c, p)
        q = {k: to64(v) for k, v in p.items() if v is not None}
        ref = dict(y=q["x"] @ q["W"] + (c.s * (q["x"] @ q["A"])) @ q["B"],
                   dx=q["dy"] @ q["W"].t() + (c.s * (q["dy"] @ q["B"].t())) @ q["A"].t())
        for k in ("y", "dx"):
            bad_ref, bad = ~torch.isfinite(ref[k]), ~torch.isfinite(out[k].double())
            assert torch.equal(bad, bad_ref), (f"{c.name} {operand}[{where}] = {value}: {k} has {int(bad.sum())} non-finite "
                                               f"elements, the reference {int(bad_ref.sum())}")
            same = out[k].view(torch.int16)[~bad] == clean[k].view(torch.int16)[~bad]
            assert bool(same.all()), f"{c.name} {operand}[{where}] = {value}: finite elements of {k} differ from the clean run"
            # an infinity keeps its sign
            inf_ref = torch.isinf(ref[k])
            assert torch.equal(out[k].double()[inf_ref], ref[k][inf_ref]), f"{c.name} {operand}[{where}]: {k} infinities"


# ---- 5. the kernels that run ---------------------------------------------------------------------------------------------
GENERIC_KERNELS = ("chain_kernel", "tn_partial_kernel", "colsum_kernel", "gemm_kernel")


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}


def _is(name, kernel):
    # demangled ("sow::chain_kernel<...>") or mangled ("_ZN3sow12chain_kernel...") names of exactly this kernel
    return f"sow::{kernel}" in name or f"{len(kernel)}{kernel}" in name


def _has(names, kernel):
    return any(_is(n, kernel) for n in names)


def _dense_layer(d_in, d_out, r, bias=True, dtype=BF16, scale=0.5):
    """SoWLinear in the state of a prepared model after accumulate(): dense W_acc, fresh A, B set to non-zero values."""
    from sow_amd import SoWLinear
    layer = SoWLinear(d_in, d_out, bias=bias, rank=r, scale=scale, init_method="normal", device=DEV, dtype=dtype)
    layer.virtual_rank = min(d_in, d_out)          # what prepare_sow sets: the accumulator stays dense
    layer.accumulate()
    assert layer.acc_downweight.shape == (d_in, d_out) and layer.acc_upweight.numel() == 0
    torch.nn.init.normal_(layer.upscale_weights[0], std=0.05)
    return layer


@pytest.mark.parametrize("d_in,d_out,r", [(2048, 5461, 200), (5461, 2048, 200)])
def test_ragged_dense_layers_run_only_the_fused_kernels(d_in, d_out, r):
    """fwd + bwd of a 5461-wide SoWLinear with a dense accumulator: gemm_rag, the ragged chain and the token-slab
    weight-gradient kernel, none of the generic ones; NO_RAGGED_GEMM swaps the product only; NO_RAGGED everything."""
    torch.manual_seed(3)
    layer = _dense_layer(d_in, d_out, r)
    x = torch.randn(4096, d_in, device=DEV, dtype=BF16, requires_grad=True)
    dy = torch.randn(4096, d_out, device=DEV, dtype=BF16)
    layer(x).backward(dy)            # warm-up: workspaces allocated, library loaded

    def step():
        layer(x).backward(dy)

    names = _kernel_names(step)
    assert names, "the profiler recorded no GPU kernels"
    for k in ("gemm_rag_kernel", "chain_wide_kernel", "tnw_partial_kernel"):
        assert _has(names, k), (k, sorted(names))
    bad = sorted(n for n in names if any(_is(n, k) for k in GENERIC_KERNELS))
    assert not bad, bad
    with _lib.switch(NO_RAGGED_GEMM=1):
        names = _kernel_names(step)
    assert _has(names, "gemm_kernel") and not _has(names, "gemm_rag_kernel") and _has(names, "chain_wide_kernel"), sorted(names)
    with _lib.switch(NO_RAGGED=1):
        names = _kernel_names(step)
    assert not _has(names, "gemm_rag_kernel") and not _has(names, "chain_wide_kernel"), sorted(names)


# ---- 6. surfaces ---------------------------------------------------------------------------------------------------------
def test_grouped_calls_equal_single_calls():
    """A ragged dense layer of each direction grouped with an aligned r = 50 layer and an aligned dense one:
    sow_forward_group / sow_backward_group equal the per-layer calls bit for bit."""
    from sow_amd import ops
    torch.manual_seed(11)
    T = 8193
    dims = [(1024, 1001, 200, 0.5, True), (1024, 512, 50, 1.0, False), (1001, 1024, 96, 0.75, True), (512, 520, 50, 1.0, True)]
    layers = []
    for d_in, d_out, r, s, dense in dims:
        x = torch.randn(T, d_in, device=DEV, dtype=BF16)
        A = (torch.randn(d_in, r, device=DEV) * 0.03).to(BF16)
        B = (torch.randn(r, d_out, device=DEV) * 0.07).to(BF16)
        W = (torch.randn(d_in, d_out, device=DEV) * 0.02).to(BF16) if dense else None
        dy = torch.randn(T, d_out, device=DEV, dtype=BF16)
        layers.append((x, A, B, W, dy, s))
    ref = []
    for x, A, B, W, dy, s in layers:
        y, h = ops.sow_forward(x, A, B, W, None, None, s)
        dx, dA, dB, _ = ops.sow_backward(dy, x, h, A, B, W, None, s, False)
        ref.append((y, dx, dA, dB))
    calls = []
    for x, A, B, W, dy, s in layers:
        r, d_out = B.shape
        dA = torch.empty(x.shape[1], r, device=DEV, dtype=BF16)
        dB = torch.empty(r, d_out, device=DEV, dtype=BF16)
        calls.append(ops.LayerCall(x, A, B, acc_down=W, scale=s, dy2=dy, dx=torch.empty_like(x), out=(dA, dB, None)))
    grp = ops.LayerGroup(calls)
    names = _kernel_names(lambda: (grp.forward(), grp.backward()))
    assert _has(names, "gemm_rag_kernel"), sorted(names)
    torch.cuda.synchronize()
    for c, (y, dx, dA, dB) in zip(calls, ref):
        dA_g, dB_g = c._keep[7], c._keep[8]
        assert torch.equal(c.y, y) and torch.equal(c.dx, dx)
        assert torch.equal(dA_g, dA) and torch.equal(dB_g, dB)


@pytest.mark.parametrize("cdt", [BF16, F16])
@pytest.mark.parametrize("d_in,d_out", [(1024, 1001), (1001, 1024)])
def test_param_f32_equals_the_plain_call_on_rounded_parameters(d_in, d_out, cdt):
    """SOW_PARAM_F32 (fp32 A, B, bias and W_acc, activations of the compute dtype): y and dX carry the bits of the plain call
    on parameters rounded once to the compute dtype; the gradients are fp32 and round to the plain call's."""
    from sow_amd import ops
    torch.manual_seed(5)
    T, r, s = 4097, 200, 0.75
    x = torch.randn(T, d_in, device=DEV).to(cdt)
    dy = torch.randn(T, d_out, device=DEV).to(cdt)
    A, B = torch.randn(d_in, r, device=DEV) * 0.03, torch.randn(r, d_out, device=DEV) * 0.07
    W, bias = torch.randn(d_in, d_out, device=DEV) * 0.02, torch.randn(d_out, device=DEV) * 0.1
    y, h = ops.sow_forward(x, A, B, W, None, bias, s, param_f32=True)
    dx, dA, dB, db = ops.sow_backward(dy, x, h, A, B, W, None, s, True, param_f32=True)
    Ar, Br, Wr, br = (t.to(cdt) for t in (A, B, W, bias))
    y2, h2 = ops.sow_forward(x, Ar, Br, Wr, None, br, s)
    dx2, dA2, dB2, db2 = ops.sow_backward(dy, x, h2, Ar, Br, Wr, None, s, True)
    bits = lambda t: t.view(torch.int16)
    assert y.dtype == cdt and torch.equal(bits(y), bits(y2)) and torch.equal(bits(dx), bits(dx2))
    for g32, g in ((dA, dA2), (dB, dB2), (db, db2)):
        assert g32.dtype == torch.float32
        assert torch.equal(bits(g32.to(cdt)), bits(g))


def test_hip_graph_capture_replays_bit_identically():
    from sow_amd import ops
    torch.manual_seed(8)
    T, d_in, d_out, r, s = 4097, 1001, 1032, 200, 0.5
    x = torch.randn(T, d_in, device=DEV, dtype=BF16)
    dy = torch.randn(T, d_out, device=DEV, dtype=BF16)
    A, B = (torch.randn(d_in, r, device=DEV) * 0.03).to(BF16), (torch.randn(r, d_out, device=DEV) * 0.07).to(BF16)
    W = (torch.randn(d_in, d_out, device=DEV) * 0.02).to(BF16)

    def step():
        y, h = ops.sow_forward(x, A, B, W, None, None, s)
        dx, dA, dB, _ = ops.sow_backward(dy, x, h, A, B, W, None, s, False)
        return y, dx, dA, dB

    eager = [t.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))


class _SmallRagged(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.up = torch.nn.Linear(264, 1001, bias=True)
        self.down = torch.nn.Linear(1001, 264, bias=False)

    def forward(self, h):
        return h + self.down(torch.nn.functional.silu(self.up(h)))


def test_module_story_prepare_step_accumulate_step():
    """prepare_sow (dense accumulators from step 0) -> step -> accumulate(model) -> step on a small ragged model, each step
    against the oracle on the layers' own inputs; the trace after accumulate() holds gemm_rag_kernel."""
    from sow_amd import SoWConfig, SoWLinear, accumulate, prepare_sow
    torch.manual_seed(21)
    base = _SmallRagged().to(DEV, BF16)
    cfg = SoWConfig(target_modules=["up", "down"], rank=66, init_method="normal", device=DEV)
    net = prepare_sow(base, cfg)
    mods = [m for m in net.modules() if isinstance(m, SoWLinear)]
    assert len(mods) == 2
    f = lambda t: t.detach().float().cpu()

    def check_step(tag):
        for m in mods:
            assert m.acc_downweight.shape == (m.in_features, m.out_features), "the accumulator is not dense"
            torch.nn.init.normal_(m.upscale_weights[0], std=0.05)
            m.zero_grad(set_to_none=True)
            xi = torch.randn(4097, m.in_features, device=DEV, dtype=BF16, requires_grad=True)
            dyi = torch.randn(4097, m.out_features, device=DEV, dtype=BF16)
            m(xi).backward(dyi)
            A, B, W = f(m.downscale_weights[0]), f(m.upscale_weights[0]), f(m.acc_downweight)
            bias = None if m.bias is None else f(m.bias)
            yr = O.sow_forward(f(xi), [A], [B], W, None, m.scale, bias)
            dxr, dAr, dBr, _ = O.sow_backward(f(dyi), f(xi), [A], [B], W, None, m.scale, bias is not None)
            tol = 2e-2
            assert rel_err(f(m(xi)), yr) < tol, tag
            assert rel_err(f(xi.grad), dxr) < tol, tag
            assert rel_err(f(m.downscale_weights[0].grad), dAr[0]) < tol, tag
            assert rel_err(f(m.upscale_weights[0].grad), dBr[0]) < tol, tag

    check_step("before accumulate")
    accumulate(net)
    check_step("after accumulate")
    x = torch.randn(4, 1024, 264, device=DEV, dtype=BF16, requires_grad=True)
    net(x).float().square().mean().backward()
    names = _kernel_names(lambda: net(x).float().square().mean().backward())
    assert _has(names, "gemm_rag_kernel") and _has(names, "chain_wide_kernel"), sorted(names)
