"""-m gpu: bf16 / f16 layers of rank 64 < r <= 256 whose d_in or d_out is not a multiple of 8 (llama_1b's 5461-wide MLP at
rank 200) on the ragged variants of
the fused chain (chain_wide.hip) and the token-slab weight-gradient kernel (skinny_tn_wide.hip), checked element by element
against float64 with the harnesses of tests/test_gpu_elementwise.py (bf16: NaN-neighboured inputs, sentinel guards,
poisoned / zeroed / repeated runs bit-identical) and tests/test_gpu_f16.py (f16); then h_save = NULL, the kernels that run,
the NO_RAGGED switch, grouped calls with deferred reductions, autocast and the module surface with a FactorBucket."""
import pytest
import torch

import test_gpu_elementwise as E
import test_gpu_f16 as F
from conftest import rel_err
from oracle import sow_oracle as O
from sow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16

Case = E.Case
# Widths cover every row residue 1 .. 7 (mod 8) in both directions: 5461 = 5, 2049 = 1, 258 = 2, 259 = 3, 100 = 4, 262 = 6,
# 263 = 7, 1001 = 1.  y of a layer without accumulator rounds once (computed from the rounded h it also saves); an
# accumulator's term is rounded before the live term is added with beta = 1 (many tiles at T = 32769).  Ranks <= 64 are
# not admitted (the generic kernels are faster there): their cases pin the generic path at these widths.
BF16_CASES = [
    Case("rag_2048x5461_r200_T4097", BF16, 4097, 2048, 5461, 200, s=0.5),
    Case("rag_5461x2048_r50_T4097", BF16, 4097, 5461, 2048, 50),
    Case("rag_2049x264_r2_T1", BF16, 1, 2049, 264, 2, s=0.5),
    Case("rag_264x2049_r8_T63_nobias", BF16, 63, 264, 2049, 8, bias=False),
    Case("rag_258x100_r62_T64", BF16, 64, 258, 100, 62, s=0.75),
    Case("rag_100x259_r64_T65", BF16, 65, 100, 259, 64),
    Case("rag_262x263_r66_T4097_grad_beta", BF16, 4097, 262, 263, 66, grad_beta=1.0),
    Case("rag_263x262_r128_T32769", BF16, 32769, 263, 262, 128, s=0.5),
    Case("rag_2049x520_r256_T4097_nobias", BF16, 4097, 2049, 520, 256, bias=False),
    Case("rag_257x2048_r50_T32769_grad_beta", BF16, 32769, 257, 2048, 50, s=0.5, grad_beta=1.0),
    Case("rag_264x1001_r66_lowrank32", BF16, 4097, 264, 1001, 66, acc="lowrank", r_acc=32, y_rounds="twice"),
    Case("rag_1001x264_r200_lowrank200_T32769", BF16, 32769, 1001, 264, 200, acc="lowrank", r_acc=200, s=0.5,
         y_rounds="twice"),
    # the generic kernels on the same inputs, within the same bounds
    Case("rag_2048x5461_r200_no_ragged", BF16, 4097, 2048, 5461, 200, s=0.5, switches=dict(NO_RAGGED=1)),
    Case("rag_5461x2048_r50_no_ragged", BF16, 4097, 5461, 2048, 50, switches=dict(NO_RAGGED=1)),
    Case("rag_264x1001_r66_lowrank32_no_ragged", BF16, 4097, 264, 1001, 66, acc="lowrank", r_acc=32, y_rounds="twice",
         switches=dict(NO_RAGGED=1)),
    # not admitted: odd r, misaligned views, dense accumulator (generic kernels)
    Case("rag_263x262_r51_generic", BF16, 4097, 263, 262, 51),
    Case("rag_2049x264_r50_misaligned", BF16, 4097, 2049, 264, 50, misalign=1),
    Case("rag_2049x264_r50_dense", BF16, 4097, 2049, 264, 50, acc="dense", y_rounds="twice"),
]


@pytest.mark.parametrize("c", BF16_CASES, ids=lambda c: c.name)
def test_ragged_layer_bf16(c):
    d = E._inputs(c)
    out = E._run_single(c, d)
    E._check(c, d, out)


F16_CASES = [
    # (T, d_in, d_out, r, acc, r_acc, bias)
    (4097, 2048, 5461, 200, "none", 0, True),
    (4097, 5461, 2048, 50, "none", 0, True),
    (63, 259, 262, 8, "none", 0, False),
    (1, 100, 263, 256, "none", 0, True),
    (4097, 263, 1001, 96, "lowrank", 200, True),
    (4097, 1001, 263, 128, "lowrank", 32, False),
]


@pytest.mark.parametrize("generic", [False, True], ids=["ragged", "no_ragged"])
@pytest.mark.parametrize("case", F16_CASES, ids=lambda v: f"T{v[0]}_{v[1]}x{v[2]}_r{v[3]}_{v[4]}{v[5] or ''}")
def test_ragged_layer_f16(case, generic, switches):
    T, d_in, d_out, r, acc, r_acc, bias = case
    if generic:
        switches("NO_RAGGED", 1)
    data, out = F._run_layer(T, d_in, d_out, r, acc, r_acc, bias, scale=0.75)
    F._check_layer(data, out, r, acc, 0.75, bwd=True, y_once=(acc == "none"))
    _, again = F._run_layer(T, d_in, d_out, r, acc, r_acc, bias, scale=0.75)
    for k in ("y", "h", "dx", "dA", "dB", "db"):
        if out[k] is not None:
            assert torch.equal(out[k].view(torch.int16), again[k].view(torch.int16)), f"{k} differs on a repeat"


@pytest.fixture
def switches():
    lib = _lib.load()
    saved = {}

    def set_(name, v):
        saved.setdefault(name, lib.sow_get_switch(name.encode()))
        assert lib.sow_set_switch(name.encode(), v) == 0

    yield set_
    for name, v in saved.items():
        lib.sow_set_switch(name.encode(), v)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("r", [50, 200])
def test_forward_without_h_save_is_bit_identical(dtype, r):
    """sow_forward(h_save = NULL) with exactly sow_forward_workspace_bytes of workspace succeeds and gives the y of the call
    that saves h."""
    lib = _lib.load()
    T, d_in, d_out = 4100, 2048, 5461
    g = torch.Generator().manual_seed(7)
    x = torch.randn(T, d_in, generator=g).to(dtype).to(DEV)
    A = (torch.randn(d_in, r, generator=g) * 0.03).to(dtype).to(DEV)
    B = (torch.randn(r, d_out, generator=g) * 0.07).to(dtype).to(DEV)
    bias = torch.randn(d_out, generator=g).to(dtype).to(DEV)
    dt = _lib.BF16 if dtype == BF16 else _lib.F16
    nws = lib.sow_forward_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_NONE, dt)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    ys = []
    for save in (True, False):
        y = torch.empty(T, d_out, dtype=dtype, device=DEV)
        h = torch.empty(lib.sow_h_save_elems(T, r), dtype=dtype, device=DEV) if save else None
        rc = lib.sow_forward(x.data_ptr(), A.data_ptr(), B.data_ptr(), None, None, bias.data_ptr(), y.data_ptr(),
                             None if h is None else h.data_ptr(), T, d_in, d_out, r, 0, _lib.ACC_NONE, 0.5, dt, ws.data_ptr(),
                             nws, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.sow_error_string(rc)
        ys.append(y)
    torch.cuda.synchronize()
    assert torch.equal(ys[0].view(torch.int16), ys[1].view(torch.int16))


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


@pytest.mark.parametrize("d_in,d_out,r", [(2048, 5461, 200), (5461, 2048, 200)])
def test_ragged_layers_run_only_the_fused_kernels(d_in, d_out, r):
    """fwd + bwd of a 5461-wide SoWLinear: the trace holds the ragged chain and weight-gradient kernels and none of the
    generic ones (chain_kernel, tn_partial_kernel, colsum_kernel, the generic GEMM)."""
    from sow_amd import SoWLinear
    torch.manual_seed(3)
    layer = SoWLinear(d_in, d_out, bias=True, rank=r, scale=0.5, init_method="normal", device=DEV, dtype=BF16)
    x = torch.randn(4096, d_in, device=DEV, dtype=BF16, requires_grad=True)
    dy = torch.randn(4096, d_out, device=DEV, dtype=BF16)
    layer(x).backward(dy)            # warm-up: workspaces allocated, library loaded

    def step():
        layer(x).backward(dy)

    names = _kernel_names(step)
    assert names, "the profiler recorded no GPU kernels"
    assert any(_is(n, "chain_wide_kernel") for n in names), sorted(names)
    assert any(_is(n, "tnw_partial_kernel") for n in names), sorted(names)
    bad = sorted(n for n in names if any(_is(n, k) for k in GENERIC_KERNELS))
    assert not bad, bad
    with _lib.switch(NO_RAGGED=1):
        names = _kernel_names(step)
    assert not any(_is(n, "chain_wide_kernel") for n in names), sorted(names)


def test_grouped_calls_with_deferred_reduction_equal_single_calls():
    """Ragged layers (r = 200 and r = 96) grouped with an aligned r = 50 layer: sow_forward_group,
    sow_backward_group(DATA | PARTIAL | GROUP_SLABS), then the deferred reduction of the whole group (the ragged layers'
    descriptors are empty) -- outputs and gradients equal the per-layer calls bit for bit."""
    from sow_amd import ops
    torch.manual_seed(11)
    T = 8193
    dims = [(1024, 1001, 200, 0.5), (1024, 512, 50, 1.0), (1001, 1024, 96, 0.75)]
    layers = []
    for d_in, d_out, r, s in dims:
        x = torch.randn(T, d_in, device=DEV, dtype=BF16)
        A = (torch.randn(d_in, r, device=DEV) * 0.03).to(BF16)
        B = (torch.randn(r, d_out, device=DEV) * 0.07).to(BF16)
        dy = torch.randn(T, d_out, device=DEV, dtype=BF16)
        layers.append((x, A, B, dy, s))
    ref = []
    for x, A, B, dy, s in layers:
        y, h = ops.sow_forward(x, A, B, None, None, None, s)
        dx, dA, dB, _ = ops.sow_backward(dy, x, h, A, B, None, None, s, False)
        ref.append((y, dx, dA, dB))
    calls = []
    for x, A, B, dy, s in layers:
        r, d_out = B.shape
        dA = torch.empty(x.shape[1], r, device=DEV, dtype=BF16)
        dB = torch.empty(r, d_out, device=DEV, dtype=BF16)
        dx = torch.empty_like(x)
        calls.append(ops.LayerCall(x, A, B, scale=s, dy2=dy, dx=dx, out=(dA, dB, None)))
    grp = ops.LayerGroup(calls)
    grp.forward()
    phases = _lib.BWD_DATA | _lib.BWD_WEIGHTS_PARTIAL | _lib.BWD_GROUP_SLABS
    grp.backward(phases)
    red = ops.DeferredReduce()
    red.add_group(grp, phases)
    assert red._blocks[0] == 0 and red._blocks[1] > 0 and red._blocks[2] == 0
    red.run()
    torch.cuda.synchronize()
    for c, (y, dx, dA, dB) in zip(calls, ref):
        dA_g, dB_g, _ = c._keep[7], c._keep[8], c._keep[9]
        assert torch.equal(c.y, y) and torch.equal(c.dx, dx)
        assert torch.equal(dA_g, dA) and torch.equal(dB_g, dB)


@pytest.mark.parametrize("cdt", [BF16, F16])
def test_autocast_ragged_layer(cdt):
    """fp32 SoWLinear(2048, 5461, rank = 200) under torch.autocast gives the bits of the plain layer on factors rounded to
    the compute dtype (y, dx; fp32 gradients rounded), and agrees with the oracle on the rounded operands."""
    import copy
    from sow_amd import SoWLinear
    torch.manual_seed(6)
    layer = SoWLinear(2048, 5461, bias=True, rank=200, scale=0.75, init_method="normal", device=DEV, dtype=torch.float32)
    torch.nn.init.normal_(layer.upscale_weights[0], std=0.05)
    torch.nn.init.normal_(layer.bias, std=0.1)
    twin = copy.deepcopy(layer).to(cdt)
    x = torch.randn(2, 1000, 2048, device=DEV, dtype=torch.float32, requires_grad=True)
    dy = torch.randn(2, 1000, 5461, device=DEV, dtype=cdt)
    with torch.autocast("cuda", dtype=cdt):
        y = layer(x)
    assert y.dtype == cdt
    y.backward(dy)
    xt = x.detach().to(cdt).requires_grad_()
    yt = twin(xt)
    yt.backward(dy)
    bits = lambda t: t.view(torch.int16)
    assert torch.equal(bits(y), bits(yt))
    assert torch.equal(bits(x.grad.to(cdt)), bits(xt.grad))
    A, B = layer.downscale_weights[0], layer.upscale_weights[0]
    for p, q in ((A, twin.downscale_weights[0]), (B, twin.upscale_weights[0]), (layer.bias, twin.bias)):
        assert p.grad.dtype == torch.float32
        assert torch.equal(bits(p.grad.to(cdt)), bits(q.grad))
    r64 = lambda t: t.detach().to(cdt).double().cpu()
    x2, dy2 = r64(x).reshape(-1, 2048), r64(dy).reshape(-1, 5461)
    y_ref = O.sow_forward(x2, [r64(A)], [r64(B)], None, None, 0.75, r64(layer.bias))
    dx_ref, dA_ref, dB_ref, db_ref = O.sow_backward(dy2, x2, [r64(A)], [r64(B)], None, None, 0.75, True)
    assert rel_err(y.detach().cpu().reshape(-1, 5461), y_ref) < 1e-2
    assert rel_err(x.grad.cpu().reshape(-1, 2048), dx_ref) < 1e-2
    assert rel_err(A.grad.cpu(), dA_ref[0]) < 1e-2 and rel_err(B.grad.cpu(), dB_ref[0]) < 1e-2
    assert rel_err(layer.bias.grad.cpu(), db_ref) < 1e-5


class _Llama1bBlock(torch.nn.Module):
    """The seven projections of a llama_1b decoder block (hidden 2048, intermediate 5461), without attention."""

    def __init__(self):
        super().__init__()
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
            setattr(self, n, torch.nn.Linear(2048, 2048, bias=False))
        self.gate_proj = torch.nn.Linear(2048, 5461, bias=False)
        self.up_proj = torch.nn.Linear(2048, 5461, bias=False)
        self.down_proj = torch.nn.Linear(5461, 2048, bias=False)

    def forward(self, h):
        a = self.q_proj(h) * 0.1 + self.k_proj(h) * 0.1 + self.v_proj(h) * 0.1
        h = h + self.o_proj(a)
        return h + self.down_proj(torch.nn.functional.silu(self.gate_proj(h)) * self.up_proj(h))


@pytest.mark.parametrize("r", [50, 200])
def test_llama_1b_block_through_the_module_surface(r, monkeypatch):
    """prepare_sow on a llama_1b-shaped block, siblings grouped, FactorBucket attached, T = 4096: every layer (the ragged
    ones included) writes its gradients through the sink; they equal those of the plain model bit for bit, and the
    forward / backward of the ragged layers match the CPU oracle."""
    import copy
    from sow_amd import SoWConfig, dp, group_siblings, prepare_sow
    from sow_amd.dp import FactorBucket, factor_parameters

    torch.manual_seed(9)
    base = _Llama1bBlock().to(DEV, BF16)
    names = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]
    cfg = SoWConfig(target_modules=names, rank=r, init_method="normal", decompose=None, device=DEV)
    ref = prepare_sow(copy.deepcopy(base), cfg)
    for p in factor_parameters(ref):
        if p.dim() == 2 and p.shape[0] == r:
            torch.nn.init.normal_(p, std=0.05)
    net = copy.deepcopy(ref)
    group_siblings(net)
    bucket = FactorBucket(factor_parameters(net))
    assert bucket.attach(net) == 7
    calls = []
    orig = dp._GradSink.queue
    monkeypatch.setattr(dp._GradSink, "queue", lambda self, *a: (calls.append(1), orig(self, *a))[1])
    x = torch.randn(2, 2048, 2048, device=DEV, dtype=BF16)
    y_ref = ref(x)
    y_ref.float().square().mean().backward()
    bucket.zero_grad()
    y = net(x)
    y.float().square().mean().backward()
    bucket.finalize()
    torch.cuda.synchronize()
    assert len(calls) == 7
    assert torch.equal(y, y_ref)
    # the sink path reduces the weight gradients of the block's aligned layers in the order of its own grouped kernels
    # (include/sow_amd.h: sow_backward_group): equal to the plain model's within fp32 rounding of the slab sums
    diff = []
    names = {id(p): n for n, p in ref.named_parameters()}
    for a, b in zip(factor_parameters(ref), factor_parameters(net)):
        name = names[id(a)]
        e = rel_err(b.grad.float(), a.grad.float())
        print(f"{name}: rel err {e:.3g}{'' if torch.equal(a.grad, b.grad) else ' (not bit-equal)'}")
        diff.append(e)
    assert max(diff) < 1e-2
    # one ragged layer of each direction against the oracle, on its own input (the model without the bucket)
    f = lambda t: t.detach().float().cpu()
    for name, d_in, d_out in (("up_proj", 2048, 5461), ("down_proj", 5461, 2048)):
        m = getattr(ref, name)
        m.zero_grad(set_to_none=True)
        xi = torch.randn(4096, d_in, device=DEV, dtype=BF16, requires_grad=True)
        dyi = torch.randn(4096, d_out, device=DEV, dtype=BF16)
        yi = m(xi)
        yi.backward(dyi)
        A, B = f(m.downscale_weights[0]), f(m.upscale_weights[0])
        yr = O.sow_forward(f(xi), [A], [B], None, None, m.scale, None)
        dxr, dAr, dBr, _ = O.sow_backward(f(dyi), f(xi), [A], [B], None, None, m.scale, False)
        tol = 2e-2
        assert rel_err(f(yi), yr) < tol
        assert rel_err(f(xi.grad), dxr) < tol
        assert rel_err(f(m.downscale_weights[0].grad), dAr[0]) < tol
        assert rel_err(f(m.upscale_weights[0].grad), dBr[0]) < tol
