"""-m gpu: wide-rank layers (64 < r <= 256) on the fused chain (chain_wide.hip) and the token-slab weight-gradient kernel
(skinny_tn_wide.hip), checked element by element against float64 with the harnesses of tests/test_gpu_elementwise.py (bf16:
NaN-neighboured inputs, sentinel guards, poisoned / zeroed / repeated runs bit-identical) and tests/test_gpu_f16.py (f16);
then h_save = NULL, the NO_WIDE_CHAIN switch, grouped calls with deferred reductions and the module surface."""
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
# admitted: bf16 / f16, even r in (64, 256], widths % 8, 16-byte views.  y of a layer without accumulator rounds once (the
# kernel computes it from the rounded h it also saves); an accumulator's term is rounded before the live term is added.
BF16_CASES = [
    Case("wide_r66_T4097", BF16, 4097, 520, 264, 66, s=0.5),
    Case("wide_r128_T1", BF16, 1, 264, 520, 128),
    Case("wide_r200_T32769_2048", BF16, 32769, 2048, 2048, 200, s=0.5),
    Case("wide_r256_T63_nobias", BF16, 63, 264, 264, 256, bias=False),
    Case("wide_r200_grad_beta", BF16, 4097, 520, 520, 200, grad_beta=1.0),
    Case("wide_r128_dense", BF16, 4097, 520, 264, 128, acc="dense", s=0.5, y_rounds="twice"),
    Case("wide_r66_lowrank96", BF16, 4097, 520, 264, 66, acc="lowrank", r_acc=96, y_rounds="twice"),
    Case("wide_r200_lowrank200", BF16, 4097, 264, 520, 200, acc="lowrank", r_acc=200, s=0.5, y_rounds="twice"),
    Case("r50_lowrank200", BF16, 4097, 264, 520, 50, acc="lowrank", r_acc=200, y_rounds="twice"),
    # the generic composition on the same inputs, within the same bounds
    Case("wide_r200_no_wide_chain", BF16, 4097, 520, 264, 200, switches=dict(NO_WIDE_CHAIN=1)),
    Case("wide_r96_lowrank200_no_wide_chain", BF16, 4097, 264, 520, 96, acc="lowrank", r_acc=200, y_rounds="twice",
         switches=dict(NO_WIDE_CHAIN=1)),
    # not admitted: odd r, misaligned views (generic composition)
    Case("wide_r97_generic", BF16, 4097, 264, 264, 97, s=0.5),
    Case("wide_r200_misaligned", BF16, 4097, 264, 264, 200, misalign=1),
]


@pytest.mark.parametrize("c", BF16_CASES, ids=lambda c: c.name)
def test_wide_layer_bf16(c):
    d = E._inputs(c)
    out = E._run_single(c, d)
    E._check(c, d, out)


F16_CASES = [
    # (T, d_in, d_out, r, acc, r_acc, bias)
    (4097, 520, 264, 66, "none", 0, True),
    (63, 264, 520, 256, "none", 0, False),
    (1, 264, 264, 128, "none", 0, True),
    (32769, 2048, 2048, 200, "none", 0, True),
    (4097, 520, 264, 128, "dense", 0, True),
    (4097, 264, 520, 200, "lowrank", 200, True),
    (4097, 520, 264, 66, "lowrank", 96, False),
]


# the generic composition (NO_WIDE_CHAIN) on every case but the K = T = 32769 one: its transposed-GEMM dB sums 32769 terms in
# one fp32 chain and misses the harness's 0.5 % bit-equal share by a few elements
F16_RUNS = [(c, False) for c in F16_CASES] + [(c, True) for c in F16_CASES if c[0] < 32768]


@pytest.mark.parametrize("case,generic", F16_RUNS,
                         ids=lambda v: (f"T{v[0]}_{v[1]}x{v[2]}_r{v[3]}_{v[4]}{v[5] or ''}" if isinstance(v, tuple)
                                        else ("no_wide_chain" if v else "wide")))
def test_wide_layer_f16(case, generic, switches):
    T, d_in, d_out, r, acc, r_acc, bias = case
    if generic:
        switches("NO_WIDE_CHAIN", 1)
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
@pytest.mark.parametrize("generic", [False, True], ids=["wide", "no_wide_chain"])
def test_forward_without_h_save_is_bit_identical(dtype, generic, switches):
    """r = 200: sow_forward(h_save = NULL) succeeds and gives the y of the call that saves h."""
    if generic:
        switches("NO_WIDE_CHAIN", 1)
    lib = _lib.load()
    T, d_in, d_out, r = 4100, 1024, 1032, 200
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
        h = torch.empty(T * r, dtype=dtype, device=DEV) if save else None
        rc = lib.sow_forward(x.data_ptr(), A.data_ptr(), B.data_ptr(), None, None, bias.data_ptr(), y.data_ptr(),
                             None if h is None else h.data_ptr(), T, d_in, d_out, r, 0, _lib.ACC_NONE, 0.5, dt, ws.data_ptr(),
                             nws, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.sow_error_string(rc)
        ys.append(y)
    torch.cuda.synchronize()
    assert torch.equal(ys[0].view(torch.int16), ys[1].view(torch.int16))


def test_grouped_calls_with_deferred_reduction_equal_single_calls():
    """A wide layer (r = 200) grouped with two r = 50 layers: sow_forward_group, sow_backward_group(DATA | PARTIAL |
    GROUP_SLABS), then the deferred reduction of the whole group (the wide layer's descriptor is empty) -- outputs and
    gradients equal the per-layer calls bit for bit."""
    from sow_amd import ops
    torch.manual_seed(11)
    T = 8193
    dims = [(1024, 1024, 200, 0.5), (1024, 512, 50, 1.0), (1024, 1032, 50, 0.75)]
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
    assert red._blocks[0] == 0 and red._blocks[1] > 0
    red.run()
    torch.cuda.synchronize()
    for c, (y, dx, dA, dB) in zip(calls, ref):
        dA_g, dB_g, _ = c._keep[7], c._keep[8], c._keep[9]
        assert torch.equal(c.y, y) and torch.equal(c.dx, dx)
        assert torch.equal(dA_g, dA) and torch.equal(dB_g, dB)


def test_sowlinear_rank200_against_oracle():
    """SoWLinear(2048, 2048, rank = 200) in bf16, forward and backward, at the bf16 tolerance of test_gpu_parity.py; the
    no-grad forward gives the training forward's y bit for bit."""
    from sow_amd import SoWLinear
    torch.manual_seed(5)
    layer = SoWLinear(2048, 2048, bias=True, rank=200, scale=0.75, init_method="normal", device=DEV, dtype=BF16)
    torch.nn.init.normal_(layer.upscale_weights[0], std=0.05)
    torch.nn.init.normal_(layer.bias, std=0.1)
    x = torch.randn(4, 1000, 2048, device=DEV, dtype=BF16, requires_grad=True)
    dy = torch.randn(4, 1000, 2048, device=DEV, dtype=BF16)
    y = layer(x)
    y.backward(dy)
    with torch.no_grad():
        y_ng = layer(x)
    assert torch.equal(y_ng, y.detach())
    f = lambda t: t.detach().float().cpu()
    A, B = f(layer.downscale_weights[0]), f(layer.upscale_weights[0])
    x2, dy2 = f(x).reshape(-1, 2048), f(dy).reshape(-1, 2048)
    y_ref = O.sow_forward(x2, [A], [B], None, None, 0.75, f(layer.bias))
    dx_ref, dA_ref, dB_ref, db_ref = O.sow_backward(dy2, x2, [A], [B], None, None, 0.75, True)
    tol = 2e-2
    assert rel_err(f(y).reshape(-1, 2048), y_ref) < tol
    assert rel_err(f(x.grad).reshape(-1, 2048), dx_ref) < tol
    assert rel_err(f(layer.downscale_weights[0].grad), dA_ref[0]) < tol
    assert rel_err(f(layer.upscale_weights[0].grad), dB_ref[0]) < tol
    assert rel_err(f(layer.bias.grad), db_ref) < tol


def test_bucket_attached_wide_layers_take_the_sink_path(monkeypatch):
    """prepare_sow(rank = 200) on a small MLP, siblings grouped, FactorBucket.attach(): the wide layers write their
    gradients through the sink (grouped PARTIAL, empty deferred reductions) and the factor gradients equal those of the
    plain model bit for bit."""
    import copy
    from sow_amd import SoWConfig, dp, group_siblings, prepare_sow
    from sow_amd.dp import FactorBucket, factor_parameters

    class Block(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.gate_proj = torch.nn.Linear(512, 1024, bias=False)
            self.up_proj = torch.nn.Linear(512, 1024, bias=False)
            self.down_proj = torch.nn.Linear(1024, 512, bias=False)

        def forward(self, h):
            return self.down_proj(torch.nn.functional.silu(self.gate_proj(h)) * self.up_proj(h))

    torch.manual_seed(9)
    base = torch.nn.Sequential(Block(), Block()).to(DEV, BF16)
    cfg = SoWConfig(target_modules=["gate_proj", "up_proj", "down_proj"], rank=200, init_method="normal", decompose=None,
                    device=DEV)
    ref = prepare_sow(copy.deepcopy(base), cfg)
    for p in factor_parameters(ref):
        if p.dim() == 2 and p.shape[0] == 200:
            torch.nn.init.normal_(p, std=0.05)
    net = copy.deepcopy(ref)
    assert group_siblings(net) == 2
    bucket = FactorBucket(factor_parameters(net))
    assert bucket.attach(net) == 6
    calls = []
    orig = dp._GradSink.queue     # every sink pass, single layer (down_proj) or sibling group (gate_proj / up_proj)
    monkeypatch.setattr(dp._GradSink, "queue", lambda self, *a: (calls.append(1), orig(self, *a))[1])
    x = torch.randn(2, 700, 512, device=DEV, dtype=BF16)
    ref(x).float().square().mean().backward()
    bucket.zero_grad()
    net(x).float().square().mean().backward()
    bucket.finalize()
    torch.cuda.synchronize()
    assert len(calls) == 6
    for a, b in zip(factor_parameters(ref), factor_parameters(net)):
        assert torch.equal(a.grad, b.grad)
