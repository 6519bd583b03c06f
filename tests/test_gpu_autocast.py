"""-m gpu: fp32 parameters with bf16 / f16 compute (include/sow_amd.h: SOW_PARAM_F32; SoWLinear under torch.autocast).

1. A flagged call on fp32 factors equals, bit for bit, the plain call on factors pre-rounded with .to(compute dtype): y,
   h_save and dx; the fp32 dA, dB and dbias rounded to the compute dtype equal the plain gradients -- on every path
   (chain2, short T, gemm4h, low-rank accumulators on both sides of r = 64, wide r, the generic fallbacks, T = 0, bias or not),
   with NaN-guarded inputs, sentinel-guarded outputs and outputs / workspaces poisoned with 0xFF, equal to a zeroed run.
2. Accumulating (grad_beta = 1) fp32 gradients against float64, element by element, within the fp32 bound (tests/numerics.py).
3. The module surface: output / gradient dtypes, agreement with the oracle, no-grad forward, refused combinations; sibling
   groups; FactorBucket + FactorAdamW; torch.amp.GradScaler in f16."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import rel_err
from numerics import check_bound, fp32_floor, to64, ulp
from oracle import sow_oracle as O
from sow_amd import SoWLinear, _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
HALF = [BF16, F16]
CODE = {BF16: _lib.BF16, F16: _lib.F16}
GUARD = 64
SENTINEL = -7.25


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


class Arena:
    """Guarded buffers of one call: inputs with NaN neighbours, outputs with sentinel guards (poisonable)."""

    def __init__(self):
        self.outs = []

    def input(self, t, dtype):
        if t is None:
            return None
        buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
        view = buf[GUARD:GUARD + t.numel()].view(t.shape)
        view.copy_(t.to(DEV, dtype))
        return view

    def output(self, shape, dtype, initial=None):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
        view = buf[GUARD:GUARD + n].view(shape)
        self.outs.append((buf, n, view, None if initial is None else initial.to(DEV, dtype)))
        return view

    def workspace(self, nbytes):
        if not nbytes:
            return None
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=DEV)
        self.outs.append((ws, ws.numel(), ws, None))
        return ws

    def fill(self, byte):
        for buf, n, view, init in self.outs:
            if init is not None:
                view.copy_(init)
            elif buf.dtype == torch.uint8:
                buf.fill_(byte)
            else:
                _bits(view).fill_(-1 if byte == 0xFF else 0)

    def check_guards(self, what):
        torch.cuda.synchronize()
        for buf, n, view, _ in self.outs:
            if buf.dtype == torch.uint8:
                continue
            for name, g in (("leading", buf[:GUARD]), ("trailing", buf[GUARD + n:])):
                assert bool((g == SENTINEL).all()), f"{what}: {name} guard of an output overwritten"


def _p(t):
    return None if t is None else t.data_ptr()


def _inputs(T, d_in, d_out, r, acc, r_acc, bias, seed=0):
    g = torch.Generator().manual_seed(4000 + seed + T + r + r_acc)

    def rnd(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std

    d = dict(x=rnd(T, d_in), A=rnd(d_in, r, std=0.05), B=rnd(r, d_out, std=0.05), bias=rnd(d_out, std=0.1) if bias else None,
             dy=rnd(T, d_out), acc_down=None, acc_up=None)
    if acc == "dense":
        d["acc_down"] = rnd(d_in, d_out, std=0.02)
    elif acc == "lowrank":
        d["acc_down"], d["acc_up"] = rnd(d_in, r_acc, std=0.05), rnd(r_acc, d_out, std=0.05)
    d["dA0"], d["dB0"] = rnd(d_in, r, std=0.5), rnd(r, d_out, std=0.5)
    d["dbias0"] = rnd(d_out, std=0.5) if bias else None
    return d


def _run(d, cdt, T, d_in, d_out, r, acc, r_acc, s, flagged, grad_beta=0.0, fills=(0xFF, 0x00), want_dh=False):
    """sow_forward + sow_backward_ex through the C ABI.  flagged: fp32 parameters and gradients with SOW_PARAM_F32; else the
    plain call on the parameters rounded to cdt.  One run per entry of `fills` (outputs and workspaces poisoned with that
    byte); asserts the runs are bit-identical and the guards intact; returns the outputs of the first.  want_dh: also the
    internal dh = rn(s dY B^T) the weight gradients were summed from -- the first region of the backward workspace (api.hip
    plan_ws: off_dh = 0), [T, 64] for r <= 64 and [T, r] beyond, like h_save."""
    lib = _lib.load()
    kind = {None: _lib.ACC_NONE, "dense": _lib.ACC_DENSE, "lowrank": _lib.ACC_LOWRANK}[acc]
    code = CODE[cdt] | (_lib.PARAM_F32 if flagged else 0)
    pdt = F32 if flagged else cdt
    ar = Arena()

    def param(t):
        return None if t is None else ar.input(t if flagged else t.to(cdt), pdt)

    x, dy = ar.input(d["x"], cdt), ar.input(d["dy"], cdt)
    A, B, bias, acc_down, acc_up = (param(d[k]) for k in ("A", "B", "bias", "acc_down", "acc_up"))
    hcols = 64 if r <= 64 else r
    y, h, dx = ar.output((T, d_out), cdt), ar.output((T, hcols), cdt), ar.output((T, d_in), cdt)
    init = (lambda k: (d[k] if flagged else d[k].to(cdt)) if grad_beta else None)
    dA, dB = ar.output((d_in, r), pdt, init("dA0")), ar.output((r, d_out), pdt, init("dB0"))
    dbias = ar.output((d_out,), pdt, init("dbias0")) if d["bias"] is not None else None
    fws = ar.workspace(lib.sow_forward_workspace_bytes(T, d_in, d_out, r, r_acc, kind, code))
    bws = ar.workspace(lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, kind, code))
    if flagged:
        assert fws is not None and bws is not None
    stream = torch.cuda.current_stream().cuda_stream
    runs = []
    for byte in fills:
        ar.fill(byte)
        _lib.check(lib.sow_forward(_p(x), _p(A), _p(B), _p(acc_down), _p(acc_up), _p(bias), _p(y), _p(h), T, d_in, d_out, r,
                                   r_acc, kind, s, code, _p(fws), 0 if fws is None else fws.numel(), stream), "sow_forward")
        _lib.check(lib.sow_backward_ex(_p(dy), _p(x), _p(h), _p(A), _p(B), _p(acc_down), _p(acc_up), _p(dx), _p(dA), _p(dB),
                                       _p(dbias), T, d_in, d_out, r, r_acc, kind, s, grad_beta, code, _p(bws), bws.numel(),
                                       _lib.BWD_DATA | _lib.BWD_WEIGHTS, stream), "sow_backward_ex")
        ar.check_guards(f"run with 0x{byte:02X}")
        runs.append(dict(y=y.clone(), h=h.clone(), dx=dx.clone(), dA=dA.clone(), dB=dB.clone(),
                         dbias=None if dbias is None else dbias.clone()))
        if want_dh:
            assert bws.data_ptr() % 256 == 0
            runs[-1]["dh"] = bws[:T * hcols * 2].view(cdt).view(T, hcols)[:, :r].clone()
    for k, v in runs[0].items():
        for other in runs[1:]:
            if v is not None and T > 0:
                assert torch.equal(_bits(v), _bits(other[k])), f"{k} differs between poisoned and zeroed memory"
    return runs[0]


# (name, T, d_in, d_out, r, acc, r_acc, bias, scale) -- the path each one reaches, read off api.hip's dispatch
PATHS = [
    ("chain2_T32768", 32768, 768, 768, 50, None, 0, True, 0.5),
    ("chain2_nobias", 32768, 768, 768, 50, None, 0, False, 1.0),
    ("short_T1000", 1000, 768, 768, 50, None, 0, True, 0.5),
    ("dense_gemm4h", 8192, 512, 512, 50, "dense", 0, True, 0.5),
    ("lowrank48", 8192, 512, 520, 50, "lowrank", 48, True, 1.0),
    ("lowrank200", 8192, 512, 520, 50, "lowrank", 200, False, 0.5),
    ("wide_r200", 8192, 1024, 1024, 200, None, 0, True, 0.5),
    ("wide_r200_nobias", 4097, 520, 264, 200, None, 0, False, 1.0),
    ("r64_colsum", 4096, 512, 512, 64, None, 0, True, 1.0),
    ("generic_dout262", 4097, 520, 262, 50, None, 0, True, 0.5),
    ("generic_r300", 4097, 520, 264, 300, None, 0, True, 0.5),
    ("T0", 0, 512, 512, 50, None, 0, True, 1.0),
]


@pytest.mark.parametrize("cdt", HALF, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", PATHS, ids=[c[0] for c in PATHS])
def test_flagged_call_equals_plain_call_on_rounded_parameters(case, cdt):
    name, T, d_in, d_out, r, acc, r_acc, bias, s = case
    d = _inputs(T, d_in, d_out, r, acc, r_acc, bias)
    mixed = _run(d, cdt, T, d_in, d_out, r, acc, r_acc, s, flagged=True)
    for k in ("dA", "dB", "dbias"):
        if mixed[k] is not None:
            assert mixed[k].dtype == F32, k
    if T == 0:
        for k in ("dA", "dB", "dbias"):
            if mixed[k] is not None:
                assert bool((mixed[k] == 0).all()), f"{k}: T = 0 must zero the whole fp32 gradient"
        return
    plain = _run(d, cdt, T, d_in, d_out, r, acc, r_acc, s, flagged=False, fills=(0xFF,))
    for k in ("y", "h", "dx"):
        assert torch.equal(_bits(mixed[k]), _bits(plain[k])), f"{name}: {k} differs from the plain call"
    for k in ("dA", "dB", "dbias"):
        if plain[k] is not None:
            assert torch.equal(_bits(mixed[k].to(cdt)), _bits(plain[k])), f"{name}: {k} rounded to {cdt} differs"


# element-wise against float64: fp32 gradients accumulated onto existing fp32 gradients (grad_beta = 1)
EW = [
    ("chain2", 4096, 768, 776, 50, None, 0, True, 0.5),
    ("dense", 4096, 512, 512, 50, "dense", 0, True, 0.5),
    ("wide_r200", 4096, 512, 520, 200, None, 0, True, 0.5),
    ("r64_colsum", 4096, 512, 512, 64, None, 0, True, 1.0),
    ("generic_r300", 2049, 520, 264, 300, None, 0, True, 0.5),
]


@pytest.mark.parametrize("grad_beta", [0.0, 1.0], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("cdt", HALF, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", EW, ids=[c[0] for c in EW])
def test_fp32_gradients_against_float64(case, cdt, grad_beta):
    """Every fp32 gradient within one fp32 ulp plus fp32 accumulation noise of its float64 reference, computed from the
    operands the kernels summed (h_save, dY, x and the kernels' own dh): a result rounded through bf16 / f16 on its way (half
    an ulp of that type) is hundreds of times past the bound."""
    name, T, d_in, d_out, r, acc, r_acc, bias, s = case
    d = _inputs(T, d_in, d_out, r, acc, r_acc, bias, seed=1)
    out = _run(d, cdt, T, d_in, d_out, r, acc, r_acc, s, flagged=True, grad_beta=grad_beta, fills=(0xFF, 0x00, 0xFF),
               want_dh=True)
    q = {k: to64(v.to(cdt)) for k, v in d.items() if v is not None and k in ("x", "A", "B", "dy")}   # what the kernels saw
    x, A, B, dy = q["x"], q["A"], q["B"], q["dy"]
    dA0, dB0 = grad_beta * to64(d["dA0"]), grad_beta * to64(d["dB0"])
    h = to64(out["h"])
    h = h[:, :r] if r <= 64 else s * h          # r <= 64: h_save = s x A; wider: x A, unscaled
    # dB from the visible h_save and dY, dbias from dY: every rounding is fp32's
    new = h.t() @ dy
    sq = (h * h).t() @ (dy * dy)
    check_bound(out["dB"], new + dB0, ulp(new + dB0, F32) + ulp(new, F32) + fp32_floor(sq, T), name=f"{name}: dB")
    if bias:
        new = dy.sum(0)
        ref = new + grad_beta * to64(d["dbias0"])
        check_bound(out["dbias"], ref, ulp(ref, F32) + ulp(new, F32) + fp32_floor((dy * dy).sum(0), T), name=f"{name}: dbias")
    # dA from x and the kernels' own dh (rounded to the compute dtype before the token sum): again only fp32 roundings
    dh = to64(out["dh"])
    assert rel_err(dh, s * (dy @ B.t())) < 1e-2, f"{name}: the workspace's dh is not s dY B^T"
    new = x.t() @ dh
    sq = (x * x).t() @ (dh * dh)
    ref = new + dA0
    check_bound(out["dA"], ref, ulp(ref, F32) + ulp(new, F32) + fp32_floor(sq, T), name=f"{name}: dA")


# ---------------------------------------------------------------------------------------------- module level
def _layer(d_in=512, d_out=520, rank=50, bias=True, seed=3):
    torch.manual_seed(seed)
    m = SoWLinear(d_in, d_out, bias=bias, rank=rank, init_method="normal", device=DEV)
    with torch.no_grad():
        m.bias.normal_(0, 0.1) if bias else None
    return m


@pytest.mark.parametrize("cdt", HALF, ids=["bf16", "f16"])
@pytest.mark.parametrize("x_dtype", ["f32", "compute"])
def test_sowlinear_under_autocast(cdt, x_dtype):
    layer = _layer()
    twin = copy.deepcopy(layer).to(cdt)          # the factors autocast would hand the kernels
    xd = F32 if x_dtype == "f32" else cdt
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(4, 1024, 512, device=DEV, generator=g).to(xd).requires_grad_()
    dy = torch.randn(4, 1024, 520, device=DEV, generator=g).to(cdt)
    with torch.autocast("cuda", dtype=cdt):
        y = layer(x)
    assert y.dtype == cdt
    y.backward(dy)
    A, B = layer.downscale_weights[0], layer.upscale_weights[0]
    assert A.grad.dtype == F32 and B.grad.dtype == F32 and layer.bias.grad.dtype == F32
    assert x.grad.dtype == xd
    # the same bits as the plain layer on rounded factors (x cast as autocast casts it)
    xt = x.detach().to(cdt).requires_grad_()
    yt = twin(xt)
    yt.backward(dy)
    assert torch.equal(_bits(y), _bits(yt))
    assert torch.equal(_bits(x.grad.to(cdt)), _bits(xt.grad)) and (xd == cdt or torch.equal(x.grad, xt.grad.float()))
    for p, q in ((A, twin.downscale_weights[0]), (B, twin.upscale_weights[0]), (layer.bias, twin.bias)):
        assert torch.equal(_bits(p.grad.to(cdt)), _bits(q.grad))
    # against the oracle on the autocast-rounded operands
    r64 = lambda t: t.detach().to(cdt).double().cpu()
    y_ref = O.sow_forward(r64(x), [r64(A)], [r64(B)], None, None, 1.0, r64(layer.bias))
    assert rel_err(y.detach().cpu(), y_ref) < 1e-2
    dx_ref, dA_ref, dB_ref, db_ref = O.sow_backward(r64(dy), r64(x), [r64(A)], [r64(B)], None, None, 1.0, True)
    assert rel_err(x.grad.cpu(), dx_ref) < 1e-2
    assert rel_err(A.grad.cpu(), dA_ref[0]) < 1e-2 and rel_err(B.grad.cpu(), dB_ref[0]) < 1e-2
    assert rel_err(layer.bias.grad.cpu(), db_ref) < 1e-5
    # the no-grad forward (h not saved) gives the training forward's bits
    with torch.no_grad(), torch.autocast("cuda", dtype=cdt):
        y_ng = layer(x.detach())
    assert y_ng.dtype == cdt and torch.equal(_bits(y_ng), _bits(y))


def test_autocast_with_accumulator_and_accumulate():
    """An fp32 layer whose dense accumulator is fp32 (after accumulate()) runs under autocast; the next forward uses the new
    accumulator."""
    layer = _layer(rank=16)
    x = torch.randn(2048, 512, device=DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        y0 = layer(x)
        layer.accumulate()
        assert layer.acc_downweight.dtype == F32 and layer.acc_downweight.numel() > 0
        y1 = layer(x)
    twin = copy.deepcopy(layer).to(BF16)
    with torch.no_grad():
        assert torch.equal(_bits(y1), _bits(twin(x.to(BF16))))
    assert rel_err(y1.float().cpu(), y0.float().cpu()) < 5e-2


def test_refused_combinations():
    x = torch.randn(64, 512, device=DEV)
    layer = _layer().to(BF16)
    with torch.autocast("cuda", dtype=F16):
        with pytest.raises(TypeError, match="bfloat16 parameters"):
            layer(x)
    fp32_layer = _layer()
    prev_on, prev_dt = torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")
    torch.set_autocast_enabled("cuda", True)
    torch.set_autocast_dtype("cuda", F32)
    try:
        with pytest.raises(TypeError, match="autocast dtype torch.float32"):
            fp32_layer(x)
    finally:
        torch.set_autocast_dtype("cuda", prev_dt)
        torch.set_autocast_enabled("cuda", prev_on)
    # outside autocast nothing changes: fp32 in, fp32 out; bf16 factors with fp32 input still raise
    assert fp32_layer(x).dtype == F32
    with pytest.raises(TypeError):
        layer(x)


# ---------------------------------------------------------------------------------------------- sibling groups
class _Block(nn.Module):
    """A llama-shaped block of SoWLinear layers: q/k/v and gate/up read the fp32 residual stream, o and down read products
    that autocast leaves in the compute dtype."""

    def __init__(self, d=256, dff=512, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        mk = lambda i, o: SoWLinear(i, o, bias=False, rank=16, init_method="normal", device=DEV)
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = mk(d, d), mk(d, d), mk(d, d), mk(d, d)
        self.gate_proj, self.up_proj, self.down_proj = mk(d, dff), mk(d, dff), mk(dff, d)

    def forward(self, h):
        a = self.q_proj(h) * self.k_proj(h) + self.v_proj(h)
        h = h + self.o_proj(a)
        return h + self.down_proj(F.silu(self.gate_proj(h)) * self.up_proj(h))


@pytest.mark.parametrize("cdt", HALF, ids=["bf16", "f16"])
def test_sibling_groups_under_autocast(cdt):
    from sow_amd import group_siblings
    base = nn.Sequential(_Block(seed=1), _Block(seed=2))
    twin = copy.deepcopy(base)
    assert group_siblings(twin) == 4
    x = torch.randn(8, 512, 256, device=DEV)
    outs = []
    for net in (base, twin):
        xi = x.clone().requires_grad_()
        with torch.autocast("cuda", dtype=cdt):
            y = net(xi)
        y.float().square().mean().backward()
        outs.append((y.detach(), xi.grad))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0]))
    assert outs[0][1].dtype == F32 and rel_err(outs[1][1].cpu(), outs[0][1].cpu()) < 1e-5
    for (n1, p1), (_, p2) in zip(base.named_parameters(), twin.named_parameters()):
        if p1.grad is not None:
            assert p1.grad.dtype == F32 and p2.grad.dtype == F32, n1
            assert rel_err(p2.grad.cpu(), p1.grad.cpu()) < 2e-2, n1
    # one block's q/k/v alone: their input gradient is the fp32 sum of the three, bit for bit
    blk_u, blk_g = copy.deepcopy(base[0]), copy.deepcopy(base[0])
    assert group_siblings(blk_g) == 2
    res = []
    for blk in (blk_u, blk_g):
        xi = x.clone().requires_grad_()
        with torch.autocast("cuda", dtype=cdt):
            ys = (blk.q_proj(xi), blk.k_proj(xi), blk.v_proj(xi))
        torch.autograd.backward([y for y in ys], [torch.ones_like(y) for y in ys])
        res.append((ys, xi.grad))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(res[0][1], res[1][1])


def test_group_plan_with_the_flag():
    """sow_backward_group_plan reports the same grouped plan for a flagged decoder block as for the plain one."""
    import ctypes
    lib = _lib.load()
    T, fake = 32768, 0x10000
    shapes = [(512, 512)] * 4 + [(512, 1376), (512, 1376), (1376, 512)]
    arr = (_lib.LayerArgs * len(shapes))()
    for i, (di, do) in enumerate(shapes):
        a = arr[i]
        a.x = a.A = a.B = a.y = a.h_save = a.dy = a.dx = a.dA = a.dB = fake
        a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale, a.grad_beta = T, di, do, 50, 0, 1.0, 1.0
        a.workspace = fake
        a.workspace_bytes = lib.sow_workspace_bytes(T, di, do, 50, 0, 0, _lib.BF16 | _lib.PARAM_F32)
    phases = _lib.BWD_WEIGHTS_PARTIAL | _lib.BWD_GROUP_SLABS
    plans = []
    for code in (_lib.BF16, _lib.BF16 | _lib.PARAM_F32):
        slabs = (ctypes.c_int * (2 * len(shapes)))()
        plans.append((lib.sow_backward_group_plan(arr, len(shapes), code, phases, slabs), list(slabs)))
    assert plans[0] == plans[1] and plans[0][0] == 1


# ---------------------------------------------------------------------------------------------- FactorBucket
def test_factor_bucket_fp32_under_bf16_autocast():
    from sow_amd import prepare
    from sow_amd.dp import FactorBucket, factor_parameters
    from sow_amd.optimizer import FactorAdamW
    base = nn.Sequential(_Block(seed=3), _Block(seed=4))
    ref = copy.deepcopy(base)
    x = torch.randn(4, 1024, 256, device=DEV)

    def loss_of(net):
        with torch.autocast("cuda", dtype=BF16):
            y = net(x)
        return y.float().square().mean()

    bucket = FactorBucket(factor_parameters(base))
    assert bucket.flat_grad.dtype == F32
    assert bucket.attach(base) == 14
    bucket.zero_grad()
    loss_of(base).backward()
    bucket.finalize()
    loss_of(ref).backward()
    for (n1, p1), (_, p2) in zip(base.named_parameters(), ref.named_parameters()):
        if p2.grad is not None and p1.dim() == 2:
            assert p1.grad.dtype == F32
            assert rel_err(p1.grad.cpu(), p2.grad.cpu()) < 1e-5, n1
    opt = FactorAdamW(bucket, lr=1e-3)
    params0 = bucket.flat_param.clone()
    for step in range(3):
        if step:
            bucket.zero_grad()
            loss_of(base).backward()
        opt.step()
        if step == 1:
            prepare.accumulate(base)
            q = base[1].q_proj
            assert q.acc_downweight.dtype == F32 and q.acc_downweight.numel() > 0
            with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
                y_after = q(x)
            sink = q.__dict__.pop("_grad_sink")
            twin = copy.deepcopy(q).to(BF16)       # a plain bf16 copy of the layer (no bucket)
            q._grad_sink = sink
            with torch.no_grad():
                assert torch.equal(_bits(y_after), _bits(twin(x.to(BF16))))   # the new fp32 accumulator, rounded once
    torch.cuda.synchronize()
    assert torch.isfinite(bucket.flat_param).all() and not torch.equal(bucket.flat_param, params0)


def test_factor_bucket_switching_precision_between_steps():
    """One fp32 bucket, steps in turn outside autocast (the F32 kernels), under bf16 and under f16 autocast (PARAM_F32): the
    sink's workspace and the cached reduction descriptors must follow the run dtype.  Each step's gradients equal the
    unattached per-layer path on the same weights."""
    from sow_amd.dp import FactorBucket, factor_parameters
    base = nn.Sequential(_Block(seed=5), _Block(seed=6))
    ref = copy.deepcopy(base)
    bucket = FactorBucket(factor_parameters(base))
    assert bucket.attach(base) == 14
    x = torch.randn(4, 1024, 256, device=DEV)
    for mode in (None, BF16, F16, None, BF16):
        bucket.zero_grad()
        ref.zero_grad(set_to_none=True)
        for net in (base, ref):
            with torch.autocast("cuda", dtype=mode or BF16, enabled=mode is not None):
                y = net(x)
            y.float().square().mean().backward()
        bucket.finalize()
        for (n1, p1), (_, p2) in zip(base.named_parameters(), ref.named_parameters()):
            if p2.grad is not None:
                assert p1.grad.dtype == F32
                assert rel_err(p1.grad.cpu(), p2.grad.cpu()) < 1e-5, (mode, n1)


# ---------------------------------------------------------------------------------------------- GradScaler (f16)
def test_grad_scaler_f16():
    layer = _layer()
    opt = torch.optim.SGD(layer.parameters(), lr=0.1)
    x = torch.randn(2048, 512, device=DEV)
    for init_scale, finite in ((2.0 ** 40, False), (1024.0, True)):
        scaler = torch.amp.GradScaler("cuda", init_scale=init_scale)
        before = [p.detach().clone() for p in layer.parameters()]
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=F16):
            loss = layer(x).float().square().mean()
        scaler.scale(loss).backward()
        A = layer.downscale_weights[0]
        assert A.grad.dtype == F32
        assert bool(torch.isfinite(A.grad).all()) == finite
        scaler.step(opt)
        scaler.update()
        changed = any(not torch.equal(b, p.detach()) for b, p in zip(before, layer.parameters()))
        assert changed == finite, "an overflowing step must be skipped, a finite one taken"
        if not finite:
            assert scaler.get_scale() < init_scale
