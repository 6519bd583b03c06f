"""Biased SoWLinear layers in the flat bucket (FactorBucket(factor_parameters(model, biases=True)).attach): the sink routes
carry dbias -- single layer, grouped siblings, shared-input siblings -- and one row-owner launch covers an encoder block.

Every case is compared against a deep copy whose bucket holds no biases, so that its (biased) layers keep autograd:
y and dX bit for bit; dA and dB bit for bit wherever both models cut the token axis into the same slabs; bias.grad
element-wise against colsum(dY) in float64 on the exact dY values, and against the oracle at test_gpu_parity.py's tolerance.

Cases whose dA / dB cannot be bit-identical (ROWS_PLAN below): 16-bit compute dtypes at 8257 and 32769 tokens.  There the
attached block of six layers takes the row-owner kernel with slab counts planned over the block (16 slabs at 8257
tokens), the autograd copy each layer's own plan (17): the fp32 slab sums are added in another order.  These cases hold
dA and dB element-wise to float64 with the bounds of test_gpu_elementwise.py (one output ulp, the hidden 16-bit rounding
of h / dh, the fp32 floor over T terms).  Every fp32 case and every 700-token case is bit-identical.
"""
import copy

import pytest
import torch
import torch.nn as nn

import test_gpu_elementwise as E
from conftest import rel_err
from numerics import UNIT_ROUNDOFF, accumulation_term, bound, check_bound, fp32_floor, to64, ulp
from oracle import sow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
U32 = UNIT_ROUNDOFF[F32]
# test_gpu_parity.py: 1e-5 for fp32, 2e-2 for bf16 against the fp32 oracle; f16 carries three more significand bits than bf16
PARITY_TOL = {F32: 1e-5, BF16: 2e-2, F16: 2e-2 / 8}
RANK, R_ACC, SCALE = 8, 24, 0.75
GEOMETRIES = {"short": (96, 200, 700),        # the short-input forms (at most 8192 tokens split K / the output columns)
              "stream": (128, 264, 8257)}     # the streaming forms, one ragged 64-token tile
FUSE_GEOMETRY = (128, 264, 32769)             # SOW_FUSE_ACC is taken from 32768 tokens on (ops.fused_acc_pays)


def ROWS_PLAN(T, cdt):
    """The attached block's weight gradients run on the row-owner kernel with slab counts planned over the block
    (sow_backward_group_plan: bf16 / f16 compute, enough tokens to fill the chip); the autograd copy keeps per-layer plans."""
    return cdt != F32 and T > 8192


class Attention(nn.Module):
    def __init__(self, mk, hidden):
        super().__init__()
        self.query, self.key, self.value, self.dense = mk(hidden, hidden), mk(hidden, hidden), mk(hidden, hidden), mk(hidden, hidden)


class Block(nn.Module):
    def __init__(self, mk, hidden, inter):
        super().__init__()
        self.attention = Attention(mk, hidden)
        self.intermediate, self.output = mk(hidden, inter), mk(inter, hidden)

    def forward(self, x):
        a = self.attention
        q, k, v = a.query(x), a.key(x), a.value(x)
        x = x + a.dense(torch.tanh(q) * torch.sigmoid(k) + v)
        return x + self.output(torch.tanh(self.intermediate(x)))


class Encoder(nn.Module):
    """Two encoder blocks of six biased SoWLinear layers; module names `layer.0.attention.query` ... `layer.1.output`."""

    def __init__(self, hidden, inter, dtype, acc, rank=RANK, gen=None):
        super().__init__()

        def mk(i, o):
            from sow_amd import SoWLinear
            m = SoWLinear(i, o, bias=True, rank=rank, scale=SCALE, init_method="normal", device=DEV, dtype=dtype)
            rnd = lambda *s, std: (torch.randn(*s, generator=gen) * std).to(DEV, dtype)
            m.downscale_weights[0].data.copy_(rnd(i, rank, std=0.08))
            m.upscale_weights[0].data.copy_(rnd(rank, o, std=0.05))
            m.bias.data.copy_(rnd(o, std=0.1))
            if acc == "dense":
                m.acc_downweight = nn.Parameter(rnd(i, o, std=0.02), requires_grad=False)
            elif acc == "lowrank":
                m.acc_downweight = nn.Parameter(rnd(i, R_ACC, std=0.1), requires_grad=False)
                m.acc_upweight = nn.Parameter(rnd(R_ACC, o, std=0.05), requires_grad=False)
            return m

        self.layer = nn.ModuleList([Block(mk, hidden, inter), Block(mk, hidden, inter)])

    def forward(self, x):
        for b in self.layer:
            x = b(x)
        return x

    def sow(self):
        from sow_amd import SoWLinear
        return [(n, m) for n, m in self.named_modules() if isinstance(m, SoWLinear)]


def _record(model):
    """Forward hooks that keep every layer's input and the gradient of its output (the exact dY the kernels read)."""
    rec = {}
    for name, m in model.sow():
        def hook(mod, inp, out, name=name):
            rec[name] = {"x": inp[0].detach()}
            out.register_hook(lambda g, name=name: rec[name].__setitem__("dy", g.detach().clone()))
        m.register_forward_hook(hook)
    return rec


def _run(model, x, w, autocast):
    x = x.detach().clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        y = model(x)
    (y.float() * w).sum().backward()
    return y.detach(), x.grad.detach()


def _grads(model):
    return {n: (m.downscale_weights[0].grad.detach().clone(), m.upscale_weights[0].grad.detach().clone(),
                m.bias.grad.detach().clone()) for n, m in model.sow()}


def _check_dbias(name, got, dy, cdt, first=None):
    """bias.grad against colsum(dY) in float64 on the exact dY values: the bound of test_gpu_elementwise.py:339-344
    (`first`: the gradient already in the buffer, grad_beta = 1)."""
    dy64 = to64(dy).reshape(-1, dy.shape[-1])
    T = dy64.shape[0]
    ref = dy64.sum(0) + (to64(first) if first is not None else 0)
    sq = (dy64 * dy64).sum(0)
    if got.dtype == F32:
        return check_bound(got, ref, bound(ref, F32, accumulation_term(sq, U32, T)), name=f"{name}: dbias")
    return E._rounded(got, ref, got.dtype, fp32_floor(sq, T), f"{name}: dbias")


def _check_dA_dB(name, m, x, dy, cdt, dA, dB):
    """dA = x^T dh and dB = h^T dY against float64, h = s x A and dh = s dY B^T rounded to the compute dtype where the test
    cannot see them: test_gpu_elementwise.py's dA bound, applied to both."""
    A, B = m.downscale_weights[0].detach(), m.upscale_weights[0].detach()
    x64, dy64 = to64(x.reshape(-1, x.shape[-1]).to(cdt)), to64(dy.reshape(-1, dy.shape[-1]))
    A64, B64 = to64(A.to(cdt)), to64(B.to(cdt))           # fp32 factors under autocast: rounded once by the library
    T, r = x64.shape[0], A64.shape[1]
    u = UNIT_ROUNDOFF[cdt]
    h, dh = SCALE * (x64 @ A64), SCALE * (dy64 @ B64.t())
    xx, dydy = x64 * x64, dy64 * dy64
    dA_ref, dA_sq = x64.t() @ dh, xx.t() @ (dh * dh)
    dB_ref, dB_sq = h.t() @ dy64, (h * h).t() @ dydy
    subA = [E._sub_term(xx.sum(0)[:, None].expand(-1, r), cdt)] if cdt == F16 else []
    subB = [E._sub_term(dydy.sum(0)[None, :].expand(r, -1), cdt)] if cdt == F16 else []
    sa = check_bound(dA, dA_ref, bound(dA_ref, dA.dtype, accumulation_term(dA_sq, u, 1), fp32_floor(dA_sq, T), *subA),
                     name=f"{name}: dA")
    sb = check_bound(dB, dB_ref, bound(dB_ref, dB.dtype, accumulation_term(dB_sq, u, 1), fp32_floor(dB_sq, T), *subB),
                     name=f"{name}: dB")
    return sa, sb


def _check_twice(name, got, first, exact):
    """A second identical backward before finalize() adds the same fp32 sum S to the stored g1 = rn(S): fp32 gradients
    double exactly; a 16-bit gradient is rn(g1 + S) with |S - g1| <= ulp(g1) / 2, within one ulp of 2 g1."""
    if exact:
        assert torch.equal(got, 2 * first), f"{name}: the second backward did not add the same gradient"
    else:
        check_bound(got, 2 * to64(first), ulp(2 * to64(first), got.dtype), name=name)


CASES = [(g, dt, acc, False) for g in GEOMETRIES for dt in (BF16, F16, F32) for acc in ("none", "dense")] + \
        [(g, F32, "none", True) for g in GEOMETRIES]


def _id(c):
    g, dt, acc, autocast = c
    return f"{g}-{str(dt).split('.')[-1]}-{acc}" + ("-autocast" if autocast else "")


def _block_case(monkeypatch, hidden, inter, T, dtype, acc, autocast, modes):
    from sow_amd import dp, group_siblings
    from sow_amd.dp import FactorBucket, factor_parameters
    cdt = BF16 if autocast else dtype
    gen = torch.Generator().manual_seed(hidden + T + 7 * len(acc))
    base = Encoder(hidden, inter, dtype, acc, gen=gen)
    x = torch.randn(T, hidden, generator=gen).to(DEV, F32 if autocast else dtype)
    w = torch.randn(T, hidden, generator=gen).to(DEV)
    calls = []
    orig = dp._GradSink.queue
    monkeypatch.setattr(dp._GradSink, "queue", lambda self, *a: (calls.append(1), orig(self, *a))[1])
    for mode in modes:
        ref, net = copy.deepcopy(base), copy.deepcopy(base)
        if mode != "ungrouped":
            for m in (ref, net):
                assert group_siblings(m, shared_input=(mode == "shared")) == 2
        ref_bucket = FactorBucket(factor_parameters(ref))               # today's behaviour: no biased layer is attached
        assert ref_bucket.attach(ref) == 0
        bucket = FactorBucket(factor_parameters(net, biases=True))
        assert bucket.attach(net) == 12
        rec = _record(net)
        tag = f"{mode} T={T} {dtype} acc={acc}" + (" autocast" if autocast else "")
        # ---- first backward
        y0, dx0 = _run(ref, x, w, autocast)
        del calls[:]
        y1, dx1 = _run(net, x, w, autocast)
        assert len(calls) == 12, f"{tag}: {len(calls)} sink passes for two blocks of six layers"
        assert all(m.bias.grad.data_ptr() == bucket.grad_ptr(m.bias) for _, m in net.sow())
        bucket.finalize()
        torch.cuda.synchronize()
        assert torch.equal(y0, y1), f"{tag}: y"
        assert torch.equal(dx0, dx1), f"{tag}: dX"
        g_ref, g1 = _grads(ref), _grads(net)
        for name, m in net.sow():
            dA, dB, db = g1[name]
            assert db.dtype == dtype and dA.dtype == dtype              # fp32 gradients under autocast (SOW_PARAM_F32)
            if ROWS_PLAN(T, cdt):
                sa, sb = _check_dA_dB(f"{tag} {name}", m, rec[name]["x"], rec[name]["dy"], cdt, dA, dB)
            else:
                assert torch.equal(dA, g_ref[name][0]), f"{tag} {name}: dA differs from the autograd copy"
                assert torch.equal(dB, g_ref[name][1]), f"{tag} {name}: dB differs from the autograd copy"
            st = _check_dbias(f"{tag} {name}", db, rec[name]["dy"], cdt)
            dy, xin = rec[name]["dy"], rec[name]["x"].to(cdt)
            f = lambda t: t.detach().float().cpu()
            kind_dn = f(m.acc_downweight.to(cdt)) if m.acc_downweight.numel() else None
            kind_up = f(m.acc_upweight.to(cdt)) if m.acc_upweight.numel() else None
            db_o = O.sow_backward(f(dy), f(xin), [f(m.downscale_weights[0].to(cdt))], [f(m.upscale_weights[0].to(cdt))],
                                  kind_dn, kind_up, SCALE, True)[3]
            assert rel_err(f(db), db_o) < PARITY_TOL[dtype], f"{tag} {name}: dbias against the oracle"
        # ---- gradient accumulation: a second backward before finalize()
        _run(net, x, w, autocast)
        bucket.finalize()
        torch.cuda.synchronize()
        g2 = _grads(net)
        for name, _ in net.sow():
            for k, what in enumerate(("dA", "dB")):
                _check_twice(f"{tag} {name}: {what} after two backward passes", g2[name][k], g1[name][k], dtype == F32)
            _check_dbias(f"{tag} {name} (second backward)", g2[name][2], rec[name]["dy"], cdt, first=g1[name][2])
        del ref, net, bucket, ref_bucket, rec


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_biased_block_against_autograd_copy(case, monkeypatch):
    g, dtype, acc, autocast = case
    hidden, inter, T = GEOMETRIES[g]
    _block_case(monkeypatch, hidden, inter, T, dtype, acc, autocast, ("ungrouped", "grouped", "shared"))


def test_biased_block_lowrank_accumulator_fused_pass(monkeypatch):
    """bf16 with a low-rank accumulator at a token count where the module surface passes SOW_FUSE_ACC."""
    from sow_amd import _lib, ops
    hidden, inter, T = FUSE_GEOMETRY
    for d_in, d_out in ((hidden, hidden), (hidden, inter), (inter, hidden)):
        assert ops.fuse_acc_default(T, d_in, d_out, RANK, R_ACC, _lib.ACC_LOWRANK, BF16)
    _block_case(monkeypatch, hidden, inter, T, BF16, "lowrank", False, ("ungrouped", "grouped"))


class One(nn.Module):
    def __init__(self, r, dtype, gen):
        super().__init__()
        from sow_amd import SoWLinear
        m = SoWLinear(96, 200, bias=True, rank=r, scale=SCALE, init_method="normal", device=DEV, dtype=dtype)
        m.downscale_weights[0].data.copy_((torch.randn(96, r, generator=gen) * 0.08).to(DEV, dtype))
        m.upscale_weights[0].data.copy_((torch.randn(r, 200, generator=gen) * 0.05).to(DEV, dtype))
        self.layer = nn.ModuleList([nn.ModuleDict({"dense": m})])

    @property
    def m(self):
        return self.layer[0]["dense"]

    def forward(self, x):
        return self.m(x)

    def sow(self):
        return [("layer.0.dense", self.m)]


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("r", [63, 64, 72])
def test_single_biased_layer_rank_63_64_72(r, dtype, monkeypatch):
    """r = 63: the last rank with a free ones column (column 62 is live and must not leak into dbias); r = 64: no free
    column, the layer keeps autograd and its gradients still land in the flat views; r = 72: the wide route, dbias from
    the PARTIAL phase (skinny_tn_wide's side sum)."""
    from sow_amd import dp
    from sow_amd.dp import FactorBucket, factor_parameters
    gen = torch.Generator().manual_seed(r)
    base = One(r, dtype, gen)
    T = 777
    x = torch.randn(T, 96, generator=gen).to(DEV, dtype)
    w = torch.randn(T, 200, generator=gen).to(DEV)
    ref, net = copy.deepcopy(base), copy.deepcopy(base)
    FactorBucket(factor_parameters(ref))
    bucket = FactorBucket(factor_parameters(net, biases=True))
    assert bucket.attach(net) == (0 if r == 64 else 1)
    calls = []
    orig = dp._GradSink.queue
    monkeypatch.setattr(dp._GradSink, "queue", lambda self, *a: (calls.append(1), orig(self, *a))[1])
    rec = _record(net)
    y0, dx0 = _run(ref, x, w, False)
    y1, dx1 = _run(net, x, w, False)
    bucket.finalize()
    torch.cuda.synchronize()
    assert len(calls) == (0 if r == 64 else 1)
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    m = net.m
    for p in (m.downscale_weights[0], m.upscale_weights[0], m.bias):
        assert p.grad.data_ptr() == bucket.grad_ptr(p)                  # attached or not, the gradients are in the flat buffer
    assert float(bucket.flat_grad.abs().sum()) > 0
    (dA0, dB0, db0), (dA, dB, db) = _grads(ref)["layer.0.dense"], _grads(net)["layer.0.dense"]
    assert torch.equal(dA, dA0) and torch.equal(dB, dB0)
    dy = rec["layer.0.dense"]["dy"]
    _check_dbias(f"r={r} {dtype}", db, dy, dtype)
    if r == 63:
        # column 62 of the saved projection is the layer's last live column, column 63 the ones column: dB's row 62 is the
        # live product, and dbias is the column sum alone (the autograd copy takes it from the same column)
        assert torch.equal(db, db0)
    assert rel_err(db.float().cpu(), dy.float().sum(0).cpu()) < PARITY_TOL[dtype]
    g1 = _grads(net)["layer.0.dense"]
    _run(net, x, w, False)
    bucket.finalize()
    torch.cuda.synchronize()
    g2 = _grads(net)["layer.0.dense"]
    for k, what in enumerate(("dA", "dB")):
        # (the wide route applies the layer's scale to dB in the epilogue of the accumulating sum: one rounding of s S + g1)
        _check_twice(f"r={r} {dtype}: {what} after two backward passes", g2[k], g1[k], dtype == F32 and r <= 64)
    _check_dbias(f"r={r} {dtype} (second backward)", g2[2], dy, dtype, first=g1[2])


def test_two_group_step_matches_torch_adamw():
    """One training step end to end in fp32: the attached model with a two-group FactorAdamW (factors at sow_lr with weight
    decay, biases at lr without) and a dense head against torch.optim.AdamW with run_glue.py's three groups on the
    autograd copy; reset_state(0) after the first step resets the factor group alone."""
    from sow_amd.dp import FactorBucket, factor_parameters
    from sow_amd.optimizer import FactorAdamW
    hidden, inter, T = GEOMETRIES["short"]
    gen = torch.Generator().manual_seed(5)
    enc = Encoder(hidden, inter, F32, "dense", gen=gen)
    head = nn.Linear(hidden, 4).to(DEV)
    ref_enc, ref_head = copy.deepcopy(enc), copy.deepcopy(head)
    x = torch.randn(T, hidden, generator=gen).to(DEV)
    w = torch.randn(T, 4, generator=gen).to(DEV)
    lr, sow_lr, wd = 2e-3, 1e-2, 0.1
    params = factor_parameters(enc, biases=True)
    bucket = FactorBucket(params)
    assert bucket.attach(enc) == 12
    n_fac = len(factor_parameters(enc))
    opt = FactorAdamW(bucket, param_groups=[{"params": params[:n_fac], "lr": sow_lr, "weight_decay": wd},
                                            {"params": params[n_fac:], "lr": lr, "weight_decay": 0.0}])
    opt_head = torch.optim.AdamW([{"params": [head.weight], "lr": lr, "weight_decay": wd},
                                  {"params": [head.bias], "lr": lr, "weight_decay": 0.0}])
    ref_fac = factor_parameters(ref_enc)
    ref_bias = [m.bias for _, m in ref_enc.sow()]
    ref_opt = torch.optim.AdamW([{"params": [ref_head.weight], "lr": lr, "weight_decay": wd},
                                 {"params": ref_fac, "lr": sow_lr, "weight_decay": wd},
                                 {"params": ref_bias + [ref_head.bias], "lr": lr, "weight_decay": 0.0}])

    def backward(e, h):
        (h(e(x)) * w).sum().backward()

    def compare(what):
        torch.cuda.synchronize()
        for p, q in zip(params, ref_fac + ref_bias):
            assert rel_err(p.data.cpu(), q.data.cpu()) < 1e-5, what          # test_adamw_flat_matches_torch's tolerances
        assert rel_err(head.weight.data.cpu(), ref_head.weight.data.cpu()) < 1e-5
        for p, o, q in zip(params, bucket.offsets, ref_fac + ref_bias):
            st = ref_opt.state[q]
            m, v = opt.exp_avg[o:o + p.numel()].view_as(p), opt.exp_avg_sq[o:o + p.numel()].view_as(p)
            if float(st["exp_avg"].abs().max()) > 0:
                assert rel_err(m.cpu(), st["exp_avg"].cpu()) < 1e-6 and rel_err(v.cpu(), st["exp_avg_sq"].cpu()) < 1e-6, what
            else:
                assert float(m.abs().max()) == 0 and float(v.abs().max()) == 0, what

    backward(ref_enc, ref_head)
    backward(enc, head)
    ref_opt.step()
    opt.step()
    opt_head.step()
    compare("first step")
    assert opt.group_steps == [1, 1]
    # reset_optimizer for the factor group alone (training_utils.py:257-277): moments and step of that group
    opt.reset_state(0)
    for q in ref_fac:
        st = ref_opt.state[q]
        st["exp_avg"].zero_()
        st["exp_avg_sq"].zero_()
        st["step"] = torch.zeros_like(st["step"]) if torch.is_tensor(st["step"]) else 0
    assert opt.group_steps == [0, 1]
    tail = bucket.offsets[n_fac]
    assert float(opt.exp_avg[:tail].abs().max()) == 0 and float(opt.exp_avg_sq[:tail].abs().max()) == 0
    assert float(opt.exp_avg[tail:].abs().max()) > 0 and float(opt.exp_avg_sq[tail:].abs().max()) > 0   # the biases keep theirs
    compare("after reset_state(0)")
    for o in (opt, opt_head, ref_opt):
        o.zero_grad()
    backward(ref_enc, ref_head)
    backward(enc, head)
    ref_opt.step()
    opt.step()
    opt_head.step()
    compare("second step")
    assert opt.group_steps == [1, 2]
