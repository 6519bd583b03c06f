"""-m gpu: float16 layers end to end -- the f16 streaming kernels (chain2_f16_kernel, gemm4_f16_kernel) and the generic kernels'
f16 instantiations, checked element by element against float64, with poisoned memory and guard bands in the style of
tests/test_gpu_elementwise.py; then the public surfaces (grouped calls, sow_gemm, qr_thin, accumulate) and the reference's
evaluation protocol (model.half()).

f16 numerics (p = 11 bits, e_min = -14, subnormal spacing 2^-24; include/sow_amd.h): fp32 accumulation, one RNE rounding per
output.  Limits:
* rounded once from operands the test can see (h_save from x, A; y from the kernel's own h_save; dB from h_save, dY): within
  one ulp of RNE_f16(fp64 reference) at every element, and bit-equal at all but 0.5 % of them (an fp32 sum lands on the other
  side of an f16 rounding boundary only within ~2^-13 ulp of a tie).  Near zero, where an f16 ulp (down to 2^-24) is finer
  than the fp32 sum itself, the limit has a floor of 4 * 2^-24 * sqrt(K) * sqrt(sum_k (a_k b_k)^2): the standard deviation
  of K fp32 roundings of partial sums, times 4;
* through a rounding the test cannot see (dX and dA through dh; y of the paths that round twice): |err| <= ulp(ref) +
  4 * 2^-11 * sqrt(sum_k (a_k b_k)^2) -- each hidden term carries an independent rounding error of at most 2^-11 relative,
  so their sum has a standard deviation below 2^-11 sqrt(sum (a_k b_k)^2) / sqrt(3); 4x that is a ~7-sigma bound.
"""
import math
import os

import pytest
import torch

from sow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16 = torch.float16
U16 = 2.0 ** -11          # unit roundoff of f16
EMIN = -14
SUB = 2.0 ** -24          # subnormal spacing
GUARD = 64
SENTINEL = -7.25          # exact in f16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- f16 helpers (tests/numerics.py knows bf16 / fp32 only) ----------------------------------------------------------
def rne16(x64):
    """fp64 -> f16, rounded once to nearest even (numpy's float64 -> float16 cast is a single rounding)."""
    import numpy as np
    return torch.from_numpy(x64.detach().cpu().numpy().astype(np.float16)).to(torch.float64)


def ulp16(x64):
    """spacing of f16 at |x| (subnormal spacing below 2^-14; 2^5 ulp above the top binade keeps inf out of the limits)."""
    a = x64.abs().clamp_min(2.0 ** EMIN)
    e = torch.floor(torch.log2(a))
    return torch.exp2(e - 10)


def fp32_floor(a64, b64):
    """4 * 2^-24 * sqrt(K) * sqrt(sum_k (a_k b_k)^2) of the product a64 @ b64."""
    return 4 * 2.0 ** -24 * math.sqrt(a64.shape[-1]) * ((a64 * a64) @ (b64 * b64)).sqrt()


def check_once(got, ref64, what, floor=None, frac=0.005):
    g = got.detach().cpu().to(torch.float64)
    r16 = rne16(ref64)
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    err = (g - r16).abs()
    lim = ulp16(r16) if floor is None else ulp16(r16) + floor
    bad = err > lim
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond 1 ulp (worst {float((err / lim).max()):.3g} ulp)"
    # at most 0.5 % not bit-equal -- and at least one allowed: below 200 elements (T = 1) the rule would demand a perfect score
    neq = int((g != r16).sum())
    assert neq <= max(1, int(frac * g.numel())), f"{what}: {neq} of {g.numel()} elements are not RNE_f16(ref)"


def check_bound16(got, a64, b64, what, bias64=None, beta_term=None, extra=None):
    """got ~ a64 @ b64 (+ bias): |err| <= ulp(ref) + 4 u sqrt(sum_k (a_k b_k)^2) (+ extra: the ulp of a first, separately
    rounded product on the paths that round y twice)."""
    g = got.detach().cpu().to(torch.float64)
    ref = a64 @ b64
    if bias64 is not None:
        ref = ref + bias64
    acc = (a64 * a64) @ (b64 * b64)
    if beta_term is not None:
        ref = ref + beta_term[0]
        acc = acc + beta_term[1]
    lim = ulp16(ref) + 4 * U16 * acc.sqrt() + SUB
    if extra is not None:
        lim = lim + extra
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    err = (g - ref).abs()
    bad = err > lim
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond the bound (worst {float((err / lim).max()):.3g})"


class Arena:
    """Guarded, NaN-neighboured inputs; sentinel-guarded, poisonable outputs; poisonable workspaces."""

    def __init__(self, misalign=0):
        self.misalign, self.outs = misalign, []

    def input(self, t):
        if t is None:
            return None
        off, n = GUARD + self.misalign, t.numel()
        buf = torch.full((n + off + GUARD,), float("nan"), dtype=F16, device=DEV)
        v = buf[off:off + n].view(t.shape)
        v.copy_(t.to(DEV, F16))
        return v

    def output(self, shape):
        off, n = GUARD + self.misalign, math.prod(shape)
        buf = torch.full((n + off + GUARD,), SENTINEL, dtype=F16, device=DEV)
        v = buf[off:off + n].view(shape)
        self.outs.append((buf, off, n, v))
        return v

    def workspace(self, nbytes):
        if not nbytes:
            return None
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=DEV)
        self.outs.append((ws, 0, ws.numel(), ws))
        return ws

    def poison(self):
        for buf, off, n, v in self.outs:
            if buf.dtype == torch.uint8:
                buf.fill_(0xFF)
            else:
                v.view(torch.int16).fill_(-1)   # 0xFFFF: NaN

    def check_guards(self, what):
        torch.cuda.synchronize()
        for buf, off, n, _ in self.outs:
            if buf.dtype != torch.uint8:
                assert (buf[:off] == SENTINEL).all() and (buf[off + n:] == SENTINEL).all(), f"{what}: output guard overwritten"


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


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


def _data(T, d_in, d_out, r, acc, r_acc, bias, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(F16)
    x = rnd(T, d_in)
    A = rnd(d_in, r, sc=1.0 / math.sqrt(d_in))
    B = rnd(r, d_out, sc=1.0 / math.sqrt(r))
    ad = au = None
    if acc == "dense":
        ad = rnd(d_in, d_out, sc=1.0 / math.sqrt(d_in))
    elif acc == "lowrank":
        ad, au = rnd(d_in, r_acc, sc=1.0 / math.sqrt(d_in)), rnd(r_acc, d_out, sc=1.0 / math.sqrt(r_acc))
    b = rnd(d_out) if bias else None
    dy = rnd(T, d_out)
    return x, A, B, ad, au, b, dy


def _kind(acc):
    return {"none": _lib.ACC_NONE, "lowrank": _lib.ACC_LOWRANK, "dense": _lib.ACC_DENSE}[acc]


def _run_layer(T, d_in, d_out, r, acc="none", r_acc=0, bias=True, save_h=True, misalign=0, scale=0.75, bwd=True, seed=0):
    lib = _lib.load()
    x, A, B, ad, au, b, dy = _data(T, d_in, d_out, r, acc, r_acc, bias, seed)
    kind = _kind(acc)
    ar = Arena(misalign)
    xv, Av, Bv, adv, auv, bv, dyv = (ar.input(t) for t in (x, A, B, ad, au, b, dy))
    y = ar.output((T, d_out))
    hcols = 64 if r <= 64 else r
    need_h = save_h or bwd or r > 64 or kind == _lib.ACC_DENSE
    h = ar.output((T, hcols)) if need_h else None
    ws = ar.workspace(lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, kind, _lib.F16))
    ar.poison()
    rc = lib.sow_forward(_p(xv), _p(Av), _p(Bv), _p(adv), _p(auv), _p(bv), _p(y), _p(h), T, d_in, d_out, r, r_acc, kind,
                         scale, _lib.F16, _p(ws), 0 if ws is None else ws.numel(), _s())
    assert rc == 0, lib.sow_error_string(rc)
    out = dict(y=y, h=h)
    if bwd:
        dx, dA, dB = ar.output((T, d_in)), ar.output((d_in, r)), ar.output((r, d_out))
        db = ar.output((d_out,)) if bias else None
        rc = lib.sow_backward(_p(dyv), _p(xv), _p(h), _p(Av), _p(Bv), _p(adv), _p(auv), _p(dx), _p(dA), _p(dB), _p(db), T, d_in,
                              d_out, r, r_acc, kind, scale, 0.0, _lib.F16, _p(ws), ws.numel(), _s())
        assert rc == 0, lib.sow_error_string(rc)
        out.update(dx=dx, dA=dA, dB=dB, db=db)
    ar.check_guards(f"T={T} {d_in}->{d_out} r={r} acc={acc}")
    return (x, A, B, ad, au, b, dy), out


def _check_layer(data, out, r, acc, scale, bwd, y_once):
    x, A, B, ad, au, b, dy = (None if t is None else t.double() for t in data)
    T = x.shape[0]
    h = out["h"]
    hk = None
    if h is not None and r <= 64 and acc != "dense_noh":
        hk = h.detach().cpu().double()
        check_once(hk[:, :r], scale * (x @ A), "h_save", scale * fp32_floor(x, A))
        if r < 63:
            assert (hk[:, r:63] == 0).all(), "h_save padding"
        if r <= 63:
            assert (hk[:, 63] == 1).all(), "h_save column 63"
    elif h is not None and r > 64:
        hk = h.detach().cpu().double()   # x . A unscaled, [T, r]
        check_once(hk, x @ A, "h (r > 64)", fp32_floor(x, A))
    hl = hk[:, :r] if (hk is not None and r <= 64) else (scale * hk if hk is not None else scale * rne16(x @ A))
    bias64 = b
    if acc == "none":
        if y_once:
            ref = hl @ B + (0 if bias64 is None else bias64)
            check_once(out["y"], ref, "y", fp32_floor(hl, B))
        else:
            check_bound16(out["y"], hl, B, "y", bias64)
    else:
        # accumulator term x W (dense) or (x Q) R (low-rank) + h B, rounded once or twice by the path: the bound form
        # (low-rank: the hidden x Q is an f16 operand, taken as RNE_f16 of its fp64 value)
        xa = torch.cat([x, hl], 1) if acc == "dense" else torch.cat([rne16(x @ ad), hl], 1)
        wa = torch.cat([ad, B], 0) if acc == "dense" else torch.cat([au, B], 0)
        first = x @ ad if acc == "dense" else rne16(x @ ad) @ au
        check_bound16(out["y"], xa, wa, "y", bias64, extra=ulp16(first))
    if not bwd:
        return
    dh = scale * (dy @ B.T)
    dB_ref_a, dB_ref_b = hl.T, dy
    if acc == "none":
        check_once(out["dB"], dB_ref_a @ dB_ref_b, "dB", fp32_floor(dB_ref_a, dB_ref_b))
    else:
        check_bound16(out["dB"], dB_ref_a, dB_ref_b, "dB")
    check_bound16(out["dA"], x.T, dh, "dA")
    if out["db"] is not None:
        check_bound16(out["db"], torch.ones(1, T, dtype=torch.float64), dy, "dbias")
    if acc == "none":
        check_bound16(out["dx"], dh, A.T, "dX")
    elif acc == "dense":
        check_bound16(out["dx"], torch.cat([dy, dh], 1), torch.cat([ad.T, A.T], 0), "dX", extra=ulp16(dy @ ad.T))
    else:
        t = rne16(dy @ au.T)
        check_bound16(out["dx"], torch.cat([t, dh], 1), torch.cat([ad.T, A.T], 0), "dX", extra=ulp16(t @ ad.T))


FWD_CASES = [
    # (T, d_in, d_out, r, acc, r_acc, bias, save_h)
    (32768, 512, 512, 50, "none", 0, True, True),
    (32768, 768, 768, 64, "none", 0, False, True),
    (4100, 512, 1376, 8, "none", 0, True, True),
    (4100, 1376, 512, 50, "none", 0, True, False),
    (4100, 2100, 2056, 50, "none", 0, True, True),
    (63, 512, 512, 50, "none", 0, True, True),
    (64, 768, 768, 8, "none", 0, False, True),
    (1, 512, 1376, 50, "none", 0, True, True),
    (4100, 512, 512, 96, "none", 0, True, True),
    (32768, 512, 512, 50, "dense", 0, True, True),
    (32768, 512, 1376, 50, "dense", 0, False, True),
    (4100, 768, 768, 64, "dense", 0, True, True),
    (63, 512, 512, 8, "dense", 0, True, True),
    (4100, 512, 512, 50, "lowrank", 50, True, True),
    (4100, 512, 512, 50, "lowrank", 96, True, True),
    (64, 768, 768, 50, "lowrank", 64, False, True),
]


@pytest.mark.parametrize("generic", [False, True], ids=["default", "generic"])
@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: f"T{c[0]}_{c[1]}x{c[2]}_r{c[3]}_{c[4]}{c[5] or ''}"
                         f"{'_bias' if c[6] else ''}{'' if c[7] else '_noh'}")
def test_f16_layer_against_fp64(case, generic, switches):
    T, d_in, d_out, r, acc, r_acc, bias, save_h = case
    if generic:
        switches("FORCE_CHAIN_V1", 1)
        switches("GEMM4", 0)
    scale = 0.75
    data, out = _run_layer(T, d_in, d_out, r, acc, r_acc, bias, save_h=save_h, scale=scale, bwd=save_h)
    # y rounds once: no accumulator at r <= 64 (chain / short split / generic chain from h), or the r > 64 composition
    # without h_save the test cannot see the H the kernel multiplied: the bound form
    _check_layer(data, out, r, acc, scale, bwd=save_h, y_once=(acc == "none" and save_h))


@pytest.mark.parametrize("acc", ["none", "dense"])
def test_f16_layer_misaligned(acc):
    data, out = _run_layer(300, 520, 264, 10, acc, 0, True, misalign=1, scale=0.5)
    _check_layer(data, out, 10, acc, 0.5, bwd=True, y_once=(acc == "none"))


def test_f16_results_do_not_depend_on_poison():
    _, a = _run_layer(4100, 512, 512, 50, "dense", 0, True, scale=0.5)
    _, b = _run_layer(4100, 512, 512, 50, "dense", 0, True, scale=0.5)
    for k in ("y", "h", "dx", "dA", "dB", "db"):
        assert torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)), k


def test_f16_overflow_becomes_inf():
    """|y| past 65504: +-inf where RNE_f16 of the fp64 product is +-inf (IEEE rounding, no saturation)."""
    T, d, r = 4096, 512, 16
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(T, d, generator=g) * 4).to(F16)
    A = (torch.randn(d, r, generator=g) * 2).to(F16)
    B = (torch.randn(r, d, generator=g) * 64).to(F16)
    from sow_amd import ops
    y, h = ops.sow_forward(x.to(DEV), A.to(DEV), B.to(DEV), None, None, None, 1.0)
    hk = h.view(T, 64)[:, :r].cpu().double()
    assert torch.isfinite(hk).all()
    ref = rne16(hk @ B.double())
    yk = y.cpu().double()
    assert torch.isinf(ref).any() and torch.isfinite(ref).any()
    assert torch.equal(torch.isinf(yk) & (yk > 0), torch.isinf(ref) & (ref > 0))
    assert torch.equal(torch.isinf(yk) & (yk < 0), torch.isinf(ref) & (ref < 0))


def test_f16_grouped_calls_are_bit_identical_to_single_calls():
    from sow_amd import ops
    T, d, r = 16384, 512, 32
    g = torch.Generator().manual_seed(5)
    mk = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(F16).to(DEV)
    x = mk(T, d)
    layers = [(mk(d, r, sc=0.05), mk(r, d, sc=0.2), mk(d)) for _ in range(3)]
    dy = [mk(T, d) for _ in range(3)]
    single = []
    for (A, B, b), g_ in zip(layers, dy):
        y, h = ops.sow_forward(x, A, B, None, None, b, 0.5)
        single.append((y, h) + tuple(ops.sow_backward(g_, x, h, A, B, None, None, 0.5, True)))
    outs = [(torch.empty_like(A), torch.empty_like(B), torch.empty_like(b)) for A, B, b in layers]
    calls = [ops.LayerCall(x, A, B, bias=b, scale=0.5, dy2=g_, dx=torch.empty_like(x), out=o)
             for (A, B, b), g_, o in zip(layers, dy, outs)]
    grp = ops.LayerGroup(calls)
    grp.forward()
    grp.backward()
    torch.cuda.synchronize()
    for c, o, s in zip(calls, outs, single):
        y, h, dx, dA, dB, db = s
        assert torch.equal(c.y, y) and torch.equal(c.h, h) and torch.equal(c.dx, dx)
        assert torch.equal(o[0], dA) and torch.equal(o[1], dB) and torch.equal(o[2], db)


@pytest.mark.parametrize("shape", [(32768, 512, 1376, False), (4096, 768, 768, True), (300, 264, 520, False),
                                   (1024, 1024, 2048, False)])
def test_f16_gemm_against_fp64(shape):
    from sow_amd import ops
    M, K, N, tb = shape
    g = torch.Generator().manual_seed(7)
    A = (torch.randn(M, K, generator=g)).to(F16)
    B = (torch.randn(N, K, generator=g) if tb else torch.randn(K, N, generator=g)).to(F16) / math.sqrt(K)
    bias = torch.randn(N, generator=g).to(F16)
    C = ops.gemm(A.to(DEV), B.to(DEV), trans_b=tb, bias=bias.to(DEV))
    Bm = B.double().T if tb else B.double()
    check_once(C, A.double() @ Bm + bias.double(), f"gemm {shape}", fp32_floor(A.double(), Bm))


def test_f16_qr_thin_matches_fp32_output():
    from sow_amd import ops
    g = torch.Generator().manual_seed(11)
    W = (torch.randn(512, 96, generator=g) * 0.02).to(F16).to(DEV)
    Q16, R16 = ops.qr_thin(W, 50)
    Q32, R32 = ops.qr_thin(W, 50, out_dtype=torch.float32)
    assert Q16.dtype == F16 and R16.dtype == F16
    q = Q16.cpu().double()
    ref = rne16(Q32.cpu().double())
    assert ((q - ref).abs() <= ulp16(ref)).all()
    r = R16.cpu().double()
    rref = rne16(R32.cpu().double())
    assert ((r - rref).abs() <= ulp16(rref)).all()


@pytest.mark.parametrize("init", ["normal_QR", "normal"])
def test_f16_accumulate_model_batched_equals_per_layer(init):
    """accumulate(model) (batched: one sow_accumulate_batch call) against SoWLinear.accumulate() layer by layer on an identical
    f16 copy with the same draws (as test_gpu_configs.py does for fp32 / bf16); the per-layer path composes torch ops, so
    the two agree to f16 rounding, not bit for bit."""
    import copy

    import torch.nn as nn

    from sow_amd import SoWLinear, accumulate
    torch.manual_seed(3)
    shapes = [(512, 512), (512, 1376), (1376, 512), (200, 264)]
    net = nn.ModuleList([SoWLinear(i, o, bias=False, rank=r, scale=0.5, init_method="normal", device=DEV, dtype=F16)
                         for (i, o), r in zip(shapes, (50, 50, 50, 34))])
    for m in net:
        m.init_method = init
        m.virtual_rank = min(m.in_features, m.out_features)          # what prepare_sow sets
    ref = copy.deepcopy(net)
    gen = torch.Generator().manual_seed(5)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))
    for call in range(2):
        for m, mr in zip(net, ref):
            b = (torch.randn(m.rank, m.out_features, generator=gen) * 0.1).to(DEV, F16)
            m.upscale_weights[0].data.copy_(b)
            mr.upscale_weights[0].data.copy_(b)
            shape = (m.in_features, m.out_features) if init == "normal_QR" else (m.in_features, m.rank)
            ds = [torch.randn(*shape, generator=gen) * 0.02]
            for mod in (m, mr):
                mod._fresh_gaussian = lambda shape, device, dtype_, _it=iter(ds): next(_it).to(device, dtype_)
        accumulate(net)
        for mr in ref:
            mr.accumulate()
        torch.cuda.synchronize()
        for m, mr in zip(net, ref):
            assert m.acc_downweight.dtype == F16 and tuple(m.acc_downweight.shape) == (m.in_features, m.out_features)
            assert torch.isfinite(m.acc_downweight).all()
            assert rel(m.acc_downweight.cpu(), mr.acc_downweight.cpu()) < 5e-3, (call, m.in_features)
            assert rel(m.downscale_weights[0].data.cpu(), mr.downscale_weights[0].data.cpu()) < 5e-3
            assert float(m.upscale_weights[0].data.abs().max()) == 0.0


def test_f16_sowlinear_training_step():
    from sow_amd import SoWLinear
    torch.manual_seed(0)
    layer = SoWLinear(512, 512, bias=True, rank=50, scale=0.5, init_method="normal", device=DEV, dtype=F16)
    x = torch.randn(8, 512, 512, device=DEV, dtype=F16, requires_grad=True)
    y = layer(x)
    y.float().square().mean().backward()
    assert y.dtype == F16 and torch.isfinite(y).all() and torch.isfinite(x.grad).all()
    assert torch.isfinite(layer.downscale_weights[0].grad).all() and torch.isfinite(layer.bias.grad).all()
    layer.accumulate()
    with torch.no_grad():
        y2 = layer(x)
    assert torch.isfinite(y2).all()


def test_reference_evaluation_protocol_half():
    """commonsense_evaluate.py:268-287: prepare_sow -> load_state_dict(assign=True) -> .to(cuda) -> .half() -> .eval() -> no-grad."""
    transformers = pytest.importorskip("transformers")
    from safetensors.torch import load_file

    from sow_amd import SoWConfig, prepare_sow
    golden = os.path.join(ROOT, "tests", "golden")

    def tiny():
        torch.manual_seed(42)
        cfg = transformers.LlamaConfig(hidden_size=64, intermediate_size=176, num_hidden_layers=2, num_attention_heads=4,
                                       num_key_value_heads=4, vocab_size=256, max_position_embeddings=64, rms_norm_eps=1e-6,
                                       tie_word_embeddings=False, attn_implementation="eager")
        model = transformers.AutoModelForCausalLM.from_config(cfg)
        return prepare_sow(model, SoWConfig(target_modules=["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj",
                                                            "down_proj"], rank=6, init_method="normal", scale=1.0,
                                            decompose="keep", device="cpu"))
    import numpy as np
    g = np.load(os.path.join(golden, "load_sow.npz"))
    tokens = torch.from_numpy(g["tokens"]).to(DEV)
    saved = load_file(os.path.join(golden, "load_sow_checkpoint.safetensors"))
    m32 = tiny()
    m32.load_state_dict(saved, assign=True, strict=False)
    m32.to(DEV).eval()
    m16 = tiny()
    m16.load_state_dict(saved, assign=True, strict=False)
    m16.to(DEV)
    m16.half()
    m16.eval()
    with torch.no_grad():
        out16 = m16(input_ids=tokens[3], labels=tokens[3].clone())
        out32 = m32(input_ids=tokens[3], labels=tokens[3].clone())
    loss = float(out16.loss)
    ref = float(g["assign_loss"])
    assert abs(loss - ref) < 5e-3 * abs(ref), (loss, ref)
    l16, l32 = out16.logits.double(), out32.logits.double()
    rel = float((l16 - l32).norm() / l32.norm())
    assert rel < 5e-3, rel
