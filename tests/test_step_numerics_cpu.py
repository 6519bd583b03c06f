"""The checks of tests/step_numerics.py and the float16 helpers of tests/numerics.py, tested on the CPU (no `gpu` mark), in
the pattern of test_numerics_cpu.py.

Each kernel is emulated in float32 in its own operation order (adamw_flat_kernel, ttadam_dense_kernel, the rank update of
accumulate.hip; Householder QR by fp32 LAPACK, torch.linalg.qr): the emulation has to pass its check with margin (worst
err / limit <= 0.7, and at most a tenth of the allowed inexact elements of a 16-bit output).  A fault catalogue has to be
rejected, and each fault records whether today's max-norm `rel_err` tolerance would have passed it.
"""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err
from numerics import F16_MAX, MAX_INEXACT, UNIT_ROUNDOFF, NumericsError, check_rounded, rne, ulp
from step_numerics import (U32, adamw_ref, check_qr, check_rank_update, check_step, lapack_q, rank_update_ref,
                           ttadam_ref)

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
MARGIN = 0.7
PAIRS = [(F32, F32), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32)]


def _np_f16(d):
    return torch.from_numpy(d.numpy().astype(np.float16).astype(np.float64))


# ---- float16 in numerics.py -------------------------------------------------------------------------------------------
def test_f16_ulp_and_rne_match_torch():
    assert ulp(torch.tensor([1.0, 3.0, 2.0 ** -14, 2.0 ** -20, 0.0, 65504.0]), F16).tolist() == \
        [2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 32.0]
    g = torch.Generator().manual_seed(5)
    d = torch.cat([torch.randn(200000, generator=g, dtype=torch.float64) * s for s in (1e-6, 1e-3, 1.0, 1e3, 3e4)])
    # numpy's float64 -> float16 cast rounds once (to nearest even), subnormals and overflow included (torch's goes
    # through fp32 and can round twice)
    assert torch.equal(rne(d, F16), _np_f16(d))
    edge = torch.tensor([65519.996, 65520.0, -65520.0, 65504.0 + 15.999, 2.0 ** -25, 2.0 ** -25 * 1.0001, 3 * 2.0 ** -25],
                        dtype=torch.float64)
    assert rne(edge, F16).tolist() == [65504.0, math.inf, -math.inf, 65504.0, 0.0, 2.0 ** -24, 2.0 ** -23]
    assert torch.equal(rne(edge, F16), _np_f16(edge))
    assert F16_MAX == float(torch.finfo(F16).max)
    # every f16 bit pattern: a finite value is its own RNE and one ulp from its neighbour
    allv = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(F16).double()
    fin = allv[torch.isfinite(allv)]
    assert torch.equal(rne(fin, F16), fin)
    assert UNIT_ROUNDOFF[F16] == 2.0 ** -11


def test_check_rounded_accepts_equal_infinities():
    ref = torch.tensor([70000.0, -1e6, 1.0], dtype=torch.float64)
    out = torch.tensor([math.inf, -math.inf, 1.0])
    check_rounded(out, ref, F16, name="inf")
    with pytest.raises(NumericsError):
        check_rounded(torch.tensor([65504.0, -math.inf, 1.0]), ref, F16, name="saturated")


# ---- emulations ------------------------------------------------------------------------------------------------------
def _f(x):
    """A Python scalar rounded to fp32 once."""
    return torch.tensor(x, dtype=torch.float64).float()


def store(x32, dtype, rtz=False):
    """An fp32 tensor stored in `dtype`: RNE (torch's cast), or rounded toward zero (the fault); float64 out."""
    if dtype == F32:
        return x32.double()
    if not rtz:
        return x32.to(dtype).double()
    x = x32.double()
    q = ulp(x, dtype)
    return torch.sign(x) * torch.floor(x.abs() / q) * q


def adamw_emulate(p, g, m, v, pdtype, sdtype, *, lr, betas, eps, wd, step, grad_scale, fault=None):
    """adamw_flat_kernel in fp32, its operation order, the host scalars formed in double; `fault` one of FAULTS' names."""
    b1, b2 = betas
    if fault == "betas_fp32":          # the kernel before this change: 1 - b and the corrections in fp32 of fp32 betas
        b1f, b2f = _f(b1), _f(b2)
        c1, c2 = 1.0 - b1f, 1.0 - b2f
        bc1 = 1.0 - b1f ** step
        bc2s = torch.sqrt(1.0 - b2f ** step)
        step_size = _f(lr) / bc1
    else:
        st = step + 1 if fault == "bias_step_off" else step
        b1f, b2f, c1, c2 = _f(b1), _f(b2), _f(1.0 - b1), _f(1.0 - b2)
        bc1 = 1.0 - b1 ** st
        bc2s = _f(math.sqrt(1.0 - b2 ** st))
        step_size = _f(lr / bc1)
    decay = _f(1.0 - lr * wd)
    gs = {"grad_scale_dropped": 1.0, "grad_scale_twice": grad_scale * grad_scale}.get(fault, grad_scale)
    P, M, V = p.float(), m.float(), v.float()
    G = g.float() * _f(gs)
    if fault != "wd_after_update":
        P = P * decay
    M = b1f * M + c1 * G
    V = b2f * V + c2 * G * G
    denom = torch.sqrt(V + _f(eps)) / bc2s if fault == "eps_in_sqrt" else torch.sqrt(V) / bc2s + _f(eps)
    P = P - step_size * (M / denom)
    if fault == "wd_after_update":
        P = P * decay
    return dict(p=store(P, pdtype, fault == "rtz_p"), m=store(M, sdtype, fault == "rtz_m"),
                v=store(V, sdtype, fault == "rtz_v"))


def ttadam_emulate(p, g, m, v, *, betas, eps, step_size, lr_wd, clamp_v, fault=None):
    """ttadam_dense_kernel in fp32 (its order: m * b1 + g * c1, v * b2 + g * g * c2, p + (m / (sqrt(v) + eps)) * -step_size,
    p + p * -lr_wd)."""
    b1, b2 = betas
    b1f, b2f = _f(b1), _f(b2)
    c1, c2 = (1.0 - b1f, 1.0 - b2f) if fault == "betas_fp32" else (_f(1.0 - b1), _f(1.0 - b2))
    P, G, M, V = p.float(), g.float(), m.float(), v.float()
    if clamp_v and fault != "no_clamp":
        V = V.clamp(min=0.0)
    M = M * b1f + G * c1
    V = V * b2f + G * G * c2
    P = P + (M / (torch.sqrt(V) + _f(eps))) * (-_f(step_size))
    if lr_wd > 0:
        P = P + P * (-_f(lr_wd))
    return dict(p=P.double(), m=M.double(), v=V.double())


def rank_update_emulate(acc, A, B, scale, beta, dtype, fault=None):
    """rank_update_batch_kernel: c = sequential fp32 fmas over k, val = scale * c (+ beta * acc), one store."""
    A64, B64 = A.double(), B.double()
    c = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float32)
    for k in range(A.shape[1]):
        c = (A64[:, k:k + 1] * B64[k:k + 1, :] + c.double()).float()      # fma: exact product, one rounding
    val = _f(scale) * c
    if beta != 0:
        val = val + _f(beta) * acc.float()
    return store(val, dtype, fault == "rtz_acc")


def _step_data(n, pdtype, sdtype, step, seed, kind="mixed"):
    g = torch.Generator().manual_seed(seed)
    p = (torch.randn(n, generator=g, dtype=torch.float64) * 0.05).to(pdtype)
    gr = torch.randn(n, generator=g, dtype=torch.float64) * 1e-2
    if kind == "mixed":       # thirds: zeros, tiny g (sqrt(v) near eps), large g
        t = n // 3
        gr[:t // 4] = 0.0
        gr[t:2 * t] *= 1e-6
        gr[2 * t:] *= 1e4 if pdtype != F16 else 1e3
    gr = gr.to(pdtype)
    if step == 1:
        m = torch.zeros(n, dtype=sdtype)
        v = torch.zeros(n, dtype=sdtype)
    else:
        m = (torch.randn(n, generator=g, dtype=torch.float64) * 1e-3).to(sdtype)
        v = (torch.rand(n, generator=g, dtype=torch.float64) * 1e-4).to(sdtype)
    return p, gr, m, v


HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.1, step=1, grad_scale=0.5)


@pytest.mark.parametrize("pdtype,sdtype", PAIRS)
@pytest.mark.parametrize("betas,step,wd,gs", [((0.9, 0.999), 1, 0.1, 0.5), ((0.9, 0.95), 2, 0.0, 1.0),
                                              ((0.9, 0.999), 10, 0.1, 1.0), ((0.9, 0.999), 1000, 0.1, 0.5)])
def test_adamw_emulation_passes_with_margin(pdtype, sdtype, betas, step, wd, gs):
    hp = dict(HP, betas=betas, step=step, wd=wd, grad_scale=gs)
    p, g, m, v = _step_data(30011, pdtype, sdtype, step, seed=step)
    out = adamw_emulate(p, g, m, v, pdtype, sdtype, **hp)
    refs, mags = adamw_ref(p, g, m, v, **hp)
    st = check_step(out, refs, mags, pdtype, sdtype, "adamw")
    _assert_margin(st, (pdtype, sdtype, betas, step))


def _assert_margin(st, what):
    """fp32 outputs: worst err / bound <= MARGIN; 16-bit outputs: inexact share <= MAX_INEXACT / 10."""
    summary = {k: (round(s["worst"], 3), round(100 * s.get("inexact", 0.0), 4)) for k, s in st.items()}
    print(f"{what}: worst err/limit, inexact % {summary}")
    for k, s in st.items():
        if "inexact" in s:
            assert s["inexact"] <= MAX_INEXACT / 10, (k, s)
        else:
            assert s["worst"] <= MARGIN, (k, s)


@pytest.mark.parametrize("clamp_v,wd", [(True, 0.0), (True, 0.01), (False, 0.01)])
def test_ttadam_emulation_passes_with_margin(clamp_v, wd):
    p, g, m, v = _step_data(20011, F32, F32, 3, seed=11)
    if clamp_v:
        v[::7] = -v[::7]                                   # negative moments left by a lossy TT re-compression
    lr, betas, step = 1e-2, (0.9, 0.999), 3
    step_size = float(_f(lr * math.sqrt(1 - betas[1] ** step) / (1 - betas[0] ** step)))
    lr_wd = float(_f(lr * wd))
    kw = dict(betas=betas, eps=1e-8, step_size=step_size, lr_wd=lr_wd, clamp_v=clamp_v)
    refs, mags = ttadam_ref(p, g, m, v, **kw)
    st = check_step(ttadam_emulate(p, g, m, v, **kw), refs, mags, F32, F32, "ttadam")
    _assert_margin(st, ("ttadam", clamp_v, wd))


def _rank_data(d_in, d_out, r, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(d_in, r, generator=g) * 0.05).to(dtype)
    B = (torch.randn(r, d_out, generator=g) * 0.05).to(dtype)
    acc = (torch.randn(d_in, d_out, generator=g) * 0.01).to(dtype)
    return acc, A, B


@pytest.mark.parametrize("dtype", [BF16, F16, F32])
@pytest.mark.parametrize("d_in,d_out,r,beta", [(259, 100, 7, 1.0), (1001, 512, 64, 1.0), (100, 259, 1, 0.0),
                                               (512, 1001, 50, 0.0)])
def test_rank_update_emulation_passes_with_margin(dtype, d_in, d_out, r, beta):
    acc, A, B = _rank_data(d_in, d_out, r, dtype, seed=r)
    out = rank_update_emulate(acc, A, B, 0.75, beta, dtype)
    st = check_rank_update(out, acc, A, B, 0.75, beta, dtype)
    _assert_margin({"acc": st}, (dtype, d_in, d_out, r, beta))


@pytest.mark.parametrize("m,n,k", [(512, 512, 512), (1376, 512, 512), (512, 1376, 512), (1001, 1001, 1001),
                                   (1001, 300, 600), (1001, 600, 300), (259, 100, 50)])
@pytest.mark.parametrize("out_dtype", [F32, BF16])
def test_qr_emulation_passes_with_margin(m, n, k, out_dtype):
    W = torch.randn(m, n, generator=torch.Generator().manual_seed(m + n))
    Q, R = _qr32(W, k)
    kc = min(m, n, k)
    R[:, kc:] = (Q.double().t() @ W[:, kc:].double()).float()     # the tail by an fp32-exact GEMM of the fp32 Q
    st = check_qr(W, Q.to(out_dtype), R.to(out_dtype), k, out_dtype)
    print(f"QR {m}x{n} k={k} -> {out_dtype}: " + ", ".join(f"{key} {s['worst']:.3g}" for key, s in st.items()))
    # a 16-bit Q and R add the hard bound 2 u_out |Q| |R| of their own rounding (check_qr), which a few terms can nearly
    # reach: the margin applies to the fp32 outputs, the 16-bit ones stay under the bound
    assert max(s["worst"] for s in st.values()) <= (MARGIN if out_dtype == F32 else 1.0), st


def _qr32(W, k):
    """fp32 LAPACK Q[:, :k], R[:k, :] (complete mode when k > min(m, n): R rows >= n are 0)."""
    m, n = W.shape
    Q, R = torch.linalg.qr(W.float(), mode="complete" if k > min(m, n) else "reduced")
    return Q[:, :k].contiguous(), R[:k].contiguous()


# ---- Householder QR with faults (float64, geqr2 + org2r as qr_panel.hpp) ----------------------------------------------
def householder(W, k, skip=None):
    """geqr2 + org2r in float64 with LAPACK's slarfg convention; skip: the index of one reflector left out of Q."""
    A = W.double().clone()
    m, n = A.shape
    kc = min(m, n, k)
    vs, taus = [], []
    for j in range(kc):
        x = A[j:, j].clone()
        alpha, xn = float(x[0]), float(x[1:].norm())
        if xn == 0:
            vs.append(None), taus.append(0.0)
            continue
        beta = -math.copysign(math.hypot(alpha, xn), alpha if alpha != 0 else 1.0)
        tau = (beta - alpha) / beta
        v = x / (alpha - beta)
        v[0] = 1.0
        A[j:, j:] -= tau * torch.outer(v, v @ A[j:, j:])
        vs.append(v), taus.append(tau)
    Q = torch.eye(m, k, dtype=torch.float64)
    for j in reversed(range(kc)):
        if vs[j] is None or j == skip:
            continue
        Q[j:] -= taus[j] * torch.outer(vs[j], vs[j] @ Q[j:])
    R = torch.triu(A)[:k]
    return Q, R


def _qr_fault(kind):
    m, n, k = 300, 200, 64
    W = torch.randn(m, n, generator=torch.Generator().manual_seed(77)).float()
    Q, R = householder(W, k, skip=5 if kind == "skip" else None)
    if kind == "sign":
        Q[:, 9], R[9] = -Q[:, 9], -R[9]
    if kind == "tail":
        R[:, k:] = Q.t() @ W[:, k - 1:n - 1].double()        # the tail from the columns one to the left
        return R, Q.t() @ W.double(), lambda o: check_qr(W, Q, o, k, F32)
    R[:, k:] = Q.t() @ W[:, k:].double()
    return Q, lapack_q(W, k), lambda o: check_qr(W, o, R, k, F32)


# ---- fault catalogue ------------------------------------------------------------------------------------------------
def _adamw_fault(fault, pdtype, sdtype, betas=(0.9, 0.999), step=1, kind="mixed", out="p"):
    hp = dict(HP, betas=betas, step=step)
    p, g, m, v = _step_data(30011, pdtype, sdtype, step, seed=3, kind=kind)
    bad = adamw_emulate(p, g, m, v, pdtype, sdtype, fault=fault, **hp)
    refs, mags = adamw_ref(p, g, m, v, **hp)
    # rel_err of today's tests looks at p (and at the fp32 state at beta2 = 0.95)
    return bad[out], refs[out], lambda o: check_step(dict(bad, **{out: o}), refs, mags, pdtype, sdtype, "adamw")


def _ttadam_fault(fault):
    p, g, m, v = _step_data(20011, F32, F32, 3, seed=12)
    v[::5] = -v[::5]
    kw = dict(betas=(0.9, 0.999), eps=1e-8, step_size=1e-3, lr_wd=float(_f(1e-4)), clamp_v=True)
    bad = ttadam_emulate(p, g, m, v, fault=fault, **kw)
    refs, mags = ttadam_ref(p, g, m, v, **kw)
    out = "p"
    return bad[out], refs[out], lambda o: check_step(dict(bad, **{out: o}), refs, mags, F32, F32, "ttadam")


def _rank_fault():
    acc, A, B = _rank_data(512, 259, 50, BF16, seed=5)
    bad = rank_update_emulate(acc, A, B, 0.75, 1.0, BF16, fault="rtz_acc")
    return bad, rank_update_ref(acc, A, B, 0.75, 1.0), lambda o: check_rank_update(o, acc, A, B, 0.75, 1.0, BF16)


# id -> (builder, rel_err tolerance of today's tests, would rel_err have passed it)
FAULTS = {
    "adamw_beta_complements_from_fp32_betas": (lambda: _adamw_fault("betas_fp32", F32, F32), 1e-5, True),
    "adamw_bias_correction_one_step_off": (lambda: _adamw_fault("bias_step_off", F32, F32, step=10), 1e-5, False),
    "adamw_weight_decay_after_update": (lambda: _adamw_fault("wd_after_update", F32, F32), 1e-5, True),
    "adamw_eps_inside_sqrt": (lambda: _adamw_fault("eps_in_sqrt", F32, F32), 1e-5, False),
    "adamw_grad_scale_dropped": (lambda: _adamw_fault("grad_scale_dropped", F32, F32, step=10), 1e-5, False),
    "adamw_grad_scale_twice": (lambda: _adamw_fault("grad_scale_twice", F32, F32, step=10), 1e-5, False),
    "adamw_bf16_p_stored_toward_zero": (lambda: _adamw_fault("rtz_p", BF16, F32), 1e-2, True),
    "adamw_f16_p_stored_toward_zero": (lambda: _adamw_fault("rtz_p", F16, F32), 1e-2, True),
    "adamw_bf16_m_stored_toward_zero": (lambda: _adamw_fault("rtz_m", BF16, BF16, out="m"), 1e-2, True),
    "adamw_f16_v_stored_toward_zero": (lambda: _adamw_fault("rtz_v", F16, F16, out="v", kind="plain"), 1e-2, False),
    "ttadam_beta_complements_from_fp32_betas": (lambda: _ttadam_fault("betas_fp32"), 1e-4, True),
    "ttadam_negative_v_not_clamped": (lambda: _ttadam_fault("no_clamp"), 1e-4, False),
    "rank_update_bf16_stored_toward_zero": (_rank_fault, 2e-2, True),
    "qr_one_reflector_skipped": (lambda: _qr_fault("skip"), 1e-4, False),
    "qr_one_column_sign_flipped": (lambda: _qr_fault("sign"), 1e-4, False),
    "qr_r_tail_from_wrong_columns": (lambda: _qr_fault("tail"), 1e-4, False),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_fault_is_rejected(fault):
    build, tol, rel_err_blind = FAULTS[fault]
    out, ref, check = build()
    with pytest.raises(NumericsError) as e:
        check(out)
    err = rel_err(out.float(), ref.float()) if not torch.isnan(out).any() else math.inf
    passes_rel_err = err < tol
    print(f"fault {fault}: rejected ({str(e.value)[:160]}); rel_err {err:.3g} "
          f"{'PASSES' if passes_rel_err else 'fails'} today's {tol:g}")
    assert passes_rel_err == rel_err_blind, (fault, err)
