"""float64 references and element-wise checks of the kernels that write the model's weights and optimizer state
(sow_adamw_flat, sow_ttadam_dense, sow_accumulate_batch, sow_qr_thin): a plain module next to numerics.py, imported by
test_step_numerics_cpu.py (which runs fp32 emulations and a fault catalogue through the checks) and by
test_gpu_step_elementwise.py (which runs the kernels through them).

Every reference is float64 arithmetic on the exact values the kernel read, with the hyperparameters as Python doubles.
Every bound is one output ulp plus a multiple of the fp32 unit roundoff u = 2^-24 counted from the kernel's operations;
the counts are given at each bound.
"""
from __future__ import annotations

import math

import torch

from numerics import (MAX_INEXACT, UNIT_ROUNDOFF, NumericsError, _tail_note, bound, check_bound, check_rounded,
                      fp32_floor, rne, to64, ulp)

F32 = torch.float32
U32 = UNIT_ROUNDOFF[F32]

# AdamW (misc.hip adamw_flat_kernel), per element, every scalar 1 - b, 1 - lr*wd, lr/bc1, sqrt(bc2) formed in double and
# rounded to fp32 once (u each), b1 and b2 rounded to fp32 (u each), grad_scale applied by one product (u):
#   m = b1*m + c1*g:         b1 or c1 (u) + its product (u) + g*grad_scale (u)             -> 3u of |b1 m| + |c1 g|
#   v = b2*v + c2*g*g:       b2 or c2 (u), two products (2u), g*grad_scale squared (2u)    -> 5u of v (every term >= 0)
#   denom = sqrt(v)/bc2s + eps: v (5u + its own rounding u) halved by sqrt (3u) + sqrt (u) + bc2s (u) + the division (u)
#                            + the sum with eps >= 0 (u)                                  -> 7u
#   step_size * (m / denom): m (3u + its rounding u), denom (7u), the division (u), step_size (u), the product (u) -> 14u
#                            of step_size * (|b1 m| + |c1 g|) / denom (the update without cancellation inside m)
#   p * (1 - lr*wd):         the factor (u) and the product (u)                           -> 2u of |p|
# The final sums round once more: one ulp of the result.  C_P = 14 covers 2u |p| + 14u |update|.
C_M, C_V, C_P = 3.0, 5.0, 14.0


def adamw_ref(p, g, m, v, *, lr, betas, eps, wd, step, grad_scale):
    """torch.optim.AdamW's step (single-tensor form, no amsgrad) in float64 on the exact stored values.  Returns the
    references of p, m, v and the magnitudes the bounds scale with."""
    b1, b2 = betas
    p, g, m, v = to64((p, g, m, v))
    g = g * grad_scale
    p1 = p * (1.0 - lr * wd)
    m_n = b1 * m + (1.0 - b1) * g
    v_n = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = v_n.sqrt() / math.sqrt(bc2) + eps
    step_size = lr / bc1
    p_n = p1 - step_size * (m_n / denom)
    m_abs = (b1 * m).abs() + ((1.0 - b1) * g).abs()
    upd_abs = step_size * m_abs / denom
    return dict(p=p_n, m=m_n, v=v_n), dict(p=p.abs() + upd_abs, m=m_abs, v=v_n.abs())


def ttadam_ref(p, g, m, v, *, betas, eps, step_size, lr_wd, clamp_v):
    """ttadam.py:84-111 in float64: v < 0 -> 0 (clamp_v), Adam moments with 1 - beta of the double betas, p -= step_size *
    m / (sqrt(v) + eps), then p += p * (-lr * wd).  step_size and lr_wd are the fp32 values the kernel was handed."""
    b1, b2 = betas
    p, g, m, v = to64((p, g, m, v))
    if clamp_v:
        v = v.clamp(min=0.0)
    m_n = b1 * m + (1.0 - b1) * g
    v_n = b2 * v + (1.0 - b2) * g * g
    denom = v_n.sqrt() + eps
    p1 = p - step_size * (m_n / denom)
    p_n = p1 + p1 * (-lr_wd) if lr_wd > 0 else p1
    m_abs = (b1 * m).abs() + ((1.0 - b1) * g).abs()
    upd_abs = step_size * m_abs / denom
    # the optional decay line adds a product and a sum (2u of |p1| lr_wd and |p1|): C_P covers it with the (1 + lr_wd)
    return dict(p=p_n, m=m_n, v=v_n), dict(p=(p.abs() + upd_abs) * (1.0 + lr_wd), m=m_abs, v=v_n.abs())


def check_rounded_noisy(out, ref, dtype, noise, name="out") -> dict:
    """A 16-bit output of an fp32 computation whose error against ref64 is at most `noise` (a rigorous bound): within one
    ulp of RNE(ref64) plus the noise everywhere (check_rounded), and bit-equal to RNE(ref64) wherever the noise interval
    [ref - noise, ref + noise] does not reach a rounding point of `dtype` -- in at most MAX_INEXACT of those elements.
    Elements whose interval holds a rounding point may round either way: the update m = b1 m + (1 - b1) g of 16-bit inputs
    lands exactly on a 16-bit tie whenever 9 m + g is a multiple of 5, and the kernel's fp32 b1 moves it off the tie."""
    st = check_rounded(out, ref, dtype, max_inexact=1.0, acc=noise, name=name)
    out64, ref64, noise = to64(out), to64(ref), to64(noise)
    decided = rne(ref64 - noise, dtype) == rne(ref64 + noise, dtype)
    miss = decided & (out64 != rne(ref64, dtype))
    st["inexact"] = float(miss.sum()) / max(1, miss.numel())
    st["undecided"] = float((~decided).sum()) / max(1, miss.numel())
    allowed = max(MAX_INEXACT * miss.numel(), 2)
    if int(miss.sum()) > allowed:
        raise NumericsError(f"{name}: {int(miss.sum())} of {miss.numel()} elements differ from RNE(ref64) although their "
                            f"fp32 noise cannot reach a rounding point, allowed {allowed:.0f} ({_tail_note(miss)})")
    return st


def check_step(out: dict, refs: dict, mags: dict, pdtype, sdtype, name: str) -> dict:
    """p (pdtype), m and v (sdtype) of one optimizer step against their float64 references: fp32 outputs within one ulp
    plus C u |magnitude| (check_bound), 16-bit outputs within one ulp of RNE(ref64) and bit-equal to it at all but a few
    (check_rounded_noisy, with the fp32 noise and the fp32 rounding before the 16-bit store as the noise)."""
    stats = {}
    for key, dt, c in (("p", pdtype, C_P), ("m", sdtype, C_M), ("v", sdtype, C_V)):
        noise = c * U32 * mags[key]
        if dt == F32:
            stats[key] = check_bound(out[key], refs[key], bound(refs[key], F32, noise), name=f"{name}.{key}")
        else:
            stats[key] = check_rounded_noisy(out[key], refs[key], dt, noise + ulp(refs[key], F32), name=f"{name}.{key}")
    return stats


# ---- rank update (accumulate.hip rank_update_batch_kernel) ----------------------------------------------------------
def rank_update_ref(acc, A, B, scale, beta):
    """acc_beta * acc + scale * A . B in float64; acc is not read when beta == 0 (it may hold NaN)."""
    A, B = to64((A, B))
    ref = scale * (A @ B)
    if beta != 0:
        ref = ref + beta * to64(acc)
    return ref


def rank_update_noise(acc, A, B, scale, beta):
    """The kernel sums the r products a_k b_k by sequential fp32 fmas (r roundings, each of a partial sum <= sum |a_k b_k|),
    multiplies by scale (one rounding) and adds beta * acc (one rounding of the product, one of the sum): the error is at most
    (r + 3) u (|scale| sum_k |a_k b_k| + |beta acc|) (Higham's gamma_n bound of recursive summation), plus one fp32 ulp of the
    result (its rounding before a 16-bit store)."""
    A, B = to64((A, B))
    mag = abs(scale) * (A.abs() @ B.abs())
    if beta != 0:
        mag = mag + abs(beta) * to64(acc).abs()
    return (A.shape[1] + 3) * U32 * mag


def check_rank_update(out, acc0, A, B, scale, beta, dtype, name="acc") -> dict:
    ref = rank_update_ref(acc0, A, B, scale, beta)
    noise = rank_update_noise(acc0, A, B, scale, beta)
    if dtype == F32:
        return check_bound(out, ref, bound(ref, F32, noise), name=name)
    return check_rounded_noisy(out, ref, dtype, noise + ulp(ref, F32), name=name)


# ---- Householder QR (qr_panel.hpp, qr.hip, the QR phase of accumulate.hip) ---------------------------------------------
# The panel reduces every column with fp32 dot products of length <= m and rank-1 updates: the normwise backward error of
# Householder QR is (Higham, Accuracy and Stability of Numerical Algorithms, Thm 19.4) a small multiple of m n u; measured
# on fp32 LAPACK (test_step_numerics_cpu.py) columnwise |W_j - (QR)_j| stays under 0.01 m u ||W_j|| and |Q^T Q - I| under
# 0.03 m u up to m = n = 1001.  The checks below use C_QR m u, C_QR = 1, i.e. at least 30x the measured error, while a
# skipped reflector or a wrong tail errs by O(1).
C_QR = 1.0


def lapack_q(W, k):
    """float64 Q[:, :k] of W in LAPACK's sign convention (torch.linalg.qr on the CPU is LAPACK geqrf / orgqr); complete
    mode when k exceeds min(m, n)."""
    W = to64(W)
    m, n = W.shape
    Q, _ = torch.linalg.qr(W, mode="complete" if k > min(m, n) else "reduced")
    return Q[:, :k]


def _condition(W):
    s = torch.linalg.svdvals(to64(W))
    return float(s[0] / s[-1]) if float(s[-1]) > 0 else math.inf


def check_orthonormal(Q, out_dtype, name="Q") -> dict:
    """|Q^T Q - I| per element within C_QR m u (fp32 panel) + 2 u_out (rounding of each Q element to out_dtype: |dQ^T Q +
    Q^T dQ| <= 2 u_out |q_i| |q_j| <= 2 u_out for unit columns; 0 for fp32, whose rounding is the panel's own)."""
    Q = to64(Q)
    m, k = Q.shape
    E = Q.t() @ Q - torch.eye(k, dtype=torch.float64)
    lim = C_QR * m * U32 + (2 * UNIT_ROUNDOFF[out_dtype] if out_dtype != F32 else 0.0)
    return check_bound(E, torch.zeros_like(E), torch.full_like(E, lim), name=name + "^T " + name + " - I")


def check_qr(W, Q, R, k, out_dtype, name="qr", against_lapack=True) -> dict:
    """The well-defined parts of Q_out = Q[:, :k], R_out = R[:k, :] of W [m, n]:
    * R strictly below the diagonal exactly 0 (rows >= min(m, n) entirely 0);
    * columnwise backward error |W_j - (Q R)_j| <= C_QR m u ||W_j|| + 2 u_out (|Q| |R|)_j for the columns j < kc =
      min(k, m, n) that the panel factors (and every column when k = min(m, n): then Q R reproduces W);
    * orthogonality (check_orthonormal);
    * the R tail, columns >= kc (fp32 GEMM Q^T W from the panel's fp32 Q): against float64 Q_vis^T W of the visible Q,
      within one output ulp + fp32_floor over m terms + u_out |Q|^T |W| (the visible Q is the fp32 Q rounded to out_dtype);
    * against_lapack: Q column by column against LAPACK's float64 Q (same sign convention) within C_QR m u kappa + one ulp,
      kappa the 2-norm condition number of W[:, :kc] (the first-order sensitivity of Q to a relative backward error)."""
    W64, Q64 = to64(W), to64(Q)
    m, n = W64.shape
    kc = min(k, m, n)
    stats = {}
    if torch.isnan(Q64).any() or (R is not None and torch.isnan(to64(R)).any()):
        raise NumericsError(f"{name}: NaN in Q or R")
    stats["orth"] = check_orthonormal(Q64, out_dtype, name=name + ".Q")
    u_out = UNIT_ROUNDOFF[out_dtype] if out_dtype != F32 else 0.0
    if R is not None:
        R64 = to64(R)
        assert R64.shape == (k, n), (R64.shape, k, n)
        low = torch.tril(torch.ones(k, n, dtype=torch.bool), diagonal=-1)
        bad = low & (R64 != 0)
        if bad.any():
            i, j = (int(t) for t in torch.nonzero(bad)[0])
            raise NumericsError(f"{name}: {int(bad.sum())} elements of R below the diagonal are not 0 (first R[{i}, {j}] = "
                                f"{float(R64[i, j])})")
        QR = Q64 @ R64[:, :kc]
        bnd = C_QR * m * U32 * W64[:, :kc].norm(dim=0) + 2 * u_out * (Q64.abs() @ R64[:, :kc].abs())
        stats["backward"] = check_bound(QR, W64[:, :kc], bnd, name=name + ".QR - W")
        if n > kc:
            ref = Q64.t() @ W64[:, kc:]
            noise = fp32_floor((Q64 * Q64).t() @ (W64[:, kc:] ** 2), m) + u_out * (Q64.abs().t() @ W64[:, kc:].abs())
            stats["tail"] = check_bound(R64[:, kc:], ref, bound(ref, out_dtype, noise), name=name + ".R tail")
    if against_lapack:
        Qr = lapack_q(W64[:, :kc] if k <= min(m, n) else W64, k)
        kap = _condition(W64[:, :kc])
        lim = C_QR * m * U32 * kap + ulp(Qr, out_dtype)
        stats["lapack"] = check_bound(Q64, Qr, lim, name=name + ".Q vs LAPACK")
    return stats
