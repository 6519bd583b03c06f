"""Cases, float64 checks and a CPU emulation of the fused low-rank-accumulator pass (SOW_FUSE_ACC, include/sow_amd.h) -- a
plain module shared by tests/test_gpu_fused_acc.py and tests/test_fused_acc_numerics_cpu.py.

The contract (chain_wide_acc.hip): products and sums in fp32, u = the compute dtype's rounding,
    forward   h_acc = rn(x Q), h_live = rn(s x A) = h_save, y = rn(h_acc R + h_live B + bias)
    backward  dh_acc = rn(dY R^T), dh_live = rn(s dY B^T), dX = rn(dh_acc Q^T + dh_live A^T)
so y and dX carry ONE output rounding.  The bound of `check` is therefore the single-rounding one: one ulp of the reference,
the fp32 noise of a sum of n = d + r_pad terms, and the hidden rounding of the accumulator projection (x Q, dY R^T) -- without
the ulp(first) term that test_gpu_elementwise._check adds for the two-pass path (y_rounds = "twice").
"""
import torch

import test_gpu_elementwise as E
from numerics import (UNIT_ROUNDOFF, accumulation_term, bound, check_bound, check_h_save, fp32_floor, rne, to64)

BF16, F16 = torch.bfloat16, torch.float16


def case(name, dtype, T, d_in, d_out, r, r_acc, s=0.75, bias=True, seed=0):
    return E.Case(name, dtype, T, d_in, d_out, r, acc="lowrank", r_acc=r_acc, bias=bias, s=s, seed=seed, y_rounds="fused")


# (T, d_in, d_out, r_live, r_acc): the smallest shapes that reach every edge of the tile code
CASES = [
    # ragged last token block, widths not multiples of 64, live columns straddle the 64-column panel boundary (total 100)
    case("ragged_tot100", BF16, 193, 72, 264, 50, 50),
    # total 250 in r_pad 256
    case("tot250", BF16, 257, 264, 72, 50, 200, bias=False),
    case("tot250_f16", F16, 257, 264, 72, 50, 200),
    # total exactly 256, r_live = 64: column 63 is data, no ones column; dbias from the saved buffers by its r = 64 route
    case("tot256_r64", BF16, 130, 520, 264, 64, 192),
    # widths below one tile, total 4
    case("tiny_tot4", BF16, 129, 8, 24, 2, 2, bias=False),
    # one panel, total 64
    case("one_panel", BF16, 64, 128, 64, 2, 62),
    # a single token
    case("one_token", BF16, 1, 264, 520, 16, 100, bias=False),
    # the shape class of test_gpu_elementwise's lowrank_racc96
    case("racc96_f16", F16, 4097, 512, 264, 50, 96, s=0.5),
]


def r_pad(c):
    return (c.r + c.r_acc + 63) // 64 * 64


def check(c, d, out):
    """Element-wise checks of a fused call's outputs (CPU tensors; float64 references).  `out`: y, and optionally h (None:
    h_save was NULL), dx, dA, dB, dbias.  Returns {stage: worst err / limit}."""
    q = {k: to64(v) for k, v in d.items() if v is not None}
    x, A, B, dy, Q, R, s = q["x"], q["A"], q["B"], q["dy"], q["Q"], q["R"], c.s
    dt, u, T, r = c.dtype, UNIT_ROUNDOFF[c.dtype], c.T, c.r
    bias = q.get("bias", torch.zeros(c.d_out, dtype=torch.float64))
    xx, AA, BB, QQ, RR, dydy = x * x, A * A, B * B, Q * Q, R * R, dy * dy
    worst = {}
    # ---- h_save: the r <= 64 contract
    h = None
    if out.get("h") is not None:
        ref, sq = s * (x @ A), s * s * (xx @ AA)
        st = check_h_save(to64(out["h"]), ref, r, dt, acc=fp32_floor(sq, c.d_in), name=f"{c.name}: h_save")
        worst["h_save"] = st["worst"]
        h = to64(out["h"]).reshape(-1, 64)[:, :r]
    # ---- y: one rounding of first + h B + bias; x Q rounded before . R is the hidden rounding
    h_vis = h if h is not None else s * (x @ A)
    hh = h_vis * h_vis
    t = x @ Q
    hidden = [accumulation_term((t * t) @ RR, u)]
    if dt == F16:
        hidden.append(E._sub_term(RR.sum(0).expand(T, -1), dt))
    if h is None:   # h_save = NULL: the live projection's rounding is hidden as well
        hidden.append(accumulation_term(hh @ BB, u))
        if dt == F16:
            hidden.append(E._sub_term(BB.sum(0).expand(T, -1), dt))
    y_ref = t @ R + h_vis @ B + bias
    y_sq = hh @ BB + xx @ QQ @ RR
    st = check_bound(out["y"], y_ref, bound(y_ref, dt, fp32_floor(y_sq, c.d_in + r_pad(c)), *hidden), name=f"{c.name}: y")
    worst["y"] = st["worst"]
    dh = s * (dy @ B.t())
    dhdh = dh * dh
    if out.get("dA") is not None:
        # ---- weight gradients: the unchanged kernels, reading the fused kernel's h_save and dh (as _check does)
        st = E._rounded(out["dB"], h.t() @ dy, dt, fp32_floor(hh.t() @ dydy, T), f"{c.name}: dB")
        worst["dB"] = st["worst"]
        if c.bias:
            st = E._rounded(out["dbias"], dy.sum(0), dt, fp32_floor(dydy.sum(0), T), f"{c.name}: dbias")
            worst["dbias"] = st["worst"]
        dA_sq = xx.t() @ dhdh
        sub = [] if dt != F16 else [E._sub_term(xx.sum(0)[:, None].expand(-1, r), dt)]
        st = check_bound(out["dA"], x.t() @ dh, bound(x.t() @ dh, dt, accumulation_term(dA_sq, u), fp32_floor(dA_sq, T), *sub),
                         name=f"{c.name}: dA")
        worst["dA"] = st["worst"]
    if out.get("dx") is None:
        return worst
    # ---- dX: one rounding of first_b + dh A^T; dh and dY R^T are hidden roundings
    tb = dy @ R.t()
    extra = [accumulation_term((tb * tb) @ QQ.t(), u)]
    if dt == F16:
        extra += [E._sub_term(QQ.sum(1)[None, :].expand(T, -1), dt), E._sub_term(AA.sum(1)[None, :].expand(T, -1), dt)]
    dx_ref = dh @ A.t() + tb @ Q.t()
    dx_sq = dhdh @ AA.t() + dydy @ RR.t() @ QQ.t()
    st = check_bound(out["dx"], dx_ref, bound(dx_ref, dt, accumulation_term(dhdh @ AA.t(), u),
                                              fp32_floor(dx_sq, c.d_out + r_pad(c)), *extra), name=f"{c.name}: dx")
    worst["dx"] = st["worst"]
    return worst


def emulate(c, d, mm=None, rounds=1):
    """The contract on the CPU: h / y / dh / dx as the fused pass defines them, the roundings by numerics.rne (one step from
    float64).  mm: the product (default: float64 matmul; pass an fp32 one to include the accumulation noise).  rounds = 2:
    the two-pass path instead (the accumulator term rounded to y / dX, the live term added with a second rounding).
    The weight gradients are not emulated: their kernels are not part of the fused pass."""
    mm = mm or (lambda a, b: a @ b)
    q = {k: to64(v) for k, v in d.items() if v is not None}
    x, A, B, dy, Q, R, s, dt = q["x"], q["A"], q["B"], q["dy"], q["Q"], q["R"], c.s, c.dtype
    bias = q.get("bias", 0.0)

    def chain(X, Fa1, Fl1, Fa2, Fl2, add):
        ha, hl = rne(mm(X, Fa1), dt), rne(s * mm(X, Fl1), dt)
        if rounds == 1:
            return hl, rne(mm(torch.cat([ha, hl], 1), torch.cat([Fa2, Fl2], 0)) + add, dt)
        return hl, rne(rne(mm(ha, Fa2), dt) + mm(hl, Fl2) + add, dt)

    hl, y = chain(x, Q, A, R, B, bias)
    dhl, dx = chain(dy, R.t(), B.t(), Q.t(), A.t(), 0.0)
    h = torch.zeros(c.T, 64, dtype=torch.float64)
    h[:, :c.r] = hl
    if c.r < 64:
        h[:, 63] = 1.0
    return dict(h=h, y=y, dx=dx)
