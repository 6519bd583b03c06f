"""float64 references and element-wise checks of the batched tensor-train kernels (sow_amd/csrc/tt_batch.hip:
sow_tt_reconstruct_batch, sow_tt_decompose_batch, sow_ttadam_batch): a plain module next to numerics.py and
step_numerics.py, imported by test_tt_numerics_cpu.py (fp32 emulations and a fault catalogue) and by
test_gpu_tt_elementwise.py (the kernels).

A train is a list of cores, core k of shape [r_k, i_k, o_k, r_{k+1}], r_0 = r_d = 1.  It stands for the matrix
[prod i_k, prod o_k] whose element (row, col), row = (i_0 .. i_{d-1}), col = (o_0 .. o_{d-1}) most significant first, is the
product core_0[:, i_0, o_0, :] ... core_{d-1}[:, i_{d-1}, o_{d-1}, :]; `rows x cols` is its un-padded upper left corner.
The padded tensor in the order (i_0, o_0, i_1, o_1, ...) is what the decomposition unfolds: L_0 = reshape(i_0 o_0, -1).

Every reference is float64 arithmetic on the exact fp32 values the kernel read.  Every bound is one fp32 ulp plus multiples
of u = 2^-24 counted from the kernel's operations; the counts are given at each bound.
"""
from __future__ import annotations

import math

import torch

from numerics import NumericsError, bound, check_bound, fp32_floor, to64, ulp
from step_numerics import C_M, C_P, C_QR, C_V, F32, U32, lapack_q, ttadam_ref

# a stage of a decomposition counts as compared with LAPACK only while its kappa-scaled limit stays below this, per element
# of a unit column (an ill-conditioned unfolding, kappa ~ 1 / (m u), has no well-defined Q to compare with)
LAPACK_LIMIT = 2.0 ** -6
# an element of p whose reference interval is wider than this share of its update says nothing about the kernel
UNDECIDED_WIDTH = 2.0 ** -10
MAX_UNDECIDED = 0.01
# step_numerics.check_orthonormal allows C_QR m u: the m-term sums of the panel, with a 30-fold margin over fp32 LAPACK.  The
# unfoldings here go down to m = 4, where what does not scale with m shows: every one of the kc reflectors carries the
# roundings of its own tau and scale (a sum, a square root, a difference and a quotient each: 6 operations) into every
# column it touches; fp32 LAPACK at m = kc = 4 errs by 7.4 u, 1.9 m u.  So the bound is C_QR max(m, 6 kc) u: the house bound
# wherever m >= 6 kc (every unfolding of 192 rows or more, every rank <= 8 above 48 rows), and the reflector term below --
# 1.2 x the house bound at 100 x 60 [1, 16, 1] (m = 80, kc = 16), 2 x at stage 0 of 512 x 1376 [1, 32, 32, 1] (m = 96,
# kc = 32), 3.2 x at m = 30, kc = 16, 6 x at m = kc = 4.
REFLECTOR_OPS = 6


def orth_bound(m, kc):
    return C_QR * max(m, REFLECTOR_OPS * kc) * U32


def _prod(xs):
    return int(math.prod(int(x) for x in xs))


def core_shapes(ranks, in_dims, out_dims):
    return [(ranks[k], in_dims[k], out_dims[k], ranks[k + 1]) for k in range(len(in_dims))]


def _cores64(cores, in_dims, out_dims):
    """float64 copies, viewed [r_k, i_k, o_k, r_{k+1}] (flat cores are reshaped; r_0 = r_d = 1)."""
    d = len(in_dims)
    out, rk = [], 1
    for k, c in enumerate(cores):
        c = to64(c)
        io = in_dims[k] * out_dims[k]
        rn = 1 if k == d - 1 else c.numel() // (rk * io)
        out.append(c.reshape(rk, in_dims[k], out_dims[k], rn))
        rk = rn
    return out


def _contract(cores, in_dims, out_dims, rows, cols):
    acc = cores[0].reshape(-1, cores[0].shape[-1])
    for c in cores[1:]:
        acc = (acc @ c.reshape(c.shape[0], -1)).reshape(-1, c.shape[-1])
    d = len(in_dims)
    full = acc.reshape([x for k in range(d) for x in (in_dims[k], out_dims[k])])
    full = full.permute(*(list(range(0, 2 * d, 2)) + list(range(1, 2 * d, 2))))
    return full.reshape(_prod(in_dims), _prod(out_dims))[:rows, :cols]


def tt_matrix_ref(cores, in_dims, out_dims, rows, cols):
    """TensorTrain.to_matrix in float64: chain contraction over the bonds, de-interleave, un-pad."""
    return _contract(_cores64(cores, in_dims, out_dims), in_dims, out_dims, rows, cols)


def tt_matrix_abs(cores, in_dims, out_dims, rows, cols):
    """The same contraction of |cores|: the sum of the magnitudes of every product that enters an element."""
    return _contract([c.abs() for c in _cores64(cores, in_dims, out_dims)], in_dims, out_dims, rows, cols)


def tt_noise(cores, in_dims, out_dims, rows, cols):
    """The fp32 error of tt_eval at every element.  The value is a chain of vector-times-matrix products: at bond k >= 1
    every entry of the new vector is r_k sequential fmas (r_k roundings, each of a partial sum of at most the sum of the
    magnitudes: Higham's gamma_{r_k}), and the errors of the earlier bonds pass through the later ones with |core|.  To
    first order that is sum_{k=1}^{d-1} r_k u times the contraction of |cores|; one more u covers the second-order terms
    (sum r_k <= 160, so (sum r_k u)^2 < u).  Order 1: the value is a copy."""
    c64 = _cores64(cores, in_dims, out_dims)
    count = 1 + sum(c.shape[0] for c in c64[1:])
    return count * U32 * _contract([c.abs() for c in c64], in_dims, out_dims, rows, cols)


def pad_interleave_ref(mat, in_dims, out_dims):
    """from_matrix's zero-pad to [prod i_k, prod o_k], reshape to (i_0 .. i_{d-1}, o_0 .. o_{d-1}) and interleave to
    (i_0, o_0, i_1, o_1, ...): the flat L_0 of the decomposition, float64."""
    mat = to64(mat)
    d = len(in_dims)
    full = torch.zeros(_prod(in_dims), _prod(out_dims), dtype=torch.float64)
    full[:mat.shape[0], :mat.shape[1]] = mat
    full = full.reshape(list(in_dims) + list(out_dims))
    perm = [ax for pair in zip(range(d), range(d, 2 * d)) for ax in pair]
    return full.permute(*perm).reshape(-1).contiguous()


def deinterleave(flat, in_dims, out_dims):
    """The inverse of pad_interleave_ref's permutation: flat (i_0, o_0, i_1, o_1, ...) -> [prod i_k, prod o_k]."""
    d = len(in_dims)
    full = flat.reshape([x for k in range(d) for x in (in_dims[k], out_dims[k])])
    full = full.permute(*(list(range(0, 2 * d, 2)) + list(range(1, 2 * d, 2))))
    return full.reshape(_prod(in_dims), _prod(out_dims))


def stage_shapes(ranks, in_dims, out_dims):
    """(m, ncols, kc, r) of the d - 1 stages: unfolding [m, ncols], truncation rank r = r_{k+1}, kc = min(r, m, ncols)
    columns go through the Householder panel, the other ncols - kc columns of R are Q^T L."""
    d = len(in_dims)
    nc = _prod(in_dims) * _prod(out_dims)
    out = []
    for k in range(d - 1):
        m = ranks[k] * in_dims[k] * out_dims[k]
        nc //= in_dims[k] * out_dims[k]
        r = ranks[k + 1]
        out.append((m, nc, min(r, m, nc), r))
    return out


def tt_decompose_ref(L0, ranks, in_dims, out_dims):
    """The sequential truncated complete-mode QR in float64 (LAPACK signs): core_k = Q[:, :r_{k+1}] of L_k = reshape(r_k i_k
    o_k, -1), L_{k+1} = R[:r_{k+1}, :]; the last core is the last remainder.  Q[:, :r] of a Householder QR depends on the
    first min(r, ncols) columns only, so the m x m Q is never formed for r <= ncols."""
    rest = to64(L0).reshape(-1)
    cores = []
    for k, (m, nc, kc, r) in enumerate(stage_shapes(ranks, in_dims, out_dims)):
        L = rest.reshape(m, nc)
        Q = lapack_q(L[:, :kc], r)
        R = Q.t() @ L
        R[:, :kc] = torch.triu(R[:, :kc])            # exact zeros where R = Q^T L holds rounding residue
        R[kc:, :] = 0.0
        cores.append(Q.reshape(ranks[k], in_dims[k], out_dims[k], r))
        rest = R.reshape(-1)
    cores.append(rest.reshape(ranks[-2], in_dims[-1], out_dims[-1], 1))
    return cores


# ---- checks ------------------------------------------------------------------------------------------------------------
def check_tt_matrix(out, cores, in_dims, out_dims, rows, cols, name="to_matrix", extra=None) -> dict:
    """out [rows, cols] against the float64 contraction of the cores the kernel read, per element within one fp32 ulp +
    tt_noise (+ `extra`, the noise of the cores themselves when they come from a decomposition under test)."""
    ref = tt_matrix_ref(cores, in_dims, out_dims, rows, cols)
    bnd = bound(ref, F32, tt_noise(cores, in_dims, out_dims, rows, cols))
    if extra is not None:
        bnd = bnd + to64(extra)
    return check_bound(out, ref, bnd, name=name)


def _merge(stats, key, st):
    if key not in stats or st["worst"] > stats[key]["worst"]:
        keep = {k: v for k, v in stats.get(key, {}).items() if k in ("counted", "stages")}
        stats[key] = dict(st, **keep)


def check_tt_decomposition(cores, L0_ref, ranks, in_dims, out_dims, input_noise=None, name="tt") -> dict:
    """The well-defined parts of a decomposition of L0_ref (flat, padded, interleaved, float64) from the visible cores.
    `input_noise`: a bound per element of L_0 on the difference between L0_ref and the L_0 the kernel itself factored (the
    Adam update's rounding; None for sow_tt_decompose_batch, whose L_0 is a copy).

    N_k is a bound per element on |L_k(visible) - L_k(kernel)|, where L_k(visible) is formed in float64 from L0_ref and
    the visible cores, L_{k+1} = reshape(core_k^T L_k), and L_k(kernel) is the fp32 unfolding the kernel factored:
      N_0 = input_noise,
      N_{k+1} = |core_k|^T N_k                                        the earlier noise through this product
              + fp32_floor((core_k^2)^T L_k^2, m) + ulp(L_{k+1})      m fp32 fmas per element of R = Q^T L, one rounding
              + 2 (orth bound) ||L_k[:, j]|| in the columns j < kc       there R comes from the panel, not from Q^T L: its
                backward error (L_j + dL_j = Q~ R_j, ||dL_j|| <= bound ||L_j||) and the distance of the visible Q from
                the orthogonal Q~ (the same bound) each move Q^T L_j by at most bound ||L_j||.
    Checks:
      orth    core k < d - 1 as [r_k i_k o_k, r_{k+1}]: |Q^T Q - I| <= C_QR max(m, REFLECTOR_OPS kc) u per element
              (step_numerics.check_orthonormal's bound, and the per-reflector term where m < 6 kc: see REFLECTOR_OPS);
      lapack  core k against lapack_q(L_k[:, :kc], r_{k+1}) within one ulp + (that bound + sqrt(2) ||N_k[:, :kc]||_F / ||L_k[:,
              :kc]||_2) kappa: check_qr's term, and the first-order perturbation bound of the Q factor, ||dQ||_F <= sqrt(2)
              kappa_2(A) ||dA||_F / ||A||_2 (Sun 1991; Higham, Accuracy and Stability, section 19.9), for the stage input's
              own noise.  A stage counts only while that limit stays below LAPACK_LIMIT; stats["lapack"]["counted"] and
              ["stages"] say how many did;
      proj    last core == core_{d-2}^T ... core_0^T L_0 within one ulp + N_{d-1};
      zero    kc < r: rows >= kc of R are exactly 0.  R is the last core, or the next unfolding, whose zero rows no
              reflector touches: there the next core holds the rows of the identity, exactly.
    """
    d = len(in_dims)
    c64 = _cores64(cores, in_dims, out_dims)
    for k, (c, shp) in enumerate(zip(c64, core_shapes(ranks, in_dims, out_dims))):
        assert tuple(c.shape) == tuple(shp), (name, k, tuple(c.shape), shp)
        if torch.isnan(c).any():
            raise NumericsError(f"{name}: NaN in core {k}")
    L = to64(L0_ref).reshape(-1)
    N = torch.zeros_like(L) if input_noise is None else to64(input_noise).reshape(-1)
    stats = {}
    counted = 0
    shapes = stage_shapes(ranks, in_dims, out_dims)
    for k, (m, nc, kc, r) in enumerate(shapes):
        Lk, Nk, Q = L.reshape(m, nc), N.reshape(m, nc), c64[k].reshape(m, r)
        floor_u = orth_bound(m, kc)
        E = Q.t() @ Q - torch.eye(r, dtype=torch.float64)
        _merge(stats, "orth", check_bound(E, torch.zeros_like(E), torch.full_like(E, floor_u), name=f"{name}.core{k}^T core{k} - I"))
        head = Lk[:, :kc]
        s = torch.linalg.svdvals(head)
        kap = float(s[0] / s[-1]) if float(s[-1]) > 0 else math.inf
        rel = float(Nk[:, :kc].norm() / s[0]) if float(s[0]) > 0 else math.inf
        lim = (floor_u + math.sqrt(2.0) * rel) * kap
        if lim < LAPACK_LIMIT:
            Qr = lapack_q(head, r)
            _merge(stats, "lapack", check_bound(Q, Qr, lim + ulp(Qr, F32), name=f"{name}.core{k} vs LAPACK"))
            counted += 1
        if kc < r:
            nxt = c64[k + 1].reshape(r, -1)
            if k + 1 == d - 1:
                nxt = nxt[kc:]
                want = torch.zeros_like(nxt)
            else:   # unfolding rows (a, i, o) with a >= kc of the next stage are zero: Q keeps the identity's rows there
                io = in_dims[k + 1] * out_dims[k + 1]
                nxt = c64[k + 1].reshape(r * io, -1)
                want = torch.eye(r * io, nxt.shape[1], dtype=torch.float64)[kc * io:]
                nxt = nxt[kc * io:]
            bad = nxt != want
            if bad.any():
                i, j = (int(t) for t in torch.nonzero(bad)[0])
                raise NumericsError(f"{name}: stage {k} has kc = {kc} < r = {r}, but {int(bad.sum())} elements of the rows "
                                    f">= kc of R are not exactly zero (first at [{i}, {j}]: {float(nxt[i, j])})")
            stats.setdefault("zero", dict(worst=0.0, over=0, numel=0, index=()))
            stats["zero"]["numel"] += nxt.numel()
        Rn = Q.t() @ Lk
        Nn = Q.abs().t() @ Nk + fp32_floor((Q * Q).t() @ (Lk * Lk), m) + ulp(Rn, F32)
        Nn[:, :kc] += 2 * floor_u * head.norm(dim=0)
        L, N = Rn.reshape(-1), Nn.reshape(-1)
    last = c64[-1].reshape(-1)
    stats["proj"] = check_bound(last, L, ulp(L, F32) + N, name=f"{name}.last core vs Q^T L_0")
    stats["proj"]["noise"] = N
    if shapes:
        stats.setdefault("lapack", dict(worst=0.0, over=0, numel=0, index=()))
        stats["lapack"]["counted"] = counted
        stats["lapack"]["stages"] = len(shapes)
    return stats


def ttadam_batch_ref(inputs):
    """float64 step of one item of sow_ttadam_batch.  inputs: p0, g [rows, cols]; cores_m0, cores_v0 (None when has_state
    is 0); ranks, in_dims, out_dims; betas (doubles), eps, step_size, lr_wd (the fp32 values of the item).
    Returns refs, mags of step_numerics.ttadam_ref at the reconstructed m and v, and their reconstruction noise e_m, e_v."""
    rows, cols = inputs["p0"].shape
    hp = dict(betas=inputs["betas"], eps=inputs["eps"], step_size=inputs["step_size"], lr_wd=inputs["lr_wd"])
    if inputs["has_state"]:
        a = (inputs["in_dims"], inputs["out_dims"], rows, cols)
        m0, v0 = tt_matrix_ref(inputs["cores_m0"], *a), tt_matrix_ref(inputs["cores_v0"], *a)
        e_m, e_v = tt_noise(inputs["cores_m0"], *a), tt_noise(inputs["cores_v0"], *a)
    else:
        m0 = v0 = e_m = e_v = torch.zeros(rows, cols, dtype=torch.float64)
    refs, mags = ttadam_ref(inputs["p0"], inputs["g"], m0, v0, clamp_v=bool(inputs["has_state"]), **hp)
    return refs, mags, m0, v0, e_m, e_v, hp


def ttadam_p_interval(inputs):
    """The interval of p over every m in [m - e_m, m + e_m] and v in [v - e_v, v + e_v] (clamped at 0 like the kernel's own
    v): p is linear in m for a fixed v and monotone in v for a fixed m, so its extremes over the box are at the four
    corners.  Returns mid, half-width, the largest magnitude of check_step's term over the corners, and the update
    magnitude step_size |m_new| / denom at the centre."""
    refs, mags, m0, v0, e_m, e_v, hp = ttadam_batch_ref(inputs)
    lo, hi, mag = refs["p"].clone(), refs["p"].clone(), mags["p"].clone()
    if inputs["has_state"]:
        for sm in (-1.0, 1.0):
            for sv in (-1.0, 1.0):
                r, g = ttadam_ref(inputs["p0"], inputs["g"], m0 + sm * e_m, v0 + sv * e_v, clamp_v=True, **hp)
                lo, hi, mag = torch.minimum(lo, r["p"]), torch.maximum(hi, r["p"]), torch.maximum(mag, g["p"])
    denom = refs["v"].sqrt() + inputs["eps"]
    upd = inputs["step_size"] * refs["m"].abs() / denom
    return (lo + hi) / 2, (hi - lo) / 2, mag, upd, (refs, mags, e_m, e_v)


def undecided_share(half, upd):
    return float((half > UNDECIDED_WIDTH * upd).sum()) / max(1, half.numel())


def check_ttadam_batch(p, cores_m, cores_v, inputs, name="ttadam", max_undecided=MAX_UNDECIDED) -> dict:
    """One item of sow_ttadam_batch: p [rows, cols] and the new m / v cores.
    p: inside the corner interval of ttadam_p_interval widened by one ulp + C_P u magnitude (check_step's term: the fp32
    rounding of the update itself).  The interval must not hide a failure: at most MAX_UNDECIDED of the elements may have
    a half-width above UNDECIDED_WIDTH of their update (stats["p"]["undecided"]; max_undecided = None leaves the
    assertion to a caller that sums stats["p"]["undecided_count"] over the items of its case).
    New cores: check_tt_decomposition of L_0 = pad_interleave(m_new), input noise C_M u (|b1 m| + |c1 g|) + b1 e_m, and of
    pad_interleave(v_new) with C_V u v_new + b2 e_v (the clamp does not widen e_v)."""
    mid, half, mag, upd, (refs, mags, e_m, e_v) = ttadam_p_interval(inputs)
    b1, b2 = inputs["betas"]
    stats = {"p": check_bound(p, mid, half + C_P * U32 * mag + ulp(mid, F32), name=f"{name}.p")}
    share = undecided_share(half, upd)
    stats["p"]["undecided"] = share
    stats["p"]["undecided_count"] = int((half > UNDECIDED_WIDTH * upd).sum())
    if max_undecided is not None and share > max_undecided:
        raise NumericsError(f"{name}.p: {100 * share:.3g} % of the elements are undecided (reference interval wider than "
                            f"2^-10 of the update); the case says too little about the kernel")
    dims = (inputs["in_dims"], inputs["out_dims"])
    for key, cores, c, b, e in (("m", cores_m, C_M, b1, e_m), ("v", cores_v, C_V, b2, e_v)):
        noise = pad_interleave_ref(c * U32 * mags[key] + b * e, *dims)
        st = check_tt_decomposition(cores, pad_interleave_ref(refs[key], *dims), inputs["ranks"], *dims, input_noise=noise,
                                    name=f"{name}.{key}")
        for k, s in st.items():
            stats[f"{key}.{k}"] = s
    return stats


# ---- test data (shared by the CPU emulation and the GPU tests) ------------------------------------------------------------
def default_dims(rows, cols, order):
    """from_matrix's mode sizes: ceil(M ** (1 / order)) in double precision, every mode alike."""
    return ([math.ceil(rows ** (1 / order))] * order, [math.ceil(cols ** (1 / order))] * order)


def quartered_grad(rows, cols, gen, small=True):
    """1e-2 N(0, 1) with a zero, a tiny (x 1e-6), a plain and a large (x 1e4) quarter, as the flat optimizer tests.
    small = False: no zero and no tiny quarter (plain and large halves) -- for the 'v_sq' state, whose near-zero and
    clamped elements leave p to v alone where g vanishes, and 1 / sqrt(v) decides nothing at v ~ 0."""
    g = torch.randn(rows * cols, generator=gen, dtype=torch.float64) * 1e-2
    t = g.numel() // 4
    if small:
        g[:t] = 0.0
        g[t:2 * t] *= 1e-6
    g[3 * t:] *= 1e4
    return g.reshape(rows, cols).float()


def small_and_plain_param(rows, cols, gen):
    """0.05 N(0, 1); every third element x 1e-4, so that its update is not hidden below C_P u |p|."""
    p = torch.randn(rows * cols, generator=gen, dtype=torch.float64) * 0.05
    p[::3] *= 1e-4
    return p.reshape(rows, cols).float()


def state_cores(kind, rows, cols, ranks, in_dims, out_dims, gen):
    """fp32 cores of a moment: the float64 decomposition of
    'm'        1e-4 (s a)(t b)^T + 1e-6 N(0, 1), a, b uniform in [0.5, 1.5], s, t random signs: of both signs, full rank, and
               bounded away from zero, so that where g = 0 the update b1 m is far above the reconstruction noise (a plain
               Gaussian m has 2 % of its elements within 1024 e_m of zero at rank 32), and a tenth of (1 - b1) g in the plain
               quarter, so that few elements of the new m cancel to within the noise;
    'v'        1e-4 a b^T + 1e-5 with a, b uniform in [0.5, 1.5]: positive and of low rank, the re-compressed v stays positive;
    'v_sq'     the square of 1e-2 N(0, 1): a lossy train of it is negative at some elements, the clamp is exercised."""
    if kind == "m":
        a = (torch.rand(rows, 1, generator=gen, dtype=torch.float64) + 0.5) * (torch.randint(0, 2, (rows, 1), generator=gen) * 2 - 1)
        b = (torch.rand(1, cols, generator=gen, dtype=torch.float64) + 0.5) * (torch.randint(0, 2, (1, cols), generator=gen) * 2 - 1)
        mat = 1e-4 * a * b + 1e-6 * torch.randn(rows, cols, generator=gen, dtype=torch.float64)
    elif kind == "v":
        a = torch.rand(rows, 1, generator=gen, dtype=torch.float64) + 0.5
        b = torch.rand(1, cols, generator=gen, dtype=torch.float64) + 0.5
        mat = 1e-4 * a * b + 1e-5
    else:
        mat = (torch.randn(rows, cols, generator=gen, dtype=torch.float64) * 1e-2) ** 2
    cores = tt_decompose_ref(pad_interleave_ref(mat, in_dims, out_dims), ranks, in_dims, out_dims)
    return [c.float() for c in cores]
