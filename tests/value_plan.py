"""Operand *values* for the element-wise checks (a plain module: CPU only, imports no GPU code).

tests/fuzz_plan.py draws shapes; every operand of the suite is Gaussian.  This module chooses values instead, for a fixed
list of cases (`cases()`, taken from fuzz_plan.plan() so that every case carries its kernel family, switches and rounding
class), in three families:

A  exact_layer / exact_gemm / exact_shared: signed sparse integers / half-integers and power-of-two scales for which the whole computation is exact.
   prove_layer / prove_gemm derive that from the float64 reference alone and raise NotExact otherwise:
   * every value a kernel stores in the narrow format before the end (h_save, dh, the first product of a "twice" path,
     x Q, dY R^T) satisfies rne(v) == v;
   * for every fp32 sum, sum_k |a_k| |b_k| divided by the unit (lsb(a) lsb(b), the largest power of two that divides every
     term) stays below 2^24, so every partial sum is an integer below 2^24 units: exact in any order, slab or K split;
   * fp32 cases: in every product one operand holds 8 significant bits (then the six plane products kept by the
     3 x bf16 split are the whole product), the other up to 24.
   Outputs need not be representable; they are compared with rne(ref64, dtype), bit for bit.
B  GRID / scale_layer: independent powers of two on x, A, B and dY, with W, Q, R, bias and the accumulated-onto
   gradients scaled to match, so that every output is the unscaled output shifted by a known exponent.  admits (from
   range_stats of the unscaled reference) and prove_gemm_range show that no operand, stored intermediate or output leaves the normal range, that no non-zero term of a
   sum lies below 2^-103 (an fp32 sum is a multiple of the ulp of its smallest addend: no partial sum is then rounded as a
   subnormal; fp32 operands: 2^-72, the lo plane of the split sits up to 2^-31 below the product) and that
   sum |terms| stays below the fp32 maximum.
C  poisons(c): one NaN, +Inf or -Inf inside the data -- an interior token row of x, the end of one row and the start of
   the next (ragged and misaligned views), the last token row, dY, A; the float64 reference evaluated on the poisoned
   operands decides which output elements may be non-finite.
"""
from __future__ import annotations

import dataclasses
import math
from typing import List

import torch

import fuzz_plan as FP
from numerics import F16_MAX, rne, to64

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
EMIN = {"bf16": -126, "f32": -126, "f16": -14}
FMAX = {"bf16": 2.0 ** 127 * (2 - 2.0 ** -7), "f32": 2.0 ** 127 * (2 - 2.0 ** -23), "f16": F16_MAX}
F32_MAX = FMAX["f32"]
EXACT_UNITS = 2.0 ** 24
TERM_FLOOR = {"bf16": 2.0 ** -103, "f16": 2.0 ** -103, "f32": 2.0 ** -72}


class NotExact(ValueError):
    pass


# ---- the case list ----------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Cases:
    layers: List[FP.Layer]
    groups: List[FP.Group]
    shared: List[FP.Shared]
    gemms: List[FP.Gemm]


# the generic-kernel cases taken: one per edge, the dtypes spread over them
GENERIC = {("bf16", "r_small_or_odd"), ("f16", "T<64"), ("f32", "ragged_r64"), ("f16", "ragged_r64"), ("bf16", "misaligned"),
           ("f32", "misaligned")}


def _pow2(s):
    return s if s > 0 and math.frexp(s)[0] == 0.5 else 0.5


def cases() -> Cases:
    """The smallest case of fuzz_plan.plan() for every (stratum, family, dtype, switches, accumulator) of the layers, six
    generic-kernel cases, the smallest group with the row-owner plan, the smallest bf16 shared-input set of two or more
    siblings and the smallest GEMM of every (kind, dtype, family); scales made powers of two (1 / r becomes 0.5)."""
    p = FP.plan()
    size = lambda c: c.T * (c.d_in + c.d_out) + (c.d_in * c.d_out if c.acc == "dense" else 0)   # noqa: E731
    best = {}
    for c in p.layers[:FP.N_FIRST_LAYERS]:   # (the first stream: the second's families have exact-operand tests of their own)
        key = (c.stratum, c.family, c.dtype, tuple(sorted(c.switches)), c.acc, c.edges if c.stratum == "generic" else ())
        if c.stratum == "generic" and (c.dtype, c.edges[0]) not in GENERIC:
            continue
        if c.stratum == "dense_long" or c.switches in ({"GEMM4": 0}, {"NO_SPLITK": 1}, {"GEMM3S": 0}) \
                or c.family == "gemm4_splitk_reduce_kernel" or (c.stratum, c.dtype) == ("gemm4h", "f16") \
                or (c.stratum == "chain2" and "TN_NARROW" in c.switches):
            continue   # (kept small for the CPU proofs: split-K, gemm2_kernel and gemm4_f16 are reached by the GEMM cases, the
            #            narrow weight-gradient kernel by the fp32 TN_NARROW case and its wide sibling by chain2)
        if key not in best or size(c) < size(best[key]):   # the smallest case of each kind (dict order: first appearance)
            best[key] = c
    layers = [dataclasses.replace(c, s=_pow2(c.s), name="v_" + c.name) for c in best.values()]
    rows = min((g for g in p.groups if g.rows), key=lambda g: sum(size(c) for c in g.layers))
    groups = [FP.Group("v_" + rows.name, [dataclasses.replace(c, s=_pow2(c.s)) for c in rows.layers], rows.deferred, rows.rows)]
    sh = min((s for s in p.shared if s.dtype == "bf16" and len(s.sibs) >= 2), key=lambda s: s.T * sum(b.d_out for b in s.sibs))
    shared = [dataclasses.replace(sh, name="v_" + sh.name)]
    gemms, seen = [], {}
    for g in p.gemms:
        key = (g.name.split("_")[1], g.dtype, g.family)
        if key[0] == "splitk" and (not g.use_ws or g.dtype == "f16"):   # (12.7 M-element operands: the bf16 one is kept)
            continue
        if key not in seen or g.M * g.N * g.K < seen[key].M * seen[key].N * seen[key].K:
            seen[key] = g
    gemms = [dataclasses.replace(g, name="v_" + g.name) for g in seen.values()]
    return Cases(layers, groups, shared, gemms)


# ---- helpers ----------------------------------------------------------------------------------------------------------
_MEMO = {}


def _memo(fn, t):
    """fn(t), kept per storage (x, dY, h and dh enter several sums, plain and transposed)."""
    key = (fn.__name__, t.data_ptr(), t.numel(), t._version)
    if key not in _MEMO:
        if len(_MEMO) > 256:
            _MEMO.clear()
        _MEMO[key] = (t, fn(t))   # holding t keeps its storage from being reused under the same key
    return _MEMO[key][1]


def lsb(t: torch.Tensor) -> float:
    """The largest power of two that divides every non-zero element of a float64 tensor (inf for an all-zero one)."""
    return _memo(_lsb, to64(t))


def _lsb(t):
    if t.numel() == 0:
        return math.inf
    bits = t.contiguous().view(torch.int64)
    exp = (bits >> 52) & 0x7FF                                   # (no subnormal float64 values occur here)
    mant = (bits & ((1 << 52) - 1)) | (1 << 52)
    low = (mant & -mant).double().view(torch.int64) >> 52       # 1023 + log2 of the lowest set bit of the significand
    p = torch.where(t != 0, low - 1023 + exp - 1075, 1 << 20).min()
    return math.inf if int(p) == 1 << 20 else 2.0 ** int(p)


def _minnz(t):
    return _memo(_minnz_, to64(t))


def _minnz_(t):
    return float(torch.where(t != 0, t.abs(), math.inf).min()) if t.numel() else math.inf


def _maxabs(t):
    return _memo(_maxabs_, to64(t))


def _maxabs_(t):
    return float(t.abs().max()) if t.numel() else 0.0


def sum_abs_bound(a, b, exact=False):
    """An upper bound of max_ij sum_k |a_ik| |b_kj|: min(max|a| max_j sum_k |b_kj|, max|b| max_i sum_k |a_ik|), or the
    product |a| @ |b| itself (exact=True)."""
    if exact:
        return float((to64(a).abs() @ to64(b).abs()).max())
    (amax, _, arow), (bmax, bcol, _) = _abs_stats(to64(a)), _abs_stats(to64(b))
    return min(amax * bcol, bmax * arow)


def _abs_stats(t):
    """(max |t|, largest column sum of |t|, largest row sum of |t|), kept per storage: a transposed view swaps the sums."""
    if t.dim() == 2 and not t.is_contiguous() and t.t().is_contiguous():
        mx, col, row = _abs_stats(t.t())
        return mx, row, col
    return _memo(_abs_stats_, t)


def _abs_stats_(t):
    a = t.abs()
    return float(a.max()), float(a.sum(0).max()), float(a.sum(-1).max())


def _fits(t, dtype):
    """rne(t, dtype) == t everywhere (a value survives the cast exactly when it is representable)."""
    t = to64(t)
    return bool((t.to(dtype).double() == t).all())


def _ternary(g, shape, density, step=1.0, twos=True):
    """Signed sparse values in {-step, 0, +step}; `twos`: a quarter of the non-zeros are +-2 step.  One uniform draw per
    element decides all three."""
    u = torch.rand(shape, generator=g)
    v = torch.zeros(shape, dtype=torch.float64)
    half = density / 2
    v[u < density] = step
    v[u < half] = -step
    if twos:
        v[(u < half / 4) | ((u >= half) & (u < half + half / 4))] *= 2
    return v


def _edges(t, rows_of_tokens=False):
    """Non-zero entries in the first and last row and column and, for a token-major operand, in the rows on both sides of
    every 64-token boundary."""
    n, m = t.shape
    rows, cols = [0, 0, n - 1, n - 1], [0, m - 1, 0, m - 1]
    if rows_of_tokens:
        for b in range(64, n, 64):
            rows += [b - 1, b]
            cols += [(b // 64) % m, (b // 64 + 1) % m]
    rows, cols = torch.tensor(rows), torch.tensor(cols)
    cur = t[rows, cols]
    t[rows, cols] = torch.where(cur != 0, cur, torch.where((rows + cols) % 2 == 0, -1.0, 1.0).double())
    return t


def _wide_values(g, shape, bits=17, frac=6):
    """Odd integers below 2^bits times 2^-frac (`bits` significant bits), random signs."""
    odd = (torch.randint(2 ** (bits - 2), 2 ** (bits - 1), shape, generator=g) * 2 + 1).double() * 2.0 ** -frac
    return torch.where(torch.rand(shape, generator=g) < 0.5, -odd, odd)


def _widen_rows(g, t, n_rows=16):
    """17-bit values in an eighth of the elements of up to n_rows token rows (the first, the last, rows next to 64-token
    boundaries, random ones): a sum over the tokens then holds at most n_rows wide terms."""
    T, m = t.shape
    rows = {0, T - 1} | {min(T - 1, b) for b in (63, 64, 255, 256)} | {int(i) for i in torch.randint(0, T, (n_rows,), generator=g)}
    rows = torch.tensor(sorted(rows)[:n_rows])
    sub = t[rows]
    hit = torch.rand(sub.shape, generator=g) < max(0.125, 2.0 / m)
    t[rows] = torch.where(hit, _wide_values(g, sub.shape), sub)
    return t


def _widen(g, t, prob):
    """17-bit values in a share `prob` of the elements of a weight."""
    return torch.where(torch.rand(t.shape, generator=g) < prob, _wide_values(g, t.shape), t)


# ---- family A: layers ---------------------------------------------------------------------------------------------------
def exact_layer(c, level=0):
    """Exact operands of a layer (a dict as test_gpu_elementwise._inputs gives, float64 values representable in c.dtype).
    Each `level` halves the densities of x and dY (the weights grow denser to keep ~2.5 terms in every h and dh).  fp32:
    one operand carries 17-bit values -- A or B at T <= 128, else 16 token rows of x or of dY, since a wide operand in
    every term of a T-long sum would take it past 2^24 units."""
    g = torch.Generator().manual_seed(77000 + c.seed + c.T + 3 * c.r)
    k = 0.5 ** level
    T, d_in, d_out, r = c.T, c.d_in, c.d_out, c.r
    long_t = max(1.0, T / 4096.0)
    px = min(0.5, max(0.25 * k / long_t, 4.0 / d_in))
    pdy = min(0.5, max(0.125 * k / long_t, 4.0 / d_out))
    pA = min(1.0, max(3.0 / r, 2.5 / (px * d_in)))
    pB = min(1.0, max(3.0 / r, 2.5 / (pdy * d_out)))
    d = dict(x=_edges(_ternary(g, (T, d_in), px, twos=False), True), A=_edges(_ternary(g, (d_in, r), pA)),
             B=_edges(_ternary(g, (r, d_out), pB)), bias=_ternary(g, (d_out,), 0.75, 0.5) if c.bias else None,
             dy=_edges(_ternary(g, (T, d_out), pdy, twos=False), True))
    if c.acc == "dense":
        d["W"] = _edges(_ternary(g, (d_in, d_out), min(1.0, 2.0 / (px * d_in))))
    elif c.acc == "lowrank":
        pQ = min(1.0, max(3.0 / c.r_acc, 2.5 / (px * d_in)))
        d["Q"] = _edges(_ternary(g, (d_in, c.r_acc), pQ))
        d["R"] = _edges(_ternary(g, (c.r_acc, d_out), min(1.0, max(3.0 / c.r_acc, 2.5 / (pdy * d_out)))))
    if c.grad_beta:
        d["dA0"], d["dB0"] = _ternary(g, (d_in, r), 0.5, 0.5), _ternary(g, (r, d_out), 0.5, 0.5)
        d["dbias0"] = _ternary(g, (d_out,), 0.5, 0.5) if c.bias else None
    if c.dtype == "f32":
        w = wide_operand(c)
        d[w] = _widen(g, d[w], 1.0 / 16) if w in ("A", "B") else _widen_rows(g, d[w])
    return d


def wide_operand(c):
    return ("A", "B")[c.seed % 2] if c.T <= 128 else ("x", "dy")[c.seed % 2]


def layer_refs(c, d):
    """float64 references of every output and of every intermediate a kernel stores, from the operands alone."""
    q = {k: to64(v) for k, v in d.items() if v is not None}
    x, A, B, dy, s, gb = q["x"], q["A"], q["B"], q["dy"], c.s, c.grad_beta
    f = dict(xA=x @ A)
    f["h"] = s * f["xA"]
    f["dh"] = s * (dy @ B.t())
    y, dx = f["h"] @ B, f["dh"] @ A.t()
    if "bias" in q:
        y = y + q["bias"]
    if c.acc == "dense":
        f["first"], f["first_b"] = x @ q["W"], dy @ q["W"].t()
    elif c.acc == "lowrank":
        f["t"], f["t_b"] = x @ q["Q"], dy @ q["R"].t()
        f["first"], f["first_b"] = f["t"] @ q["R"], f["t_b"] @ q["Q"].t()
    if c.acc:
        y, dx = y + f["first"], dx + f["first_b"]
    f.update(y=y, dx=dx, dA=x.t() @ f["dh"] + (gb * q["dA0"] if gb else 0), dB=f["h"].t() @ dy + (gb * q["dB0"] if gb else 0))
    if "bias" in q:
        f["dbias"] = dy.sum(0) + (gb * q["dbias0"] if gb else 0)
    return f


def layer_products(c, d, f):
    """(name, a, b, extra addends) of every sum a kernel forms."""
    q = {k: to64(v) for k, v in d.items() if v is not None}
    x, A, B, dy, gb = q["x"], q["A"], q["B"], q["dy"], c.grad_beta
    ones = torch.ones(1, c.T, dtype=torch.float64)
    out = [("h", x, A, []), ("y", f["h"], B, [q["bias"]] if "bias" in q else []), ("dh", dy, B.t(), []),
           ("dA", x.t(), f["dh"], [gb * q["dA0"]] if gb else []), ("dB", f["h"].t(), dy, [gb * q["dB0"]] if gb else []),
           ("dx", f["dh"], A.t(), [])]
    if "bias" in q:
        out.append(("dbias", ones, dy, [gb * q["dbias0"]] if gb else []))
    if c.acc == "dense":
        out += [("xW", x, q["W"], [f["h"] @ B]), ("dyW", dy, q["W"].t(), [f["dh"] @ A.t()])]
    elif c.acc == "lowrank":
        out += [("xQ", x, q["Q"], []), ("tR", f["t"], q["R"], [f["h"] @ B]), ("dyR", dy, q["R"].t(), []),
                ("tQ", f["t_b"], q["Q"].t(), [f["dh"] @ A.t()])]
    return out


STORED = ("xA", "h", "dh", "t", "t_b", "first", "first_b")


def prove_layer(c, d):
    """The exactness proof of family A for a layer; returns the references."""
    dtype = DT[c.dtype]
    for k, v in d.items():
        if v is not None and not _fits(v, dtype):
            raise NotExact(f"{c.name}: operand {k} is not representable in {c.dtype}")
    f = layer_refs(c, d)
    for k in STORED:
        if k in f and not _fits(f[k], dtype):
            raise NotExact(f"{c.name}: stored intermediate {k} is not representable in {c.dtype}")
    f["_sums"] = {name: _prove_sum(f"{c.name}: {name}", a, b, extra, c.dtype) for name, a, b, extra in layer_products(c, d, f)}
    return f


def _prove_sum(what, a, b, extra, dt):
    if dt == "f32" and not (_fits(a, torch.bfloat16) or _fits(b, torch.bfloat16)):
        raise NotExact(f"{what}: neither operand fits 8 significant bits")
    unit = min([lsb(a) * lsb(b)] + [lsb(e) for e in extra])
    add = sum(_maxabs(e) for e in extra)
    total = sum_abs_bound(a, b)
    if math.isfinite(unit) and (total + add) / unit >= EXACT_UNITS:
        total = sum_abs_bound(a, b, exact=True)
    if math.isfinite(unit) and (total + add) / unit >= EXACT_UNITS:
        raise NotExact(f"{what}: sum |terms| = {(total + add) / unit:.3g} units, not below 2^24")
    return total


def exact_layer_proved(c):
    """The densest exact operands of the ladder that pass prove_layer and the density conditions: (operands, refs)."""
    err = None
    for level in range(5):
        d = exact_layer(c, level)
        try:
            f = prove_layer(c, d)
            check_density(c, d, f)
            return d, f
        except NotExact as e:
            err = e
    raise err


def outputs_of(c):
    return ("h", "y", "dx", "dA", "dB") + (("dbias",) if c.bias else ())


def check_density(c, d, f):
    """Exactness is not bought with emptiness: half of every output non-zero, the edges of every operand populated, and at
    most a quarter of a 16-bit weight gradient beyond the integers its format resolves."""
    for k in outputs_of(c):
        nz = float((f[k] != 0).double().mean())
        if nz < 0.5:
            raise NotExact(f"{c.name}: {k} has {100 * nz:.0f} % non-zero elements")
    for k, v in d.items():
        if v is None or v.dim() != 2 or k in ("dA0", "dB0"):
            continue
        rows = [0, v.shape[0] - 1]
        if k in ("x", "dy"):
            rows += [b + o for b in range(64, v.shape[0], 64) for o in (-1, 0)]
        if not bool((v[rows] != 0).any(1).all()) or not bool((v[:, [0, -1]] != 0).any(0).all()):
            raise NotExact(f"{c.name}: an edge row or column of {k} is empty")
    if c.dtype != "f32":
        for k in ("dA", "dB"):
            bad = float((rne(f[k], DT[c.dtype]) != f[k]).double().mean())
            if bad > 0.25:
                raise NotExact(f"{c.name}: {100 * bad:.0f} % of {k} is not representable in {c.dtype}")
    if f32_gradients(c):
        for k in ("dA", "dB") + (("dbias",) if c.bias else ()):
            if not _fits(f[k], torch.float32):
                raise NotExact(f"{c.name}: {k} is not representable in fp32 (the run with fp32 gradients allows 0 %)")


def f32_gradients(c):
    """The long-T bf16 / f16 cases that run again with fp32 parameters and gradients (SOW_PARAM_F32): a 16-bit dA / dB above
    2^8 (2^11) is rounded once and may hide a dropped token; the fp32 gradient of the same exact sum hides nothing."""
    return c.dtype != "f32" and c.T >= 8192 and c.stratum in ("chain2", "gemm4h", "gemm2h", "lowrank")


# ---- family A: GEMM -------------------------------------------------------------------------------------------------------
def exact_gemm(gm):
    """op(A) [M, K], op(B) [K, N], bias, C0 of sow_gemm_ex with exact values; fp32: a 17-bit operand on one side."""
    g = torch.Generator().manual_seed(88000 + gm.seed)
    M, N, K = gm.M, gm.N, gm.K
    a = _edges(_ternary(g, (M, K), min(1.0, max(0.125, 8.0 / K))))
    b = _edges(_ternary(g, (K, N), min(1.0, max(1.0 / 16, 8.0 / K))))
    if gm.dtype == "f32":
        if gm.seed % 2:
            a = _widen(g, a, 1.0 / 64)
        else:
            b = _widen(g, b, 1.0 / 64)
    bias = _ternary(g, (N,), 0.75, 0.5) if gm.bias else None
    c0 = _ternary(g, (M, N), 0.5, 0.5) if gm.beta else None
    return a, b, bias, c0


def gemm_ref(gm, a, b, bias, c0):
    ref = gm.alpha * (to64(a) @ to64(b))
    if bias is not None:
        ref = ref + to64(bias)
    if c0 is not None:
        ref = ref + gm.beta * to64(c0)
    return ref


def prove_gemm(gm, a, b, bias, c0):
    for k, v in (("a", a), ("b", b), ("bias", bias), ("c0", c0)):
        if v is not None and not _fits(v, DT[gm.dtype]):
            raise NotExact(f"{gm.name}: operand {k} is not representable in {gm.dtype}")
    extra = ([to64(bias) / abs(gm.alpha)] if bias is not None else []) + ([gm.beta * to64(c0) / abs(gm.alpha)] if c0 is not None else [])
    _prove_sum(gm.name, to64(a), to64(b), extra, gm.dtype)
    ref = gemm_ref(gm, a, b, bias, c0)
    if float((ref != 0).double().mean()) < 0.5:
        raise NotExact(f"{gm.name}: fewer than half of C non-zero")
    return ref


def prove_gemm_range(gm, a, b, bias, c0, ea, eb):
    """Family B's condition for the GEMM operands a * 2^ea, b * 2^eb, bias and C0 * 2^(ea + eb)."""
    dt = gm.dtype
    lo, hi = 2.0 ** EMIN[dt], FMAX[dt]
    ref = gemm_ref(gm, a, b, bias, c0)
    for k, v, e in (("a", a, ea), ("b", b, eb), ("bias", bias, ea + eb), ("c0", c0, ea + eb), ("C", ref, ea + eb)):
        if v is not None and not (_minnz(v) * 2.0 ** e >= 2 * lo and _maxabs(v) * 2.0 ** e <= hi / 2):
            raise NotExact(f"{gm.name}: {k} * 2^{e} leaves the normal range of {dt}")
    extra = [v for v in (bias, c0) if v is not None]
    floor = min([_minnz(a) * _minnz(b) * abs(gm.alpha)] + [_minnz(v) * min(1.0, abs(gm.beta) or 1.0) for v in extra])
    if floor * 2.0 ** (ea + eb) < TERM_FLOOR[dt]:
        raise NotExact(f"{gm.name}: a non-zero term below {TERM_FLOOR[dt]:.3g}")
    total = abs(gm.alpha) * sum_abs_bound(a, b) + sum(_maxabs(v) for v in extra)
    if total * 2.0 ** (ea + eb) >= F32_MAX / 2:
        raise NotExact(f"{gm.name}: sum |terms| near the fp32 maximum")


def gemm_scales(gm):
    """(ea, eb) of the two grid points of a GEMM: near the top and near the bottom of the normal range."""
    hi = 100 if gm.dtype != "f16" else 4
    lo = -90 if gm.dtype == "bf16" else (-40 if gm.dtype == "f32" else -2)
    return ((hi // 2, hi - hi // 2), (lo // 2, lo - lo // 2))


# ---- shared-input sets ------------------------------------------------------------------------------------------------
def sib_layers(sp):
    """One Layer per sibling of a shared-input set (sow_backward_shared accumulates only dX: grad_beta = 0 here)."""
    return [FP.Layer(f"{sp.name}.s{j}", sp.dtype, sp.T, sp.d_in, sb.d_out, sb.r, bias=sb.bias, s=_pow2(sb.s), seed=17 * j + 1)
            for j, sb in enumerate(sp.sibs)]


def exact_shared(sp):
    """Exact operands of a sibling set: the siblings share the x of the first one's exact operands, each keeps its own A,
    B, bias and dY; the one dX = sum_i dh_i A_i^T + grad_beta dX0 is proved as one sum.  Returns (sibling layers, x,
    per-sibling operands, dX0, per-sibling references, the reference of dX)."""
    sibs = sib_layers(sp)
    first = [exact_layer_proved(c)[0] for c in sibs]
    x = first[0]["x"]
    ds = [dict(d, x=x) for d in first]
    fs = [prove_layer(c, d) for c, d in zip(sibs, ds)]
    for c, d, f in zip(sibs, ds, fs):
        check_density(c, d, f)
    dx0 = _ternary(torch.Generator().manual_seed(5), (sp.T, sp.d_in), 0.5, 0.5) if sp.grad_beta else None
    _prove_sum(f"{sp.name}: dX", torch.cat([f["dh"] for f in fs], 1), torch.cat([d["A"].t() for d in ds], 0),
               [sp.grad_beta * dx0] if sp.grad_beta else [], sp.dtype)
    ref_dx = sum(f["dx"] for f in fs) + (sp.grad_beta * dx0 if sp.grad_beta else 0)
    per = [dict(A=d["A"], B=d["B"], bias=d["bias"], dy=d["dy"]) for d in ds]
    return sibs, x, per, dx0, fs, ref_dx


# ---- family B: powers of two ------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Scale:
    x: int = 0
    A: int = 0
    B: int = 0
    dy: int = 0

    def exps(self):
        """Exponent shift of every operand, stored intermediate and output of a layer (Q scales as A, R as B, W as A B;
        bias and the gradients accumulated onto as the outputs they join)."""
        h, y, dh = self.x + self.A, self.x + self.A + self.B, self.dy + self.B
        return dict(x=self.x, A=self.A, B=self.B, dy=self.dy, Q=self.A, R=self.B, W=self.A + self.B, bias=y, xA=h, h=h, t=h,
                    y=y, first=y, dh=dh, t_b=dh, dx=dh + self.A, first_b=dh + self.A, dA=self.x + dh, dA0=self.x + dh,
                    dB=h + self.dy, dB0=h + self.dy, dbias=self.dy, dbias0=self.dy, one=0)

    def tag(self):
        return f"x{self.x:+d}A{self.A:+d}B{self.B:+d}dy{self.dy:+d}"


# The grid walks the products from near the top of the normal range to near its bottom; which points a case admits is
# decided by admits(), from its reference (Gaussian operands reach down to 2^-25 of their scale, so only exact operands
# admit the lowest point).  f16: dY * 2^16 is representable only for |dY| < 1, and with factors of order 1 it takes
# dh = s dY B^T past 65504 -- the overflow a GradScaler's inf check exists for -- so the GradScaler point carries dY of
# magnitude 2^-3 and x, A, B of 2^-2 .. 2^-5; a bias gradient (a sum over all tokens) overflows there whatever the
# factors, and so does dB at long T with these integer operands, so only some layers admit it.
GRADSCALER = Scale(-3, -2, -5, 13)   # dY of magnitude 2^-3 times a GradScaler's 2^16
GRID = {"bf16": (Scale(40, 30, 20, 30), Scale(50, -45, 20, -10), Scale(-20, -12, -8, -15), Scale(-40, -25, -15, -35)),
        "f32": (Scale(40, 30, 20, 30), Scale(50, -45, 20, -10), Scale(-8, -5, -3, -6), Scale(-20, -12, -8, -15)),
        "f16": (Scale(3, 2, 1, 2), Scale(2, -1, 1, 0), GRADSCALER, Scale(-1, 0, -1, -1))}
PRODUCT_EXPS = dict(h=("x", "A"), y=("h", "B"), dh=("dy", "B"), dA=("x", "dh"), dB=("h", "dy"), dx=("dh", "A"),
                    dbias=("one", "dy"), xW=("x", "W"), dyW=("dy", "W"), xQ=("x", "Q"), tR=("t", "R"), dyR=("dy", "R"),
                    tQ=("t_b", "Q"))
PRODUCT_OUT = dict(h="h", y="y", dh="dh", dA="dA", dB="dB", dx="dx", dbias="dbias", xW="y", dyW="dx", xQ="t", tR="y", dyR="t_b",
                   tQ="dx")


def scale_layer(d, e: Scale):
    exp = e.exps()
    return {k: (None if v is None else torch.ldexp(to64(v), torch.tensor(exp[k]))) for k, v in d.items()}


def range_stats(c, d, f=None):
    """What admits() needs of the unscaled case: (smallest non-zero, largest) magnitude of every operand, stored
    intermediate and output, and per sum the smallest non-zero factors and a bound of sum |terms|."""
    f = f or layer_refs(c, d)
    mm = {k: (_minnz(v), _maxabs(v)) for k, v in d.items() if v is not None}
    mm.update({k: (_minnz(f[k]), _maxabs(f[k])) for k in STORED + outputs_of(c) if k in f})
    mn = {}

    def minnz(t):   # x, dY, h and dh enter several sums
        if id(t) not in mn:
            mn[id(t)] = (t, _minnz(t))
        return mn[id(t)][1]

    known = f.get("_sums", {})
    sums = {name: (minnz(a), minnz(b), known[name] if name in known else sum_abs_bound(a, b),
                   min([_minnz(e) for e in extra] + [math.inf]), sum(_maxabs(e) for e in extra))
            for name, a, b, extra in layer_products(c, d, f)}
    return dict(mm=mm, sums=sums)


def admits(c, st, e: Scale, exact, bottom=True):
    """Family B's condition for layer c at grid point e, from range_stats of the unscaled operands: None when it holds,
    else the reason.  No operand, stored intermediate or output outside the normal range of c.dtype (a Gaussian output may
    cancel to anything: with exact=False an output -- never a stored intermediate -- below the range is left to the float64
    check and named in the returned set instead), no non-zero term below TERM_FLOOR, sum |terms| below half the fp32
    maximum.  bottom=False asks for the upper end only (f16 Gaussian operands hold h and dh of any size already unscaled:
    such a run is held to its float64 limits, not to the shift identity)."""
    dt, exp = c.dtype, e.exps()
    lo, hi = 2.0 ** EMIN[dt], FMAX[dt]
    below = set()
    for k, (mn, mx) in st["mm"].items():
        sc = 2.0 ** exp[k]
        if mx * sc > hi / 2:
            return f"{k} reaches {mx * sc:.3g}"
        if bottom and mn * sc < 2 * lo:
            if exact or k not in outputs_of(c) or k == "h":
                return f"{k} has a non-zero element of {mn * sc:.3g}"
            below.add(k)
    for name, (ma, mb, tot, me, xe) in st["sums"].items():
        ea, eb = (exp[k] for k in PRODUCT_EXPS[name])
        eo = exp[PRODUCT_OUT[name]]
        if bottom and (ma * mb * 2.0 ** (ea + eb) < TERM_FLOOR[dt] or me * 2.0 ** eo < TERM_FLOOR[dt]):
            return f"{name} has a non-zero term below {TERM_FLOOR[dt]:.3g}"
        if tot * 2.0 ** (ea + eb) + xe * 2.0 ** eo >= F32_MAX / 2:
            return f"{name}: sum |terms| near the fp32 maximum"
    return below


def grid_for(c, st, exact, bottom=True):
    """[(Scale, outputs below the normal range)] of the grid points layer c admits."""
    out = []
    for e in GRID[c.dtype]:
        r = admits(c, st, e, exact, bottom)
        if not isinstance(r, str):
            out.append((e, r))
    return out


# ---- family C: non-finite values inside the data --------------------------------------------------------------------------
POISON_VALUES = (float("nan"), float("inf"), float("-inf"))


def poisons(c):
    """(tag, operand, [(row, column), ...]) placements for layer c: (i) one element of an interior token row of x, (ii) the
    last element of a row and the first of the next (ragged widths and misaligned views), (iii) the last token row,
    (iv) one element of dY, (v) one element of A -- in the middle of a row, and at the head of a row (the element that
    follows the previous row in storage)."""
    T, mid = c.T, c.T // 2 + 1
    out = [("x_mid", "x", [(mid, c.d_in // 3)])]
    if (c.d_in % 8 or c.misalign) and T > 2:
        out.append(("x_wrap", "x", [(mid, c.d_in - 1), (mid + 1, 0)]))
    out += [("x_last", "x", [(T - 1, c.d_in - 1)]), ("dy", "dy", [(T // 3, c.d_out // 2)]), ("A", "A", [(c.d_in // 2, c.r // 2)]),
            ("A_head", "A", [(c.d_in // 2, 0)])]
    return out


def a_overlap_columns(c, row, col):
    """The columns of dX that a non-finite A[row, col] may take with it (include/sow_amd.h): the kernels read a row of A
    together with what follows it in storage, up to 64 elements, against explicit zeros -- and 0 x NaN is NaN.  The rows
    i < row whose 64-element windows reach the element: (row - i) r + col < 64."""
    return range(max(0, row - (63 - col) // c.r), row) if col <= 63 else range(row, row)


def poison(d, operand, where, value):
    d = dict(d)
    t = d[operand].clone()
    for i, j in where:
        t[i, j] = value
    d[operand] = t
    return d
