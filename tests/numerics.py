"""Element-wise comparators of kernel outputs against float64 references (a plain module, imported by the tests like
protocols.py).

`rel_err` (conftest.py) is a max-norm over a whole tensor: it cannot see a ragged tail that went missing, a truncating
store or a second rounding.  The checks here hold every element to its own limit:

* check_rounded -- a stage whose inputs the test can see (h_save = RNE(s x A), y from the kernel's own h_save, dB and dbias
  from h_save and dY): every element within `max_ulp` ulp of RNE_dtype(ref64), and at most `max_inexact` of the elements
  not bit-equal to it.  fp32 accumulation inside the kernel moves a result across a rounding point only rarely (CPU
  emulation, tests/test_numerics_cpu.py: under 0.05 % of bf16 elements at K = 512 .. 11008); a truncating store differs in
  about half of them, a second rounding in about a quarter.
* check_bound -- a stage with an intermediate rounding the test cannot see (dh in dA and dX, fp32 sums): |out - ref64| <=
  bound at every element, bound = one output ulp + LAMBDA * u * sqrt(n * sum_k (a_k b_k)^2) (accumulation_term).

On failure every checker names the worst element, its err / limit ratio, the number of elements over the limit and
whether they sit in the last row or column block (a ragged tail).
"""
from __future__ import annotations

import math

import torch

# significand bits (implicit bit included) and unit roundoff u = 2^-p of round-to-nearest
_P = {torch.bfloat16: 8, torch.float32: 24, torch.float16: 11}
UNIT_ROUNDOFF = {dt: 2.0 ** -p for dt, p in _P.items()}
# smallest normal exponent: 2^-126 for bf16 and fp32, 2^-14 for f16 (whose subnormal spacing is 2^-24)
_EMIN = {torch.bfloat16: -126, torch.float32: -126, torch.float16: -14}
# largest finite f16: RNE takes |t| >= 65504 + 16 (half an ulp, the tie rounds to the even 2^16) to inf
F16_MAX = 65504.0

# LAMBDA of the probabilistic accumulation term.  A sum of n intermediates c_k, each rounded with relative error
# |delta_k| <= u, errs by sum c_k delta_k: at most u * sqrt(n) * sqrt(sum c_k^2) (Cauchy-Schwarz), and for large n close to
# normal with standard deviation <= u * sqrt(sum c_k^2 / 3).  LAMBDA = 4 is then a hard bound up to n = 16 terms and
# 6.9 standard deviations beyond (an expected 1e-11 false alarms per element), while a lost term of average size stands
# out at T ~ 32768 (test_numerics_cpu.py keeps the kernels' emulation at <= 0.7 of the bound, the faults above 1).
LAMBDA = 4.0

# default fraction of elements allowed to differ from RNE(ref64) (check_rounded); the emulated kernels stay below a
# tenth of it at every shape of test_numerics_cpu.py
MAX_INEXACT = 0.005


def to64(v):
    """float64 CPU copy of a tensor (lists / tuples elementwise, everything else unchanged)."""
    if isinstance(v, torch.Tensor):
        return v.detach().to(device="cpu", dtype=torch.float64)
    if isinstance(v, (list, tuple)):
        return type(v)(to64(u) for u in v)
    return v


def ref64(fn, *args, **kw):
    """The oracle `fn` (oracle/sow_oracle.py works in its input dtype) evaluated on float64 copies of the exact inputs the
    kernel saw: ref64(O.sow_forward, x, [A], [B], None, None, s, bias)."""
    return fn(*to64(args), **{k: to64(v) for k, v in kw.items()})


def ulp(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Spacing of `dtype` (bf16 / fp32 / f16) at |t|, as float64: 2^(e - p) for |t| in [2^(e-1), 2^e); subnormal spacing
    below."""
    t = to64(t)
    _, e = torch.frexp(t.abs())
    emin = _EMIN[dtype]
    e = torch.where(t == 0, emin + 1, torch.clamp(e, min=emin + 1))
    return torch.ldexp(torch.ones_like(t), e - _P[dtype])


def rne(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Round a float64 tensor to the nearest `dtype` value, ties to even, in one step (no double rounding through fp32);
    returned as float64."""
    t = to64(t)
    q = ulp(t, dtype)
    r = torch.round(t / q) * q   # t / q and the product are exact (powers of two); torch.round is half-to-even
    if dtype == torch.float16:
        r = torch.where(r.abs() > F16_MAX, torch.copysign(torch.full_like(r, float("inf")), r), r)
    return r


def accumulation_term(sq: torch.Tensor, u: float, n: int = 1, lam: float = LAMBDA) -> torch.Tensor:
    """lam * u * sqrt(n * sq): `sq` = sum_k (a_k b_k)^2 of the terms whose rounding the test cannot see (the oracle
    evaluated on squared inputs).  n = 1 for intermediates rounded once each (dh in bf16); n = the reduction length for
    fp32 running sums, whose errors scale with the partial sums rather than with the terms."""
    return lam * u * torch.sqrt(n * to64(sq))


def fp32_floor(sq: torch.Tensor, n: int) -> torch.Tensor:
    """The fp32 accumulation noise of an n-term kernel sum whose squared terms sum to `sq` (check_rounded's `acc`)."""
    return accumulation_term(sq, UNIT_ROUNDOFF[torch.float32], n)


def bound(ref: torch.Tensor, dtype: torch.dtype, *terms: torch.Tensor) -> torch.Tensor:
    """One output ulp at |ref| plus the accumulation terms."""
    b = ulp(ref, dtype)
    for t in terms:
        b = b + t
    return b


class NumericsError(AssertionError):
    pass


def _tail_note(over: torch.Tensor) -> str:
    """Where the elements over the limit sit: share of them in the last 64-row block / last 64-column block."""
    n = int(over.sum())
    if n == 0:
        return ""
    parts = []
    if over.dim() >= 2 and over.shape[0] > 64:
        k = int(over[-64:].sum())
        parts.append(f"{k}/{n} in the last row block")
    if over.shape[-1] > 64:
        k = int(over[..., -64:].sum())
        parts.append(f"{k}/{n} in the last column block")
    if over.dim() >= 2:
        rows = torch.nonzero(over.reshape(over.shape[0], -1).any(dim=1)).flatten()
        if rows.numel() <= 4:
            parts.append(f"rows {rows.tolist()}")
    cols = torch.nonzero(over.reshape(-1, over.shape[-1]).any(dim=0)).flatten()
    if cols.numel() <= 4:
        parts.append(f"columns {cols.tolist()}")
    return "; ".join(parts)


def _report(name: str, err: torch.Tensor, lim: torch.Tensor, out64: torch.Tensor, ref: torch.Tensor, what: str):
    # err = 0 is within any limit, a limit of 0 included (max_ulp = 0: 0 / 0 is not "over"); err > 0 over a limit of 0 is inf
    ratio = torch.where(err == 0, torch.zeros_like(err), err / lim)
    ratio = torch.where(torch.isnan(err) | torch.isnan(ratio), torch.full_like(err, math.inf), ratio)
    flat = int(torch.argmax(ratio.reshape(-1)))
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape)) if ratio.dim() else ()
    over = ratio > 1
    stats = dict(worst=float(ratio.reshape(-1)[flat]) if ratio.numel() else 0.0, index=idx, over=int(over.sum()),
                 numel=ratio.numel())
    msg = (f"{name}: {what}: worst element {idx} err/limit = {stats['worst']:.3g} (got {float(out64.reshape(-1)[flat]):.9g}, "
           f"ref {float(ref.reshape(-1)[flat]):.9g}, limit {float(lim.reshape(-1)[flat]):.3g}); "
           f"{stats['over']} of {ratio.numel()} elements over the limit")
    tail = _tail_note(over) if ratio.dim() else ""
    return stats, over, msg + (f" ({tail})" if tail else "")


def check_rounded(out: torch.Tensor, ref: torch.Tensor, dtype: torch.dtype, max_ulp: float = 1,
                  max_inexact: float = MAX_INEXACT, min_count: int = 2, acc=None, name: str = "out") -> dict:
    """`out` (stored in `dtype`) within max_ulp ulp of RNE_dtype(ref) everywhere, and not bit-equal to it in at most
    max(max_inexact * numel, min_count) elements (min_count: a handful of rare tie-crossings in a small tensor).
    `acc`: the fp32 accumulation noise of the kernel's sums (accumulation_term(sq, 2^-24, K)), added to the limit -- it
    matters only where the sum cancels to far below its terms, where one ulp of the result is below fp32's resolution of
    the terms.  max_ulp = 0, max_inexact = 0, min_count = 0 means bit-exact: every element equal to RNE_dtype(ref), the
    first one that is not named in the error.  Returns the statistics (worst ratio, inexact fraction)."""
    out64, ref = to64(out), to64(ref)
    assert out64.shape == ref.shape, f"{name}: shape {tuple(out64.shape)} vs reference {tuple(ref.shape)}"
    r = rne(ref, dtype)
    err = torch.where(out64 == r, torch.zeros_like(r), (out64 - r).abs())   # an f16 inf equal to RNE(ref) = inf: err 0
    lim = max_ulp * ulp(r, dtype)
    if acc is not None:
        lim = lim + to64(acc)
    stats, over, msg = _report(name, err, lim, out64, r, f"more than {max_ulp} ulp from RNE(ref64)")
    inexact = int(((out64 != r) | torch.isnan(out64)).sum())
    stats["inexact"] = inexact / max(1, err.numel())
    if stats["over"]:
        raise NumericsError(msg)
    allowed = max(max_inexact * err.numel(), min_count)
    if inexact > allowed:
        raise NumericsError(f"{name}: {inexact} of {err.numel()} elements ({100 * stats['inexact']:.3g} %) differ from "
                            f"RNE(ref64), allowed {allowed:.0f} ({_tail_note(out64 != r)}); {msg}")
    return stats


def check_bound(out: torch.Tensor, ref: torch.Tensor, bnd: torch.Tensor, name: str = "out") -> dict:
    """|out - ref| <= bnd at every element (NaN fails).  Returns the statistics (worst err / bound)."""
    out64, ref = to64(out), to64(ref)
    assert out64.shape == ref.shape, f"{name}: shape {tuple(out64.shape)} vs reference {tuple(ref.shape)}"
    bnd = torch.broadcast_to(to64(bnd), ref.shape)
    err = (out64 - ref).abs()
    stats, over, msg = _report(name, err, bnd, out64, ref, "|out - ref64| over the bound")
    if stats["over"] or torch.isnan(err).any():
        raise NumericsError(msg)
    return stats


def check_h_save(h: torch.Tensor, ref_live: torch.Tensor, r: int, dtype: torch.dtype, bnd=None, acc=None,
                 name: str = "h_save") -> dict:
    """The h_save contract of DESIGN section 3 for r <= 64: h [T, 64]; columns < r equal RNE(s x A) (check_rounded, or
    check_bound with `bnd` for fp32; `acc` as in check_rounded), columns r..62 exactly 0, column 63 exactly 1.0 when r <= 63."""
    h64 = to64(h).reshape(-1, 64)
    live = h64[:, :r]
    stats = check_rounded(live, ref_live, dtype, acc=acc, name=name + "[:, :r]") if bnd is None else \
        check_bound(live, ref_live, bnd, name=name + "[:, :r]")
    pad_end = 63 if r <= 63 else 64
    if pad_end > r:
        pad = h64[:, r:pad_end]
        bad = torch.zeros_like(h64, dtype=torch.bool)
        bad[:, r:pad_end] = (pad != 0) | torch.isnan(pad)
        if bad.any():
            i, j = (int(v) for v in torch.nonzero(bad)[0])
            raise NumericsError(f"{name}: {int(bad.sum())} padding elements are not 0 (first at row {i}, column {j}: "
                                f"{float(h64[i, j])}); {_tail_note(bad)}")
    if r <= 63:
        ones = h64[:, 63]
        bad = ones != 1.0
        if bad.any():
            i = int(torch.nonzero(bad)[0])
            raise NumericsError(f"{name}: column 63 is not 1.0 in {int(bad.sum())} rows (first row {i}: {float(ones[i])})")
    return stats


def gemm_epilogue(prod: torch.Tensor, alpha: float, beta: float, c0=None, bias=None) -> torch.Tensor:
    """The fp32 epilogue of sow_gemm (C = alpha * acc + beta * C0 + bias): three fp32 roundings, each at most u of the sum
    of the operand magnitudes."""
    t = abs(alpha) * to64(prod).abs()
    if c0 is not None:
        t = t + abs(beta) * to64(c0).abs()
    if bias is not None:
        t = t + to64(bias).abs()
    return 3 * UNIT_ROUNDOFF[torch.float32] * t


def gemm_f32_bound(ref: torch.Tensor, sq: torch.Tensor, prod: torch.Tensor, K: int, epi: torch.Tensor) -> torch.Tensor:
    """fp32 sow_gemm (gemm_x3's 3 x bf16 split with six plane products, or the fp32 generic kernel): one fp32 ulp, the
    accumulation term of K fp32 running sums (as chain3f's planes, test_numerics_cpu.py: mm3f) and the epilogue.  A running
    sum errs by sum_k delta_k S_k over its partial sums S_k; those follow the drift of the result as well as the
    fluctuation of the terms: S_k ~ (k / K) prod + noise, so sum_k S_k^2 <= K (sq + prod^2 / 3) up to the noise -- the
    drift term matters for a large |prod| (a long generic fp32 chain: K = 730 at a 3-sigma element)."""
    return bound(ref, torch.float32, accumulation_term(sq + to64(prod) ** 2 / 3, UNIT_ROUNDOFF[torch.float32], K), epi)


def check_gaps(buf: torch.Tensor, live: torch.Tensor, sentinel: float, name: str = "out"):
    """Every element of an output buffer outside the live view (guards, the ldc gaps of a strided C) still holds the
    sentinel."""
    bad = (buf != sentinel) & ~live
    if bad.any():
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise NumericsError(f"{name}: {int(bad.sum())} elements outside the view overwritten (first at flat index {i})")
