"""A float64 / integer reference of the E4M3 accumulator format (include/sow_amd.h: SOW_ACC_DENSE_FP8) -- a plain module,
imported by test_fp8_acc_cpu.py and test_gpu_fp8_acc.py.  Nothing here touches torch's float8 casts or the library: the code
table comes from the bit fields, the exponent from integer comparisons, the rounding from a search in the table.

    e_n    = the smallest integer with amax_n <= 448 * 2^e_n, clamped to EXP_RANGE[dtype]; 0 for an all-zero column
    q[k,n] = the E4M3 code nearest to clamp(W[k,n] * 2^-e_n, -448, 448), ties to the even code
    W^     = value(q) * 2^e
"""
from __future__ import annotations

import math

import torch

E4M3_MAX = 448.0
EXP_RANGE = {torch.bfloat16: (-117, 119), torch.float16: (-15, 7)}
NAN_CODES = (0x7F, 0xFF)


def code_value(c: int) -> float:
    """The value of code c (0 .. 255) from its fields: sign, 4 exponent bits (bias 7), 3 mantissa bits; S.1111.111 is NaN."""
    s, e, m = c >> 7, (c >> 3) & 15, c & 7
    if e == 15 and m == 7:
        return math.nan
    v = (m / 8.0) * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
    return -v if s else v


TABLE = torch.tensor([code_value(c) for c in range(256)], dtype=torch.float64)
# the non-negative finite values, ascending: code i has value POS[i] for i = 0 .. 126
POS = TABLE[:127].clone()


def column_exponent(amax: float, dtype: torch.dtype) -> int:
    """The smallest integer e with amax <= 448 * 2^e (amax a finite float, exact arithmetic on its frexp form), clamped."""
    lo, hi = EXP_RANGE[dtype]
    if amax == 0:
        return 0
    m, x = math.frexp(amax)                     # amax = m * 2^x, 0.5 <= m < 1;  448 = 0.875 * 2^9
    e = x - 9 if m <= 0.875 else x - 8
    # the definition, checked with exact power-of-two scalings
    assert amax <= math.ldexp(448.0, e) and amax > math.ldexp(448.0, e - 1)
    return max(lo, min(hi, e))


def quantize(W: torch.Tensor):
    """(codes uint8 [d_in, d_out], exponents int8 [d_out]) of a bf16 / f16 matrix, on the CPU in float64."""
    dtype = W.dtype
    w = W.detach().cpu().to(torch.float64)
    if not bool(torch.isfinite(w).all()):
        raise ValueError("non-finite accumulator")
    amax = w.abs().amax(dim=0)
    e = torch.tensor([column_exponent(float(a), dtype) for a in amax], dtype=torch.int64)
    v = (w * torch.exp2(-e.to(torch.float64))).clamp(-E4M3_MAX, E4M3_MAX)
    a = v.abs()
    hi = torch.searchsorted(POS, a.contiguous()).clamp(max=126)        # first code with value >= a
    lo = (hi - 1).clamp(min=0)
    d_hi, d_lo = POS[hi] - a, a - POS[lo]
    pick_lo = (d_lo < d_hi) | ((d_lo == d_hi) & (lo % 2 == 0))         # nearest; a tie goes to the even code
    code = torch.where(pick_lo, lo, hi)
    code = code + 128 * ((v < 0) | ((v == 0) & (torch.signbit(v)))).to(torch.int64)
    return code.to(torch.uint8), e.to(torch.int8)


def dequantize(codes: torch.Tensor, exps: torch.Tensor) -> torch.Tensor:
    """W^ in float64 (NaN for the two NaN codes)."""
    return TABLE[codes.cpu().to(torch.int64)] * torch.exp2(exps.cpu().to(torch.float64))


def error_bound(W: torch.Tensor, exps: torch.Tensor) -> torch.Tensor:
    """|W^ - W| <= 2^-4 |W| + 2^(e_n - 10): half an ulp of a normal code (3 mantissa bits) or of the subnormal spacing 2^-9."""
    w = W.detach().cpu().to(torch.float64)
    return w.abs() * 2.0 ** -4 + torch.exp2(exps.cpu().to(torch.float64) - 10)
