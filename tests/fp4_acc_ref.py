"""An integer reference of the MXFP4 accumulator format (include/sow_amd.h: SOW_ACC_DENSE_FP4) -- a plain module, imported by
test_fp4_acc_cpu.py and test_gpu_fp4_acc.py.  It works on the BIT PATTERNS of bf16 / f16 with integer arithmetic only (torch
int64 tensors and Python ints): no floating operation, no torch cast and no library call enters a result.

    |w|      = M * 2^E            M the significand with its hidden bit, from the fields of the bit pattern
    e[kb,n]  = the smallest integer with max_{k in block} |W[k,n]| <= 6 * 2^e  (blocks of 32 rows of a column), clamped to
               EXP_RANGE[dtype]; 0 for an all-zero block; stored as the byte e + 127
    q[k,n]   = the E2M1 code nearest to min(|w| * 2^-e, 6), ties to the even code, with the sign bit of w
    codes    = q[k,n] | q[k+1,n] << 4  for even k
    W^       = value(q) * 2^e     as a bit pattern of the dtype (always a normal number or a signed zero)
"""
from __future__ import annotations

import torch

BLOCK = 32
EXP_RANGE = {torch.bfloat16: (-125, 125), torch.float16: (-13, 13)}
# (mantissa bits, exponent bias, exponent-field mask)
_FIELDS = {torch.bfloat16: (7, 127, 0xFF), torch.float16: (10, 15, 0x1F)}
# the code magnitudes in units of 1/2, and the seven midpoints in units of 1/4 with "a tie goes up" (to the even code above)
VALUES_X2 = (0, 1, 2, 3, 4, 6, 8, 12)
MIDPOINTS_X4 = ((1, False), (3, True), (5, False), (7, True), (10, False), (14, True), (20, False))


def bits_of(W: torch.Tensor) -> torch.Tensor:
    """The 16-bit patterns of a bf16 / f16 tensor as non-negative int64."""
    return W.detach().cpu().contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def fields(bits: torch.Tensor, dtype):
    """(sign, M, E) with |w| = M * 2^E, M an integer (0 for zero); raises on Inf / NaN."""
    mb, bias, emask = _FIELDS[dtype]
    sign = bits >> 15
    ef = (bits >> mb) & emask
    mf = bits & ((1 << mb) - 1)
    if bool((ef == emask).any()):
        raise ValueError("non-finite accumulator")
    normal = ef > 0
    M = torch.where(normal, mf + (1 << mb), mf)
    E = torch.where(normal, ef, torch.ones_like(ef)) - bias - mb
    return sign, M, E


def _bit_length(M: torch.Tensor) -> torch.Tensor:
    L = torch.zeros_like(M)
    for j in range(12):
        L += (M >= (1 << j)).to(torch.int64)
    return L


def block_exponent_of(M: int, E: int, dtype) -> int:
    """The clamped block exponent of amax = M * 2^E (Python ints): the definition itself, by integer comparison."""
    lo, hi = EXP_RANGE[dtype]
    if M == 0:
        return 0
    # amax <= 6 * 2^e  <=>  M * 2^E <= 6 * 2^e: search the smallest e from well below
    e = E - 4
    while not _le_6_2e(M, E, e):
        e += 1
    assert not _le_6_2e(M, E, e - 1)
    return max(lo, min(hi, e))


def _le_6_2e(M: int, E: int, e: int) -> bool:
    return (M << (E - e)) <= 6 if E >= e else M <= (6 << (e - E))


def block_exponents(bits: torch.Tensor, dtype) -> torch.Tensor:
    """e [d_in / 32, d_out] int64 (clamped), vectorised: amax = m * 2^x with m in [0.5, 1): e = x - 3 if m <= 0.75 else x - 2."""
    lo, hi = EXP_RANGE[dtype]
    d_in, d_out = bits.shape
    assert d_in % BLOCK == 0
    mag = (bits & 0x7FFF).view(d_in // BLOCK, BLOCK, d_out).amax(dim=1)       # magnitudes order as their bit patterns
    _, M, E = fields(mag, dtype)
    L = _bit_length(M)                                                       # 2^(L-1) <= M < 2^L: x = L + E, m = M / 2^L
    e = L + E - 3 + (4 * M > 3 * (torch.ones_like(M) << L)).to(torch.int64)
    return torch.where(M == 0, torch.zeros_like(e), e).clamp(lo, hi)


def quantize(W: torch.Tensor):
    """(packed codes uint8 [d_in / 2, d_out], scale bytes uint8 [d_in / 32, d_out]) of a bf16 / f16 matrix."""
    dtype = W.dtype
    bits = bits_of(W)
    sign, M, E = fields(bits, dtype)
    e = block_exponents(bits, dtype)
    s = E - e.repeat_interleave(BLOCK, dim=0) + 2                # |w| * 2^-e in units of 1/4 = M * 2^s
    # M < 2^11: past a shift of 16 the left side exceeds every midpoint, past -40 every midpoint exceeds it
    lhs = M << s.clamp(0, 16)
    down = (-s).clamp(0, 40)
    q = torch.zeros_like(M)
    for t, up_on_tie in MIDPOINTS_X4:
        rhs = torch.full_like(M, t) << down
        q += ((lhs > rhs) | ((lhs == rhs) & up_on_tie)).to(torch.int64)
    q = q | (sign << 3)
    codes = q[0::2] | (q[1::2] << 4)
    return codes.to(torch.uint8), (e + 127).to(torch.uint8)


def unpack(codes: torch.Tensor) -> torch.Tensor:
    """q [d_in, d_out] int64 (4-bit codes) of packed codes [d_in / 2, d_out]."""
    c = codes.cpu().to(torch.int64)
    q = torch.empty((2 * c.shape[0], c.shape[1]), dtype=torch.int64)
    q[0::2], q[1::2] = c & 15, c >> 4
    return q


def dequantize_bits(codes: torch.Tensor, scales: torch.Tensor, dtype) -> torch.Tensor:
    """The bit patterns (int16) of W^ [d_in, d_out] in `dtype`; view(dtype) gives the image.  Code magnitude c >= 2 is
    (1 + (c & 1) / 2) * 2^((c >> 1) - 1), c = 1 is 2^-1, c = 0 is zero: exponent field and top mantissa bit, no arithmetic on
    values."""
    mb, bias, emask = _FIELDS[dtype]
    q = unpack(codes)
    e = scales.cpu().to(torch.int64).repeat_interleave(BLOCK, dim=0) - 127
    c, sign = q & 7, q >> 3
    p = torch.where(c >= 2, (c >> 1) - 1, torch.full_like(c, -1))
    ef = p + e + bias
    mant = torch.where(c >= 2, (c & 1) << (mb - 1), torch.zeros_like(c))
    out = torch.where(c == 0, torch.zeros_like(c), (ef << mb) | mant)
    nz = c != 0
    if bool(nz.any()):
        assert int(ef[nz].min()) >= 1 and int(ef[nz].max()) < emask, "W^ leaves the normal range: the scale is outside the clamps"
    out = out | (sign << 15)
    return torch.where(out >= 0x8000, out - 0x10000, out).to(torch.int16)


def dequantize(codes: torch.Tensor, scales: torch.Tensor, dtype) -> torch.Tensor:
    """W^ as a CPU tensor of `dtype` (a view of the bit patterns)."""
    return dequantize_bits(codes, scales, dtype).view(dtype)
