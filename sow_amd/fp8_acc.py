"""FP8 (OCP E4M3) storage of frozen dense accumulators -- include/sow_amd.h: SOW_ACC_DENSE_FP8.

The dense accumulator that prepare_sow leaves on a pretrained model (and commonsense_evaluate.py reloads for generate()) is
the largest tensor of a finetune and is never trained.  `quantize_accumulators(model)` stores it as one byte per element with
one power-of-two exponent per output column:

    e_n    = the smallest integer with max_k |W[k, n]| <= 448 * 2^e_n   (frexp, exact), clamped to [-117, 119] for bfloat16
             and [-15, 7] for float16; 0 for an all-zero column
    q[k,n] = e4m3fn_rne(clamp(W[k, n] * 2^-e_n, -448, 448))             (the scaling is exact; the clamp keeps the NaN codes out)
    W^     = q * 2^e                                                     exactly a number of the compute dtype

Every kernel path computes what it computes for a dense accumulator, on W^: no-grad calls of at most 32 tokens stream the
codes themselves (skinny_fwd.hip: half the bytes), every other call -- larger inputs, training, the backward -- runs the
existing dense path on the image that one streaming pass writes into a scratch arena (ops.acc_images).  Autograd saves the
codes, never the image.  `|W^ - W| <= 2^-4 |W| + 2^(e_n - 10)`: half an E4M3 ulp, relative for normal codes, absolute below.

`quantize_accumulators(model, fmt="mxfp4")` (SOW_ACC_DENSE_FP4) stores it as MXFP4 instead -- 0.53 bytes per element:

    e[kb,n] = the smallest integer with max_{k in block kb} |W[k, n]| <= 6 * 2^e  (blocks of 32 consecutive rows of one column),
              clamped to [-125, 125] for bfloat16 and [-13, 13] for float16; 0 for an all-zero block; stored as the byte e + 127
    q[k,n]  = e2m1_rne(clamp(W[k, n] * 2^-e, -6, 6))   one of +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the even code, sign kept
    codes   = q[k, n] | q[k + 1, n] << 4 for even k     uint8 [d_in / 2, d_out]
    W^      = q * 2^e                                    exactly a normal number (or zero) of the compute dtype

with the same dispatch and `|W^ - W| <= 2^-2 |W| + 2^(e - 2)`.
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn as nn

from . import ops
from .layer import SoWLinear

E4M3_MAX = 448.0
EXP_RANGE = {torch.bfloat16: (-117, 119), torch.float16: (-15, 7)}
FORMATS = ("fp8_e4m3", "mxfp4")
E2M1_MAX = 6.0
FP4_BLOCK = ops.FP4_BLOCK
FP4_EXP_RANGE = {torch.bfloat16: (-125, 125), torch.float16: (-13, 13)}


def quantize_tensor(W: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(codes [d_in, d_out] float8_e4m3fn, exponents [d_out] int8) of a bf16 / f16 matrix, on W's device, with plain torch
    ops (a one-off).  The arithmetic is float64, where every step before the one E4M3 rounding is exact: |W| has at most 11
    significant bits, the scale is a power of two, and no subnormal of the narrower formats is involved."""
    if W.dtype not in EXP_RANGE:
        raise TypeError(f"sow_amd.quantize_tensor: a bfloat16 or float16 matrix, got {W.dtype}")
    if W.dim() != 2:
        raise ValueError("sow_amd.quantize_tensor: a 2-D matrix [d_in, d_out]")
    if not bool(torch.isfinite(W).all()):
        raise ValueError("sow_amd.quantize_tensor: the accumulator holds non-finite values")
    lo, hi = EXP_RANGE[W.dtype]
    w = W.detach().to(torch.float64)
    amax = w.abs().amax(dim=0) if w.shape[0] else w.new_zeros(w.shape[1])
    # amax = m * 2^x with m in [0.5, 1), 448 = 0.875 * 2^9:  amax <= 448 * 2^e  <=>  e >= x - 9 (m <= 0.875) or x - 8
    m, x = torch.frexp(amax)
    e = x.to(torch.int64) - 9 + (m > 0.875).to(torch.int64)
    e = torch.where(amax == 0, torch.zeros_like(e), e).clamp_(lo, hi)
    scaled = (w * torch.exp2(-e.to(torch.float64))).clamp_(-E4M3_MAX, E4M3_MAX)
    codes = scaled.to(torch.float32).to(ops.FP8)     # float64 -> float32 is exact here; ONE rounding, to nearest even
    return codes.contiguous(), e.to(torch.int8)


def quantize_tensor_fp4(W: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(packed codes [d_in / 2, d_out] uint8, E8M0 block scales [d_in / 32, d_out] uint8) of a bf16 / f16 matrix with d_in a
    multiple of 32, on W's device, with plain torch ops (a one-off).  The arithmetic is float64, where every step before the
    one E2M1 rounding is exact; the rounding itself is a comparison against the seven midpoints, ties to the even code."""
    if W.dtype not in FP4_EXP_RANGE:
        raise TypeError(f"sow_amd.quantize_tensor_fp4: a bfloat16 or float16 matrix, got {W.dtype}")
    if W.dim() != 2 or W.shape[0] % FP4_BLOCK:
        raise ValueError("sow_amd.quantize_tensor_fp4: a 2-D matrix [d_in, d_out] with d_in a multiple of 32")
    if not bool(torch.isfinite(W).all()):
        raise ValueError("sow_amd.quantize_tensor_fp4: the accumulator holds non-finite values")
    lo, hi = FP4_EXP_RANGE[W.dtype]
    d_in, d_out = W.shape
    w = W.detach().to(torch.float64).view(d_in // FP4_BLOCK, FP4_BLOCK, d_out)
    amax = w.abs().amax(dim=1)
    # amax = m * 2^x with m in [0.5, 1), 6 = 0.75 * 2^3:  amax <= 6 * 2^e  <=>  e >= x - 3 (m <= 0.75) or x - 2
    m, x = torch.frexp(amax)
    e = x.to(torch.int64) - 3 + (m > 0.75).to(torch.int64)
    e = torch.where(amax == 0, torch.zeros_like(e), e).clamp_(lo, hi)
    a = (w * torch.exp2(-e.to(torch.float64)).unsqueeze(1)).clamp_(-E2M1_MAX, E2M1_MAX).view(d_in, d_out)
    mag = a.abs()
    # code c has value v_c = (0, .5, 1, 1.5, 2, 3, 4, 6); the midpoint above an even code belongs to it, the one above an odd
    # code to the next
    q = torch.zeros_like(mag, dtype=torch.uint8)
    for mid, up_on_tie in ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False)):
        q += (mag >= mid) if up_on_tie else (mag > mid)
    q |= torch.signbit(W.detach()).to(torch.uint8) << 3          # the sign of W itself: -0 stays -0
    codes = q[0::2] | (q[1::2] << 4)
    return codes.contiguous(), (e + 127).to(torch.uint8).contiguous()


def _quantizable(m: SoWLinear, fmt: str = "fp8_e4m3") -> bool:
    acc = m.acc_downweight
    return (not m.acc_quantized() and acc.numel() != 0 and m.acc_upweight.numel() == 0 and acc.dtype in EXP_RANGE
            and tuple(acc.shape) == (m.in_features, m.out_features) and m.in_features % (FP4_BLOCK if fmt == "mxfp4" else 8) == 0
            and m.out_features % 8 == 0)


def quantize_accumulators(model: nn.Module, fmt: str = "fp8_e4m3", strict: bool = False) -> int:
    """Store every dense bf16 / f16 accumulator of `model` whose widths are multiples of 8 as E4M3 codes: acc_downweight
    becomes a frozen float8_e4m3fn parameter, the int8 column exponents go to the persistent buffer acc_exponent (so the state
    dict carries both).  Other SoWLinear layers -- no accumulator, a low-rank one, fp32, ragged widths, already quantised --
    are left alone, or raise ValueError under strict=True.  Returns the number of layers converted.  Quantise in the dtype
    the model will run in: the exponent clamps are those of the accumulator's dtype.
    fmt="mxfp4": packed E2M1 codes (a frozen uint8 parameter [d_in / 2, d_out]) and E8M0 block scales (acc_exponent, uint8
    [d_in / 32, d_out]); in_features must then be a multiple of 32."""
    if fmt not in FORMATS:
        raise ValueError(f"sow_amd.quantize_accumulators: format {fmt!r} is not supported ({', '.join(FORMATS)})")
    n = 0
    for name, m in model.named_modules():
        if not isinstance(m, SoWLinear):
            continue
        if not _quantizable(m, fmt):
            if strict:
                raise ValueError(f"sow_amd.quantize_accumulators(strict=True): layer {name!r} has no dense bfloat16 / float16 "
                                 "accumulator with widths that are multiples of 8" + (" (in_features of 32)" if fmt == "mxfp4" else ""))
            continue
        codes, exps = (quantize_tensor_fp4 if fmt == "mxfp4" else quantize_tensor)(m.acc_downweight.data)
        m.acc_downweight = nn.Parameter(codes, requires_grad=False)
        m.register_buffer("acc_exponent", exps, persistent=True)
        n += 1
    return n


def dequantize_tensor(codes: torch.Tensor, exps: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """W^ = codes * 2^exps in `dtype` (bf16 / f16), exactly, as a new tensor (the library's streaming pass), for E4M3 codes with
    int8 column exponents and for packed MXFP4 codes with uint8 block scales."""
    return ops.acc_dequantize(codes, exps, dtype)


def dequantize_accumulators(model: nn.Module) -> int:
    """The inverse storage change: every quantised layer gets W^ back as a frozen parameter of its factors' dtype and loses
    the acc_exponent buffer (W^, not the matrix that was quantised).  Returns the number of layers converted."""
    n = 0
    for m in model.modules():
        if isinstance(m, SoWLinear) and m.acc_quantized():
            dtype = m.downscale_weights._parameters["0"].dtype
            w = dequantize_tensor(m.acc_downweight.data, m.acc_exponent, dtype)
            del m._buffers["acc_exponent"]
            m.acc_downweight = nn.Parameter(w, requires_grad=False)
            n += 1
    return n
