"""Quantised storage of frozen dense accumulators: the quantiser and the module conversions (a format is described once, in
acc_format.py; format-specific here: the rounding to a code, _ROUND).  FP8 (OCP E4M3, SOW_ACC_DENSE_FP8): the dense accumulator that
prepare_sow leaves is the largest tensor of a finetune and is never trained; it is stored as one byte per element, one exponent per column:

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
from .acc_format import FORMATS, AccFormat
from .layer import SoWLinear


def _round_e2m1(a: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """Packed E2M1 codes (rows k, k + 1 of a column in one byte): a comparison against the seven midpoints, ties to the even code."""
    mag = a.abs()
    # code c has value v_c = (0, .5, 1, 1.5, 2, 3, 4, 6); the midpoint above an even code belongs to it, the one above an odd
    # code to the next
    q = torch.zeros_like(mag, dtype=torch.uint8)
    for mid, up_on_tie in ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False)):
        q += (mag >= mid) if up_on_tie else (mag > mid)
    q |= torch.signbit(W.detach()).to(torch.uint8) << 3          # the sign of W itself: -0 stays -0
    return q[0::2] | (q[1::2] << 4)


# the one rounding of a scaled, clamped float64 value `a` to a code (E4M3: float64 -> float32 is exact here, then to nearest even)
_ROUND = {"fp8_e4m3": lambda a, W: a.to(torch.float32).to(torch.float8_e4m3fn), "mxfp4": _round_e2m1}


def quantize_tensor(W: torch.Tensor, fmt: str = "fp8_e4m3") -> Tuple[torch.Tensor, torch.Tensor]:
    """(codes, scales) of a bf16 / f16 matrix [d_in, d_out] in the format `fmt` (acc_format.py), on W's device, with plain torch
    ops (a one-off).  The arithmetic is float64, where every step before the one rounding to a code is exact: |W| has at most
    11 significant bits, the scale is a power of two, and no subnormal of the narrower formats is involved."""
    f = FORMATS.get(fmt)
    if f is None:
        raise ValueError(f"sow_amd.quantize_tensor: format {fmt!r} is not supported ({', '.join(FORMATS)})")
    if W.dtype not in f.exp_range:
        raise TypeError(f"sow_amd.quantize_tensor: a bfloat16 or float16 matrix, got {W.dtype}")
    if W.dim() != 2 or W.shape[0] % (f.block or 1):
        raise ValueError("sow_amd.quantize_tensor: a 2-D matrix [d_in, d_out]" + (f" with d_in a multiple of {f.block}" if f.block else ""))
    if not bool(torch.isfinite(W).all()):
        raise ValueError("sow_amd.quantize_tensor: the accumulator holds non-finite values")
    (lo, hi), (t, o), (d_in, d_out) = f.exp_range[W.dtype], f.frexp, W.shape
    rows = f.block or d_in                      # one scale per block of a column: the whole column without blocks
    w = W.detach().to(torch.float64).reshape(d_in // rows if rows else 1, rows, d_out)
    amax = w.abs().amax(dim=1) if rows else w.new_zeros(1, d_out)
    # amax = m * 2^x with m in [0.5, 1), code_max = t * 2^o:  amax <= code_max * 2^e  <=>  e >= x - o (m <= t) or x - o + 1
    m, x = torch.frexp(amax)
    e = x.to(torch.int64) - o + (m > t).to(torch.int64)
    e = torch.where(amax == 0, torch.zeros_like(e), e).clamp_(lo, hi)
    a = (w * torch.exp2(-e.to(torch.float64)).unsqueeze(1)).clamp_(-f.code_max, f.code_max).reshape(d_in, d_out)
    return _ROUND[fmt](a, W).contiguous(), (e + f.scale_bias).to(f.scale_dtype).reshape(f.scale_shape(d_in, d_out)).contiguous()


def _quantizable(m: SoWLinear, f: AccFormat) -> bool:
    acc = m.acc_downweight
    return (not m.acc_quantized() and acc.numel() != 0 and m.acc_upweight.numel() == 0 and acc.dtype in f.exp_range
            and tuple(acc.shape) == (m.in_features, m.out_features) and m.in_features % f.d_in_multiple == 0
            and m.out_features % f.d_out_multiple == 0)


def quantize_accumulators(model: nn.Module, fmt: str = "fp8_e4m3", strict: bool = False) -> int:
    """Store every dense bf16 / f16 accumulator of `model` whose widths the format admits as codes of `fmt` (acc_format.py):
    acc_downweight becomes a frozen parameter of the code dtype, the scales the persistent buffer acc_exponent (the state dict
    carries both).  Other SoWLinear layers -- no accumulator, a low-rank one, fp32, ragged widths, already quantised -- are left
    alone, or raise ValueError under strict=True.  Returns the number converted.  Quantise in the dtype the model will run in."""
    if fmt not in FORMATS:
        raise ValueError(f"sow_amd.quantize_accumulators: format {fmt!r} is not supported ({', '.join(FORMATS)})")
    f, n = FORMATS[fmt], 0
    for name, m in model.named_modules():
        if not isinstance(m, SoWLinear):
            continue
        if not _quantizable(m, f):
            if strict:
                raise ValueError(f"sow_amd.quantize_accumulators(strict=True): layer {name!r} has no dense bfloat16 / float16 accumulator "
                                 f"with in_features a multiple of {f.d_in_multiple} and out_features of {f.d_out_multiple}")
            continue
        codes, exps = quantize_tensor(m.acc_downweight.data, fmt)
        m.acc_downweight = nn.Parameter(codes, requires_grad=False)
        m.register_buffer("acc_exponent", exps, persistent=True)
        n += 1
    return n


def dequantize_accumulators(model: nn.Module) -> int:
    """The inverse storage change: every quantised layer gets W^ back as a frozen parameter of its factors' dtype and loses
    the acc_exponent buffer (W^, not the matrix that was quantised).  Returns the number of layers converted."""
    n = 0
    for m in model.modules():
        if isinstance(m, SoWLinear) and m.acc_quantized():
            dtype = m.downscale_weights._parameters["0"].dtype
            w = ops.acc_dequantize(m.acc_downweight.data, m.acc_exponent, dtype)
            del m._buffers["acc_exponent"]
            m.acc_downweight = nn.Parameter(w, requires_grad=False)
            n += 1
    return n
