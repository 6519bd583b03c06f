"""float64 reference of the device gradient record (include/sow_amd.h: sow_grad_stats) and of the clipped AdamW step it
drives: a plain module next to step_numerics.py, imported by test_grad_stats_cpu.py (which holds it against
torch.nn.utils.clip_grad_norm_) and by test_gpu_grad_stats.py (which holds the kernels against it).
"""
from __future__ import annotations

import math

import torch


def sumsq(tensors) -> float:
    """Sum over all tensors of the float64 squares of the stored values, summed in float64."""
    if isinstance(tensors, torch.Tensor):
        tensors = [tensors]
    return float(sum(float(t.detach().double().square().sum()) for t in tensors))


def sumsq_bound(n: int, ref: float) -> float:
    """|any-order float64 sum of n non-negative doubles - another one| <= n 2^-52 ref: each is within (n - 1) 2^-53 of the
    true sum (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2) and the squares are exact."""
    return max(n, 1) * 2.0 ** -52 * ref


def record(sq: float, *, grad_scale: float = 1.0, loss_scale: float = 1.0, max_norm=None, extra_sq: float = 0.0,
           found_inf: float = 0.0) -> dict:
    """Every field of the record from the squared norm `sq` of the flat buffer, in Python doubles."""
    mult0 = grad_scale / loss_scale
    total_sq = mult0 * mult0 * sq + extra_sq
    norm = math.sqrt(total_sq) if total_sq >= 0 and math.isfinite(total_sq) else (math.inf if total_sq > 0 else math.nan)
    clip = 1.0
    if max_norm is not None and 0.0 < max_norm < math.inf and math.isfinite(norm):
        clip = min(1.0, max_norm / (norm + 1e-6))
    return dict(sumsq=sq, total_sq=total_sq, total_norm=norm, clip_coef=clip, grad_mult=mult0 * clip,
                nonfinite=int(not math.isfinite(total_sq) or found_inf != 0.0))


def clip_ref(grads, max_norm, **kw) -> dict:
    """record() of a list of gradient tensors taken as one vector (torch.nn.utils.clip_grad_norm_'s global 2-norm)."""
    return record(sumsq(grads), max_norm=max_norm, **kw)


def f32_ulp(x: float) -> float:
    """The spacing of fp32 at the float64 `x`: 2^(e - 23) for 2^e <= |x| < 2^(e + 1), the subnormal spacing below 2^-126."""
    _, e = math.frexp(abs(x))                # |x| = m 2^e with 0.5 <= m < 1, so 2^(e - 1) <= |x| < 2^e
    return 2.0 ** (max(e - 1, -126) - 23)


def within_f32_ulps(got: float, want: float, ulps: float = 1.0) -> bool:
    """got (an fp32 value) within `ulps` fp32 ulps -- the real spacing at `want`, not 2^-23 |want| -- of the float64 `want`."""
    if want == 0.0:
        return got == 0.0
    return abs(got - want) <= ulps * f32_ulp(want)
