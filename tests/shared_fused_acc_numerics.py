"""Cases, the float64 check and a CPU emulation of the shared-input data gradient of siblings that carry a low-rank
accumulator (sow_backward_shared under SOW_FUSE_ACC, chain_shared_acc.hip) -- a plain module shared by
tests/test_gpu_shared_fused_acc.py and tests/test_shared_fused_acc_cpu.py.

The contract: products and sums in fp32, u = the compute dtype's rounding, siblings i = 0 .. n - 1 on one input,
    dh_acc_i = rn(dY_i R_i^T),  dh_live_i = rn(s_i dY_i B_i^T),
    dX = rn(grad_beta dX + sum_i (dh_acc_i Q_i^T + dh_live_i A_i^T))
so dX carries ONE output rounding however many siblings there are.  The bound of `check_dx`:
  * one ulp of the reference;
  * the fp32 noise of a sum of sum_i (d_out_i + r_pad_i) terms;
  * the hidden roundings of every dh_acc_i and dh_live_i: independent errors delta_k c_k, |delta_k| <= u, pooled into ONE
    accumulation term lam u sqrt(sum_k c_k^2) over all siblings (numerics.accumulation_term); in f16 the subnormal floor of
    those roundings as well;
  * grad_beta: the epilogue forms acc + grad_beta * dX_old in fp32 before the one rounding: two fp32 roundings of the
    operand magnitudes.
What the bound does not have is an ulp per sibling or per add: the grouped path (one rounded dX_i per sibling, n - 1 rounded
adds) is `emulate(rounds = n)`, and at least one case must reject it (test_shared_fused_acc_cpu.py).
"""
import dataclasses
from typing import List

import torch

import test_gpu_elementwise as E
from numerics import UNIT_ROUNDOFF, accumulation_term, bound, check_bound, fp32_floor, rne, to64

BF16, F16 = torch.bfloat16, torch.float16


@dataclasses.dataclass
class Sib:
    d_out: int
    r: int
    r_acc: int
    s: float = 0.75

    @property
    def r_pad(self):
        return (self.r + self.r_acc + 63) // 64 * 64


@dataclasses.dataclass
class Set:
    name: str
    dtype: torch.dtype
    T: int
    d_in: int
    sibs: List[Sib]
    grad_beta: float = 0.0
    seed: int = 0


# T just above 8192 (the admission threshold) with a ragged last token block; the smallest widths that reach each edge
CASES = [
    # r_pad of 128, 128 and 64; the live columns of the first sibling straddle a panel boundary (columns 50 .. 99)
    Set("mixed_rpad", BF16, 8257, 264, [Sib(264, 50, 50), Sib(72, 16, 100, s=0.5), Sib(136, 2, 62, s=1.0)]),
    # sum of r_pad = 512, f16
    Set("sum512_f16", F16, 8193, 72, [Sib(520, 50, 200), Sib(264, 50, 200, s=0.5)]),
    # sum of r_pad = 768: three siblings of r_pad = 256 (136 KiB of LDS); r = 64 has no ones column in dh
    Set("sum768", BF16, 8200, 520, [Sib(264, 64, 192), Sib(72, 50, 200, s=0.5), Sib(72, 56, 200)]),
    # four tiny siblings, grad_beta = 1 onto a non-zero dX
    Set("four_tiny_beta", BF16, 8193, 8, [Sib(24, 2, 2), Sib(24, 2, 2, s=0.5), Sib(24, 2, 2, s=1.0), Sib(24, 2, 2)],
        grad_beta=1.0),
    # the largest set the LDS plan admits: r_pad 256, 256, 256, 192 = 15 panels, 120 + 40 = exactly 160 KiB
    Set("lds_max_15_panels", BF16, 8193, 72, [Sib(72, 64, 192), Sib(72, 50, 200, s=0.5), Sib(136, 56, 200), Sib(72, 2, 190, s=1.0)]),
]


def inputs(st: Set):
    """x, per-sibling A, B, Q, R, dy (CPU tensors of the set's dtype), dx0 (grad_beta != 0: what dX holds before the call)."""
    g = torch.Generator().manual_seed(4000 + st.seed + st.T + st.d_in)

    def rnd(*shape, std=1.0):
        return (torch.randn(*shape, generator=g) * std).to(st.dtype)

    d = dict(x=rnd(st.T, st.d_in), sibs=[])
    for sb in st.sibs:
        d["sibs"].append(dict(A=rnd(st.d_in, sb.r, std=0.05), B=rnd(sb.r, sb.d_out, std=0.05),
                              Q=rnd(st.d_in, sb.r_acc, std=0.05), R=rnd(sb.r_acc, sb.d_out, std=0.05), dy=rnd(st.T, sb.d_out)))
    # of the size of the sum it is added to: the rounding of the sum shows
    d["dx0"] = rnd(st.T, st.d_in, std=0.02) if st.grad_beta else None
    return d


def dx_reference(st: Set, d):
    """(ref, bound) of dX in float64 (see the module docstring)."""
    dt, u, u32 = st.dtype, UNIT_ROUNDOFF[st.dtype], UNIT_ROUNDOFF[torch.float32]
    ref = torch.zeros(st.T, st.d_in, dtype=torch.float64)
    sq, hidden, sub = torch.zeros_like(ref), torch.zeros_like(ref), torch.zeros(st.d_in, dtype=torch.float64)
    n_terms = 0
    for sb, p in zip(st.sibs, d["sibs"]):
        A, B, Q, R, dy = (to64(p[k]) for k in ("A", "B", "Q", "R", "dy"))
        AA, QQ, RR = A * A, Q * Q, R * R
        dh, tb = sb.s * (dy @ B.t()), dy @ R.t()
        ref += dh @ A.t() + tb @ Q.t()
        hid = (dh * dh) @ AA.t() + (tb * tb) @ QQ.t()       # what the rounded dh_live_i and dh_acc_i are multiplied into
        hidden += hid
        sq += (dh * dh) @ AA.t() + (dy * dy) @ RR.t() @ QQ.t()
        sub += AA.sum(1) + QQ.sum(1)
        n_terms += sb.d_out + sb.r_pad
    terms = [accumulation_term(hidden, u), fp32_floor(sq, n_terms)]
    if dt == F16:
        terms.append(E._sub_term(sub[None, :].expand(st.T, -1), dt))
    if st.grad_beta:
        old = st.grad_beta * to64(d["dx0"])
        terms.append(2 * u32 * (ref.abs() + old.abs()))
        ref = ref + old
    return ref, bound(ref, dt, *terms)


def check_dx(st: Set, d, dx, name="dX"):
    """|dx - ref64| within the single-rounding bound at every element; returns the statistics (worst err / bound)."""
    ref, bnd = dx_reference(st, d)
    return check_bound(dx, ref, bnd, name=f"{st.name}: {name}")


def emulate(st: Set, d, mm=None, rounds=1):
    """The contract on the CPU, the roundings by numerics.rne (one step from float64).  mm: the product (default: float64
    matmul; pass an fp32 one to include the accumulation noise).  rounds = 1: the contract.  rounds = n (the number of
    siblings): the grouped path instead -- every sibling's dX_i rounded on its own (the single fused pass), then summed
    last sibling first with one rounding per add, as _SoWGroupFunction._input_grad does; grad_beta is one more rounded add.
    Returns dict(dx, dh = [dh_i [T, 64] in the r <= 64 contract])."""
    mm = mm or (lambda a, b: a @ b)
    dt, n = st.dtype, len(st.sibs)
    assert rounds in (1, n)
    parts, dhs = [], []
    for sb, p in zip(st.sibs, d["sibs"]):
        A, B, Q, R, dy = (to64(p[k]) for k in ("A", "B", "Q", "R", "dy"))
        ha, hl = rne(mm(dy, R.t()), dt), rne(sb.s * mm(dy, B.t()), dt)
        parts.append(mm(torch.cat([ha, hl], 1), torch.cat([Q.t(), A.t()], 0)))
        h = torch.zeros(st.T, 64, dtype=torch.float64)
        h[:, :sb.r] = hl
        if sb.r < 64:
            h[:, 63] = 1.0
        dhs.append(h)
    old = st.grad_beta * to64(d["dx0"]) if st.grad_beta else 0.0
    if rounds == 1:
        total = parts[0]
        for part in parts[1:]:
            total = total + part
        return dict(dx=rne(total + old, dt), dh=dhs)
    each = [rne(part, dt) for part in parts]
    total = each[-1]
    for e in reversed(each[:-1]):
        total = rne(total + e, dt)
    if st.grad_beta:
        total = rne(total + old, dt)
    return dict(dx=total, dh=dhs)
