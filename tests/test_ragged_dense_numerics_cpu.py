"""CPU emulation of the ragged dense product (gemm_rag.hip): bf16 operands, exact products, an fp32 running sum in the
kernel's k order (ascending k, groups of four consecutive k summed before they join the accumulator), ONE RNE
rounding at the store.  K = 5461 (tail of 21 in the last tile) and K = 2048, N = 93 (ragged).  The groups of four are a
model of the order, not the kernel's instruction: v_mfma_f32_32x32x16 takes 16 k per instruction (8 per lane half) and sums
them inside the unit in an order and precision that is not documented, so the emulation keeps the 4-wide fp32 groups the
rounding statistics of this check were first measured with.  What it fixes is the kind of sum -- short groups joined to
one long fp32 chain in ascending k -- which is what decides the share of elements off RNE(ref64).

The emulation must pass the check the GPU tests hold the kernel to -- numerics.check_rounded with acc = fp32_floor(sq, K)
and the default MAX_INEXACT (0.5 % of the elements not bit-equal to RNE(ref64)); the share it reaches is printed and held
below a tenth of that cap (reached: 0.022 % at K = 5461, worst err / limit 0.13; 0 at K = 2048).  A catalogue of the faults such a kernel can have must be rejected by the same check:

  fault                                                   check_rounded   rel_err < 2e-2 alone
  the K tail (k >= 64 floor(K / 64)) dropped              rejected        rejected (21 of 5461 terms: 0.077)
  the K tail of one operand left unzeroed against a NaN   rejected        rejected (NaN)
  the last column of a ragged N dropped                   rejected        rejected (a whole column at its full size)
  a row read one element off (the realignment bug)        rejected        rejected
  a truncating store                                      rejected        PASSES (0.006: under one bf16 ulp of the largest element)

The last column of the table is asserted as well: it is why the GPU tests compare element by element."""
import pytest
import torch

from conftest import rel_err
from numerics import MAX_INEXACT, NumericsError, check_rounded, fp32_floor, to64

BF16 = torch.bfloat16
M, N = 48, 93


def _operands(K, seed=0):
    g = torch.Generator().manual_seed(seed + K)
    x = torch.randn(M, K, generator=g).to(BF16)
    w = (torch.randn(K, N, generator=g) * 0.02).to(BF16)
    return x, w


def _emulate(x, w, k_end=None, trunc=False):
    """fp32 running sum over k in groups of four (the products are exact in fp32), RNE (or truncating) store to bf16.
    x [M, K], w [K, N] as float32 tensors holding bf16 values (NaN allowed); k_end: terms k >= k_end are left out."""
    K = x.shape[1] if k_end is None else k_end
    acc = torch.zeros(x.shape[0], w.shape[1], dtype=torch.float32)
    for k in range(0, K, 4):
        g = torch.zeros_like(acc)
        for j in range(k, min(k + 4, K)):
            g = g + x[:, j:j + 1] * w[j:j + 1, :]
        acc = acc + g
    if trunc:
        return (acc.view(torch.int32) & -65536).view(torch.float32).to(BF16)
    return acc.to(BF16)


def _check(out, x, w, K):
    x64, w64 = to64(x), to64(w)
    ref = x64 @ w64
    return check_rounded(out, ref, BF16, acc=fp32_floor((x64 * x64) @ (w64 * w64), K), name=f"K = {K}")


@pytest.mark.parametrize("K", [5461, 2048])
def test_emulated_kernel_passes_check_rounded(K):
    x, w = _operands(K)
    st = _check(_emulate(x.float(), w.float()), x, w, K)
    print(f"K = {K}: {100 * st['inexact']:.4f} % of the elements differ from RNE(ref64) (cap {100 * MAX_INEXACT} %), worst "
          f"err / limit {st['worst']:.3f}")
    assert st["inexact"] <= MAX_INEXACT / 10


def _faults(K):
    """name -> (output of the faulty kernel, whether rel_err < 2e-2 alone lets it through)."""
    x, w = _operands(K)
    xf, wf = x.float(), w.float()
    out = {}
    out["k_tail_dropped"] = (_emulate(xf, wf, k_end=K // 64 * 64), False)
    # the last K tile padded to 64: A's padding zeroed, B's holds the neighbour's NaN -- 0 x NaN
    pad = (-K) % 64
    xa = torch.cat([xf, torch.zeros(M, pad)], 1)
    wb = torch.cat([wf, torch.full((pad, N), float("nan"))], 0)
    out["k_tail_unzeroed_vs_nan"] = (_emulate(xa, wb), False)
    good = _emulate(xf, wf)
    dropped = good.clone()
    dropped[:, -1] = 0
    out["last_column_dropped"] = (dropped, False)
    # every row read one element late: row m starts at flat element m K + 1
    flat = torch.cat([xf.reshape(-1), torch.zeros(1)])
    shifted = flat[1:].reshape(M, K)
    out["row_one_element_off"] = (_emulate(shifted, wf), False)
    out["truncating_store"] = (_emulate(xf, wf, trunc=True), True)
    return x, w, out


@pytest.mark.parametrize("fault", ["k_tail_dropped", "k_tail_unzeroed_vs_nan", "last_column_dropped", "row_one_element_off",
                                   "truncating_store"])
def test_fault_is_rejected(fault):
    K = 5461
    x, w, faults = _faults(K)
    bad, rel_passes = faults[fault]
    with pytest.raises(NumericsError):
        _check(bad, x, w, K)
    e = rel_err(bad.float(), to64(x) @ to64(w))
    print(f"{fault}: rel_err {e:.3g}")
    assert (e < 2e-2) == rel_passes, f"{fault}: rel_err = {e}"
