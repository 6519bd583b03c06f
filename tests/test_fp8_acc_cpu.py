"""The E4M3 accumulator format (include/sow_amd.h: SOW_ACC_DENSE_FP8) on the CPU: the float64 / integer reference of
fp8_acc_ref.py against the definitions, and sow_amd's quantiser (plain torch ops, so it runs here) against the reference,
bit for bit.  No GPU, no library call."""
import math

import pytest
import torch

import fp8_acc_ref as R
from sow_amd import acc_quant

BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
_ID = {BF16: "bf16", F16: "f16"}.get
_BITS = {BF16: torch.int16, F16: torch.int16}


def _ulp_up(v: float, dtype) -> float:
    """The next number of `dtype` above v > 0."""
    t = torch.tensor([v], dtype=dtype)
    assert float(t) == v, "not a number of the dtype"
    return float((t.view(torch.int16) + 1).view(dtype))


def _ulp_down(v: float, dtype) -> float:
    t = torch.tensor([v], dtype=dtype)
    assert float(t) == v
    return float((t.view(torch.int16) - 1).view(dtype))


def _both(W):
    """The reference's and the package's quantisation of W, asserted bit-identical; returns the reference's."""
    codes, exps = R.quantize(W)
    q, e = acc_quant.quantize_tensor(W)
    assert q.dtype == torch.float8_e4m3fn and e.dtype == torch.int8 and q.shape == W.shape and e.shape == (W.shape[1],)
    assert torch.equal(e, exps), f"exponents differ: {e[e != exps][:8].tolist()} vs {exps[e != exps][:8].tolist()}"
    bad = q.view(torch.uint8) != codes
    assert not bad.any(), (f"{int(bad.sum())} codes differ; first at {tuple(int(v) for v in torch.nonzero(bad)[0])}: "
                           f"{int(q.view(torch.uint8)[bad][0])} vs {int(codes[bad][0])}")
    return codes, exps


def test_code_table_matches_the_dtype():
    """The table built from the bit fields is torch's float8_e4m3fn, code by code; exactly two codes are NaN."""
    want = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64)
    nan = torch.isnan(R.TABLE)
    assert sorted(torch.nonzero(nan).flatten().tolist()) == sorted(R.NAN_CODES)
    assert torch.equal(torch.isnan(want), nan)
    assert torch.equal(R.TABLE[~nan], want[~nan])
    assert float(R.TABLE[0x7E]) == R.E4M3_MAX and float(R.TABLE[1]) == 2.0 ** -9


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_exponent_on_powers_of_two(dtype):
    lo, hi = R.EXP_RANGE[dtype]
    ks = range(-20, 16) if dtype == F16 else range(-120, 121)
    for k in ks:
        # 2^k <= 448 * 2^e  <=>  e >= k - log2(448): the smallest is k - 8 (448 >= 256 = 2^8, 448 < 512)
        assert R.column_exponent(2.0 ** k, dtype) == max(lo, min(hi, k - 8)), k
    W = torch.tensor([[2.0 ** k for k in ks]], dtype=dtype)
    codes, exps = _both(W)
    assert exps.tolist() == [max(lo, min(hi, k - 8)) for k in ks]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_exponent_at_448_times_a_power_of_two(dtype):
    """amax = 448 * 2^k sits exactly on the bound: e = k, code 0x7E; one ulp above needs e = k + 1, one below keeps k.  A
    log2-based exponent gets one of the three wrong."""
    lo, hi = R.EXP_RANGE[dtype]
    ks = range(-12, 7) if dtype == F16 else range(-100, 100)
    cols, want = [], []
    for k in ks:
        v = 448.0 * 2.0 ** k
        cols += [v, _ulp_up(v, dtype), _ulp_down(v, dtype)]
        want += [k, k + 1, k]
    W = torch.tensor([cols], dtype=dtype)
    codes, exps = _both(W)
    assert exps.tolist() == [max(lo, min(hi, e)) for e in want]
    assert all(int(c) == 0x7E for c in codes[0, 0::3]), "448 * 2^k must be the largest code under e = k"
    assert bool((R.dequantize(codes, exps)[0, 0::3] == W.double()[0, 0::3]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_clamps(dtype):
    """Columns past the exponent range keep the clamped exponent: large ones saturate at +-448 * 2^hi, small ones fall to
    the subnormal codes or to zero -- and no code is NaN."""
    lo, hi = R.EXP_RANGE[dtype]
    big = torch.finfo(dtype).max
    tiny = float(torch.tensor([1], dtype=torch.int16).view(dtype))       # the smallest subnormal
    W = torch.tensor([[big, -big, tiny, -tiny, 448.0 * 2.0 ** hi, 2.0 ** (lo - 9)],
                      [1.0, 1.0, tiny, 0.0, 1.0, 0.0]], dtype=dtype)
    codes, exps = _both(W)
    assert exps.tolist()[:4] == [hi, hi, lo, lo] and exps.tolist()[4:] == [hi, lo]
    if dtype == F16:     # 65504 > 448 * 2^7: the clamp to 448 acts
        assert codes[0].tolist()[:2] == [0x7E, 0xFE]
    assert int(codes[0, 5]) == 1, "2^(lo - 9) is the smallest subnormal code under e = lo"
    assert not any(int(c) in R.NAN_CODES for c in codes.flatten())
    assert bool(torch.isfinite(R.dequantize(codes, exps)).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_zero_columns(dtype):
    g = torch.Generator().manual_seed(3)
    W = (torch.randn(24, 16, generator=g) * 0.02).to(dtype)
    W[:, 3] = 0
    W[:, 7] = -0.0
    codes, exps = _both(W)
    assert int(exps[3]) == 0 and int(exps[7]) == 0
    assert bool((codes[:, 3] == 0).all()) and bool((codes[:, 7] == 0x80).all())
    assert bool((R.dequantize(codes, exps)[:, [3, 7]] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_image_is_representable_and_within_the_bound(dtype):
    """N(0, 0.02^2) columns (and scaled copies across the exponent range inside the clamps): W^ is exactly a number of the
    dtype, |W^ - W| <= 2^-4 |W| + 2^(e_n - 10), and the bound is not slack by more than a small factor."""
    g = torch.Generator().manual_seed(11)
    base = torch.randn(512, 96, generator=g) * 0.02
    shifts = [0, -1, 5] if dtype == F16 else [0, -90, -30, 40, 100]
    worst = 0.0
    for s in shifts:
        W = (base * 2.0 ** s).to(dtype)
        codes, exps = _both(W)
        lo, hi = R.EXP_RANGE[dtype]
        assert int(exps.min()) > lo and int(exps.max()) < hi, "the case must sit inside the clamps"
        img = R.dequantize(codes, exps)
        assert bool((img.to(dtype).double() == img).all()), "W^ is not a number of the compute dtype"
        err, bnd = (img - W.double()).abs(), R.error_bound(W, exps)
        assert bool((err <= bnd).all()), float((err / bnd).max())
        worst = max(worst, float((err / bnd).max()))
        assert not any(int(c) in R.NAN_CODES for c in codes.flatten()[::97])
        assert not bool(((codes & 0x7F) == 0x7F).any()), "a NaN code was emitted"
    print(f"{_ID(dtype)}: worst |W^ - W| / bound = {worst:.3f}")
    assert worst > 0.5, "the bound is not tight: the test would not see a format with more error"


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_every_column_reaches_the_top_binade(dtype):
    """The smallest exponent: the column maximum lies in (224, 448] before the rounding, so its code is in the top binade [224, 448]."""
    g = torch.Generator().manual_seed(5)
    W = (torch.randn(64, 40, generator=g) * 0.02).to(dtype)
    codes, exps = _both(W)
    top = R.TABLE[codes.to(torch.int64)].abs().amax(dim=0)
    assert bool((top >= 224).all()) and bool((top <= 448).all())


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_non_finite_is_refused(bad):
    W = torch.zeros(8, 8, dtype=BF16)
    W[2, 5] = bad
    with pytest.raises(ValueError):
        acc_quant.quantize_tensor(W)
    with pytest.raises(ValueError):
        R.quantize(W)


def test_other_dtypes_and_formats_are_refused():
    with pytest.raises(TypeError):
        acc_quant.quantize_tensor(torch.zeros(8, 8))
    with pytest.raises(ValueError):
        acc_quant.quantize_accumulators(torch.nn.Linear(8, 8), fmt="int8")


def test_ties_round_to_the_even_code():
    """Halfway between two codes: 17 = (16 + 18) / 2 under e = 0 (a 448 in the column pins it) goes to 16 (mantissa 000), 19
    to 20 (mantissa 010)."""
    W = torch.tensor([[448.0, 448.0, 448.0], [17.0, 19.0, -17.0]], dtype=BF16)
    codes, exps = _both(W)
    assert exps.tolist() == [0, 0, 0]
    assert R.TABLE[codes[1].to(torch.int64)].tolist() == [16.0, 20.0, -16.0]
