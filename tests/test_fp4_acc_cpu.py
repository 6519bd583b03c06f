"""The MXFP4 accumulator format (include/sow_amd.h: SOW_ACC_DENSE_FP4) on the CPU: the integer reference of fp4_acc_ref.py
against the definitions, and sow_amd's quantiser (plain torch ops, so it runs here) against the reference, bit for bit.  No
GPU, no library call."""
import math

import pytest
import torch

import fp4_acc_ref as R
from sow_amd import acc_quant

BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
_ID = {BF16: "bf16", F16: "f16"}.get
VAL = torch.tensor([v / 2 for v in R.VALUES_X2] + [-v / 2 for v in R.VALUES_X2], dtype=torch.float64)   # value of code 0 .. 15


def _ulp(v: float, dtype, step: int) -> float:
    t = torch.tensor([v], dtype=dtype)
    assert float(t) == v, "not a number of the dtype"
    return float((t.view(torch.int16) + step).view(dtype))


def _column(vals, dtype, rows=32):
    """A [rows, len(vals)] matrix whose row 0 is `vals` and whose other rows are zero: block maximum = |vals|."""
    W = torch.zeros(rows, len(vals), dtype=dtype)
    W[0] = torch.tensor(vals, dtype=torch.float64).to(dtype)
    assert W[0].double().tolist() == [float(v) for v in vals], "a test value is not a number of the dtype"
    return W


def _both(W):
    """The reference's and the package's quantisation of W, asserted bit-identical; returns (codes, scale bytes)."""
    codes, scales = R.quantize(W)
    q, s = acc_quant.quantize_tensor(W, "mxfp4")
    assert q.dtype == torch.uint8 and s.dtype == torch.uint8
    assert q.shape == (W.shape[0] // 2, W.shape[1]) and s.shape == (W.shape[0] // 32, W.shape[1])
    assert torch.equal(s, scales), f"scales differ: {s[s != scales][:8].tolist()} vs {scales[s != scales][:8].tolist()}"
    bad = q != codes
    assert not bad.any(), (f"{int(bad.sum())} code bytes differ; first at {tuple(int(v) for v in torch.nonzero(bad)[0])}: "
                           f"{int(q[bad][0]):#x} vs {int(codes[bad][0]):#x}")
    return codes, scales


def _exps(scales):
    return (scales.to(torch.int64) - 127).tolist()


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_exponent_at_6_times_a_power_of_two(dtype):
    """amax = 6 * 2^k sits exactly on the bound: e = k, code 7; one ulp above needs e = k + 1, one below keeps k."""
    lo, hi = R.EXP_RANGE[dtype]
    ks = range(-11, 12) if dtype == F16 else range(-110, 111)
    vals, want = [], []
    for k in ks:
        v = 6.0 * 2.0 ** k
        vals += [v, _ulp(v, dtype, +1), _ulp(v, dtype, -1)]
        want += [k, k + 1, k]
    W = _column(vals, dtype)
    codes, scales = _both(W)
    assert _exps(scales)[0] == want
    assert all(int(c) & 15 == 7 for c in codes[0, 0::3]), "6 * 2^k must be the largest code under e = k"
    assert torch.equal(R.dequantize(codes, scales, dtype)[0, 0::3], W[0, 0::3])
    for v, e in zip(vals, want):            # the vectorised exponent against the definition (integer search)
        _, M, E = R.fields(R.bits_of(torch.tensor([v], dtype=dtype)), dtype)
        assert R.block_exponent_of(int(M), int(E), dtype) == e


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_exponent_at_the_mantissa_boundary(dtype):
    """m = 0.75 exactly (amax = 3 * 2^j = 6 * 2^(j-1)) takes e = x - 3; powers of two (m = 0.5) too; m just above 0.75 takes
    x - 2."""
    vals, want = [], []
    for j in (-9, -1, 0, 1, 7):
        vals += [3.0 * 2.0 ** j, _ulp(3.0 * 2.0 ** j, dtype, +1), 2.0 ** j, _ulp(2.0 ** (j + 1), dtype, -1)]
        # 3 * 2^j: x = j + 2, m = .75 -> j - 1; above -> j; 2^j: x = j + 1 -> j - 2; just under 2^(j+1): x = j + 1, m > .75 -> j - 1
        want += [j - 1, j, j - 2, j - 1]
    codes, scales = _both(_column(vals, dtype))
    assert _exps(scales)[0] == want


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_clamps_and_zero_blocks(dtype):
    """Blocks past the exponent range keep the clamped exponent: large ones saturate at +-6 * 2^hi, small ones fall to the low
    codes or to zero.  The byte stays inside [2, 252]; an all-zero block (of either sign) gets e = 0."""
    lo, hi = R.EXP_RANGE[dtype]
    big = torch.finfo(dtype).max
    tiny = float(torch.tensor([1], dtype=torch.int16).view(dtype))       # the smallest subnormal
    W = _column([big, -big, tiny, -tiny, 6.0 * 2.0 ** hi, 2.0 ** (lo - 1), 0.0, -0.0], dtype, rows=64)
    W[32:, 0] = 1.0           # a second block of column 0 with an exponent of its own
    codes, scales = _both(W)
    assert _exps(scales)[0] == [hi, hi, lo, lo, hi, lo, 0, 0]
    assert _exps(scales)[1] == [-2, 0, 0, 0, 0, 0, 0, 0]
    assert int(scales.min()) >= 2 and int(scales.max()) <= 252
    q = R.unpack(codes)
    if dtype == F16:     # 65504 > 6 * 2^13: the clamp to 6 acts
        assert q[0].tolist()[:2] == [7, 15]
    assert int(q[0, 5]) == 1, "2^(lo - 1) is code 0.5 under e = lo"
    assert q[0].tolist()[6:] == [0, 8], "-0 keeps its sign"
    assert q[:, 7].tolist() == [8] + [0] * 63
    img = R.dequantize(codes, scales, dtype)
    assert bool(torch.isfinite(img.double()).all())
    assert int(R.dequantize_bits(codes, scales, dtype)[0, 7]) == -0x8000


def test_ties_round_to_the_even_code():
    """Scaled 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4 (a 6 in the block pins e = 0), both signs; one
    ulp either side of a tie goes to the nearer code."""
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    lower = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0]
    upper = [0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    for dtype in DTYPES:
        W = torch.zeros(32, 7, dtype=dtype)
        W[0] = 6.0
        W[1] = torch.tensor(ties, dtype=dtype)
        W[2] = -W[1]
        W[3] = torch.tensor([_ulp(t, dtype, -1) for t in ties], dtype=dtype)
        W[4] = torch.tensor([_ulp(t, dtype, +1) for t in ties], dtype=dtype)
        codes, scales = _both(W)
        assert _exps(scales) == [[0] * 7]
        v = VAL[R.unpack(codes)]
        assert v[1].tolist() == want and v[2].tolist() == [-x for x in want]
        assert v[3].tolist() == lower and v[4].tolist() == upper
        assert (R.unpack(codes)[2] >> 3).tolist() == [1] * 7, "the sign is kept, on a zero code too"


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_saturation_and_negative_zero(dtype):
    hi = R.EXP_RANGE[dtype][1]
    big = torch.finfo(dtype).max
    W = torch.zeros(32, 4, dtype=dtype)
    W[0] = torch.tensor([big, -big, big, big], dtype=dtype)
    W[1] = torch.tensor([big, big, -big, -0.0], dtype=dtype)
    codes, scales = _both(W)
    q = R.unpack(codes)
    assert _exps(scales) == [[hi] * 4]
    assert q[0].tolist() == [7, 15, 7, 7] and q[1].tolist() == [7, 7, 15, 8]
    assert bool((q[2:] == 0).all())


def test_nibble_packing():
    """byte[k / 2, n] = code(k, n) | code(k + 1, n) << 4: every code value in the low and in the high nibble."""
    W = torch.zeros(32, 2, dtype=BF16)
    vals = [v / 2 for v in R.VALUES_X2]
    W[0:16, 0] = torch.tensor(vals + [-v for v in vals], dtype=BF16)          # codes 0 .. 15 in rows 0 .. 15
    W[16:32, 1] = W[0:16, 0]
    W[0, 1] = 6.0
    codes, scales = _both(W)
    assert _exps(scales) == [[0, 0]]
    assert codes[:8, 0].tolist() == [(2 * i) | ((2 * i + 1) << 4) for i in range(8)]
    assert codes[8:, 1].tolist() == [(2 * i) | ((2 * i + 1) << 4) for i in range(8)]
    assert codes[0, 1] == 7 and R.unpack(codes)[:16, 0].tolist() == list(range(16))
    assert torch.equal(R.dequantize(codes, scales, BF16), W) and torch.equal(
        R.dequantize_bits(codes, scales, BF16), W.view(torch.int16)), "-0 must come back as -0"


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_image_is_representable_normal_and_within_the_bound(dtype):
    """N(0, 0.02^2) columns (and scaled copies across the exponent range inside the clamps): every W^ is a normal number of
    the dtype or a zero (the integer reference builds the bit pattern and asserts the exponent field), it equals value(q) * 2^e
    computed in float64, and |W^ - W| <= 2^-2 |W| + 2^(e - 2).  Recorded on this seed (bf16, shift 0): worst error / bound 0.80,
    relative Frobenius error 0.118 per block against 0.130 with one exponent per column."""
    g = torch.Generator().manual_seed(11)
    base = torch.randn(512, 96, generator=g) * 0.02
    shifts = [0, -2, 8] if dtype == F16 else [0, -90, -30, 40, 100]
    lo, hi = R.EXP_RANGE[dtype]
    worst = 0.0
    for s in shifts:
        W = (base * 2.0 ** s).to(dtype)
        codes, scales = _both(W)
        e = scales.to(torch.int64) - 127
        assert int(e.min()) > lo and int(e.max()) < hi, "the case must sit inside the clamps"
        img = R.dequantize(codes, scales, dtype)
        ef = torch.exp2(e.to(torch.float64)).repeat_interleave(32, dim=0)
        assert torch.equal(img.double(), VAL[R.unpack(codes)] * ef), "the bit pattern is not value(q) * 2^e"
        tiny = torch.finfo(dtype).tiny
        assert bool(((img.double().abs() >= tiny) | (img == 0)).all()), "a subnormal W^"
        err, bnd = (img.double() - W.double()).abs(), W.double().abs() * 0.25 + ef * 0.25
        assert bool((err <= bnd).all()), float((err / bnd).max())
        worst = max(worst, float((err / bnd).max()))
        if s == 0:
            rel = float((img.double() - W.double()).norm() / W.double().norm())
            # one exponent per column, for comparison: the same codes rule under the column's exponent
            Wc = W.double()
            amax = Wc.abs().amax(dim=0)
            m, x = torch.frexp(amax)
            ec = (x - 3 + (m > 0.75)).to(torch.float64)
            a = (Wc * torch.exp2(-ec)).clamp(-6, 6)
            idx = (a.abs().unsqueeze(-1) - VAL[:8]).abs().argmin(dim=-1)
            relc = float((torch.sign(a) * VAL[idx] * torch.exp2(ec) - Wc).norm() / Wc.norm())
            print(f"{_ID(dtype)}: relative Frobenius error {rel:.3f} per block, {relc:.3f} per column")
    print(f"{_ID(dtype)}: worst |W^ - W| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_every_block_reaches_the_top_binade(dtype):
    """The smallest exponent: the block maximum lies in (3, 6] before the rounding, so its code is 4 or 6 (magnitude codes 6, 7)."""
    g = torch.Generator().manual_seed(5)
    W = (torch.randn(96, 40, generator=g) * 0.02).to(dtype)
    codes, scales = _both(W)
    top = (R.unpack(codes) & 7).view(3, 32, 40).amax(dim=1)
    assert bool((top >= 5).all())      # (3, 3.5) rounds to 3 (code 5); everything above to 4 or 6


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_non_finite_is_refused(bad):
    W = torch.zeros(32, 8, dtype=BF16)
    W[2, 5] = bad
    with pytest.raises(ValueError):
        acc_quant.quantize_tensor(W, "mxfp4")
    with pytest.raises(ValueError):
        R.quantize(W)


def test_other_dtypes_shapes_and_formats_are_refused():
    with pytest.raises(TypeError):
        acc_quant.quantize_tensor(torch.zeros(32, 8), "mxfp4")
    with pytest.raises(ValueError):
        acc_quant.quantize_tensor(torch.zeros(24, 8, dtype=BF16), "mxfp4")
    with pytest.raises(ValueError):
        acc_quant.quantize_accumulators(torch.nn.Linear(8, 8), fmt="int4")
    assert "mxfp4" in acc_quant.FORMATS and "fp8_e4m3" in acc_quant.FORMATS
    assert acc_quant.quantize_accumulators(torch.nn.Linear(8, 8), fmt="mxfp4") == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_torch_quantiser_equals_the_integer_reference(dtype):
    """Random matrices with wide dynamic range, subnormals, exact ties, zeros of both signs and several blocks per column."""
    g = torch.Generator().manual_seed(23)
    span = 6 if dtype == F16 else 60
    W = (torch.randn(160, 136, generator=g) * torch.exp2(torch.randint(-span, span, (5, 136), generator=g).float())
         .repeat_interleave(32, dim=0)).to(dtype)
    W[torch.rand(160, 136, generator=g) < 0.05] = 0.0
    W[torch.rand(160, 136, generator=g) < 0.02] = -0.0
    W[3, :] = torch.finfo(dtype).tiny / 4
    W = torch.where(torch.isfinite(W), W, torch.zeros_like(W))
    _both(W)
    # exact ties in every block: multiples of 0.25 of the block scale
    T = (torch.randint(-24, 25, (64, 40), generator=g).double() * 0.25)
    T[0::32] = 6.0
    _both(T.to(dtype))
