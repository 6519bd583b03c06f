"""-m gpu: MXFP4 dense accumulators -- include/sow_amd.h SOW_ACC_DENSE_FP4, sow_acc_dequantize_fp4,
sow_amd.quantize_accumulators(fmt="mxfp4").

The contract: a quantised layer computes what the dense-accumulator layer computes on the dequantised matrix
W^ = e2m1(codes) * 2^(block scale), which is exactly a number of the compute dtype.  So nothing here has a tolerance of its own:
* the quantiser and the image pass are compared bit for bit with the integer reference of fp4_acc_ref.py -- the image test
  is also what pins the hardware conversion's semantics (which nibble is the first element, how the scale operand is read,
  that -0 stays -0);
* the skinny forward is held bit for bit to W^ on one-hot inputs, element by element to test_gpu_skinny._reference /
  numerics.bound with W := W^ through test_gpu_skinny's buffer protocol (NaN neighbours, sentinel guards, poisoned / zeroed /
  poisoned memory, three runs bit-identical), and bit for bit on value_plan's exact operands;
* the module paths are bit-identical to the C-ABI call (no-grad, T <= 32) or to an unquantised twin whose accumulator IS W^
  (larger T, training, FactorBucket sinks, sibling groups), and so are their HIP-graph replays.
"""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn

import fp4_acc_ref as R
import graph_replay as GR
import skinny_sweep as SW
import test_gpu_elementwise as E
import test_gpu_fp8_acc as F8
import test_gpu_skinny as S
import value_plan as VP
from numerics import rne, to64
from sow_amd import _lib, dequantize_accumulators, acc_quant, ops, quantize_accumulators

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
DT = S.DT
ERR_UNSUPPORTED = -6
KIND = getattr(_lib, "ACC_DENSE_FP4", None)
GUARD = 64
SENTINEL = -7.25
SCALE_BYTES = {"bf16": (2, 119, 127, 135, 252), "f16": (114, 127, 140)}


def _quant(W):
    """(packed codes uint8, scale bytes uint8, W^ in W's dtype) on the CPU, through the integer reference."""
    codes, scales = R.quantize(W)
    return codes, scales, R.dequantize(codes, scales, W.dtype)


def _quantised(d):
    """The operands of a layer with W replaced by its quantisation: W = W^ (what the reference sees), q / e = what the kernel
    reads."""
    codes, scales, what = _quant(d["W"])
    return dict(d, W=what, q=codes, e=scales)


def _guarded_bytes(t, fill):
    """A uint8 operand between guards of `fill`: 0x77 around the codes (6, 6) and 254 around the scales (2^127) -- a read past
    either is a huge value in y."""
    return F8._guarded_bytes(t, fill)


def _run(dtype, layers, x_shared=False, runs=(0xFF, 0x00, 0xFF), what="fp4 skinny"):
    """test_gpu_skinny._run for layers with an MXFP4 accumulator (dicts from _quantised; "q" absent: no accumulator)."""
    lib = _lib.load()
    ar = E.Arena(dtype)
    arr = (_lib.LayerArgs * len(layers))()
    ys, keep = [], []
    x0 = None
    for i, d in enumerate(layers):
        x = x0 if (x_shared and x0 is not None) else ar.input(d["x"])
        x0 = x0 if x0 is not None else x
        A, B, bias = (ar.input(d.get(k)) for k in ("A", "B", "bias"))
        fp4 = d.get("q") is not None
        q = _guarded_bytes(d["q"], 0x77) if fp4 else None
        e = _guarded_bytes(d["e"], 254) if fp4 else None
        T, d_in = d["x"].shape
        r, d_out = d["B"].shape
        kind = KIND if fp4 else _lib.ACC_NONE
        y = ar.output((T, d_out))
        nws = (lib.sow_forward_skinny_fp4_workspace_bytes(T, d_in, d_out, r, E._dt(dtype)) if fp4
               else lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, kind, E._dt(dtype)))
        assert nws > 0, (T, d_in, d_out, r, kind)
        ws = ar.workspace(nws)
        a = arr[i]
        a.x, a.A, a.B, a.acc_down, a.acc_up, a.bias, a.y = (E._ptr(t) for t in (x, A, B, q, e, bias, y))
        a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, kind, d["s"]
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        ys.append(y)
        keep.append((x, A, B, bias, q, e, ws))
    outs = []
    for byte in runs:
        ar.fill(byte)
        _lib.check(lib.sow_forward_skinny(arr, len(layers), E._dt(dtype), E._stream()), "sow_forward_skinny")
        ar.check_guards(f"{what} run {len(outs)}")
        outs.append([y.clone() for y in ys])
    for k in range(1, len(outs)):
        for i, (a, b) in enumerate(zip(outs[0], outs[k])):
            assert torch.equal(E._bits(a), E._bits(b)), f"{what}: y of layer {i} differs between run 0 and run {k}"
    return [y.cpu() for y in outs[0]]


def _check(name, dtype, d, y):
    """test_gpu_skinny's comparator on W^ (d["W"]): no other tolerance."""
    return S._check("fp4_" + name, dtype, {k: v for k, v in d.items() if k not in ("q", "e")}, y)


# ---- 1. the image pass: every code, position, scale ------------------------------------------------------------------------------
def _dequant(codes, scales, dtype, ldd=None):
    """sow_acc_dequantize_fp4 into a [d_in, ldd] buffer full of sentinels, between guards; (image, whole buffer) on the CPU."""
    d_in, d_out = 2 * codes.shape[0], codes.shape[1]
    ldd = ldd or d_out
    buf = torch.full((d_in * ldd + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    out = buf[GUARD:GUARD + d_in * ldd].view(d_in, ldd)
    q, e = _guarded_bytes(codes, 0x77), _guarded_bytes(scales, 254)
    rc = _lib.load().sow_acc_dequantize_fp4(q.data_ptr(), e.data_ptr(), d_in, d_out, out.data_ptr(), ldd, E._dt(dtype), E._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + d_in * ldd:] == SENTINEL).all()), "guards"
    return out[:, :d_out].cpu(), out.cpu()


def _same_image(got, codes, scales, dtype, what=""):
    """Bit for bit against the integer reference.  On a mismatch the message says which reading of the instruction the image
    does follow, if any: nibbles swapped, or zeros without their sign."""
    want = R.dequantize_bits(codes, scales, dtype)
    bits = got.view(torch.int16)
    if torch.equal(bits, want):
        return
    swapped = R.dequantize_bits(((codes << 4) | (codes >> 4)).to(torch.uint8), scales, dtype)
    unsigned_zero = torch.where(want == -0x8000, torch.zeros_like(want), want)
    bad = bits != want
    i = tuple(int(v) for v in torch.nonzero(bad)[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the integer reference; first at {i}: "
                         f"{int(bits[i]) & 0xFFFF:#06x} vs {int(want[i]) & 0xFFFF:#06x} (code byte {int(codes[i[0] // 2, i[1]]):#04x}, "
                         f"scale byte {int(scales[i[0] // 32, i[1]])}); equals the nibble-swapped image: {torch.equal(bits, swapped)}; "
                         f"equals the image with -0 as +0: {torch.equal(bits, unsigned_zero)}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_dequantise_every_byte_in_every_position_under_every_scale(dt):
    """512 rows x 128 columns: column n sees all 256 byte values (byte (kp + 37 n) mod 256 in code row kp) -- all 16 codes in
    both rows of a pair, in every one of the 8 byte positions of every one of the 16 lanes of a group -- and over the shifts
    every (block, column) meets every scale byte of the set, the ends of the clamped range among them.  ldd > d_out on the way."""
    dtype = DT[dt]
    kp, n = torch.arange(256).view(-1, 1), torch.arange(128).view(1, -1)
    codes = ((kp + 37 * n) % 256).to(torch.uint8)
    sb = torch.tensor(SCALE_BYTES[dt], dtype=torch.uint8)
    kb = torch.arange(16).view(-1, 1)
    for shift in range(len(sb)):
        scales = sb[(kb + n + shift) % len(sb)].contiguous()
        ldd = 128 if shift else 128 + 24
        got, whole = _dequant(codes, scales, dtype, ldd=ldd)
        _same_image(got, codes, scales, dtype, what=f"{dt} shift {shift}")
        assert bool((whole[:, 128:] == SENTINEL).all()), "the gap between rows was written"
        assert int((got.view(torch.int16) == -0x8000).sum()) == 2 * 16 * 128, "every column holds the -0 code 16 times per nibble"
    # the wrapper, and a shape that is no multiple of the 256-thread block with an odd row pitch
    g = torch.Generator().manual_seed(7)
    codes = torch.randint(0, 256, (80, 136), generator=g).to(torch.uint8)
    scales = sb[torch.randint(0, len(sb), (5, 136), generator=g)].contiguous()
    got, whole = _dequant(codes, scales, dtype, ldd=136 + 8)
    _same_image(got, codes, scales, dtype, what="160 x 136")
    assert bool((whole[:, 136:] == SENTINEL).all())
    img = ops.acc_dequantize(codes.to(DEV), scales.to(DEV), dtype)
    _same_image(img.cpu(), codes, scales, dtype, what="ops.acc_dequantize")


def test_dequantise_refusals():
    lib = _lib.load()
    q = torch.zeros(32, 64, dtype=torch.uint8, device=DEV)
    e = torch.full((2, 64), 127, dtype=torch.uint8, device=DEV)
    out = torch.full((64, 64), SENTINEL, dtype=BF16, device=DEV)
    call = lambda d_in, d_out, ldd, dt, qp=q.data_ptr(): lib.sow_acc_dequantize_fp4(qp, e.data_ptr(), d_in, d_out, out.data_ptr(), ldd, dt, E._stream())  # noqa: E731
    assert call(64, 60, 64, _lib.BF16) == ERR_UNSUPPORTED and call(64, 64, 60, _lib.BF16) == _lib.ERR_SHAPE
    assert call(64, 64, 64, _lib.F32) == _lib.ERR_DTYPE and call(56, 64, 64, _lib.BF16) == ERR_UNSUPPORTED
    assert call(64, 64, 64, _lib.BF16, q.data_ptr() + 4) == -4
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- 2. the quantiser on a device tensor ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_quantiser_matches_the_reference_bit_for_bit(dt):
    dtype = DT[dt]
    g = torch.Generator().manual_seed(160 + (1 if dt == "f16" else 0))
    W = (torch.randn(160, 136, generator=g) * 0.02).to(dtype)
    tiny = float(torch.tensor([1], dtype=torch.int16).view(dtype))
    W[:, 3] = 0                                                          # zero blocks: e = 0
    W[32:64, 4] = -0.0
    W[:, 9] = (torch.randint(-40, 41, (160,), generator=g) * tiny).to(dtype)        # subnormal magnitude: the lower clamp
    W[:, 17] = (torch.randn(160, generator=g) * 8000).to(dtype)
    W[0, 17] = torch.finfo(dtype).max if dt == "f16" else 2.0 ** 127                 # the upper clamp
    W[:, 25] = (torch.randint(-24, 25, (160,), generator=g).double() * 0.25 * 2.0 ** -5).to(dtype)   # exact ties
    W[::32, 25] = 6.0 * 2.0 ** -5
    codes, scales = R.quantize(W)
    q, e = acc_quant.quantize_tensor(W.to(DEV), "mxfp4")
    assert q.is_cuda and q.dtype == torch.uint8 and e.dtype == torch.uint8 and q.is_contiguous() and e.is_contiguous()
    assert q.shape == (80, 136) and e.shape == (5, 136)
    assert torch.equal(e.cpu(), scales), "scale bytes"
    bad = q.cpu() != codes
    assert not bad.any(), f"{int(bad.sum())} code bytes differ from the reference; first at {tuple(int(v) for v in torch.nonzero(bad)[0])}"
    lo, hi = R.EXP_RANGE[dtype]
    assert scales[:, 3].tolist() == [127] * 5 and int(scales[0, 9]) == lo + 127 and int(scales[0, 17]) == hi + 127
    with pytest.raises(ValueError):
        bad_w = W.to(DEV)
        bad_w[3, 4] = float("inf")
        acc_quant.quantize_tensor(bad_w, "mxfp4")


# ---- 3. one-hot rows: y[t, :] = W^[k_t, :] -------------------------------------------------------------------------------------------
def _staircase(dtype, d_in, d_out, seed):
    """W whose neighbouring blocks of a column, and neighbouring columns of a block, lie `step` binades apart (20 for bf16; 6 for
    f16, whose whole range is 26): a wrong block, column or slab index in the scale load shows as a wrong power of two."""
    step = 20 if dtype == BF16 else 6
    g = torch.Generator().manual_seed(seed)
    kb, n = torch.arange(d_in // 32).view(-1, 1), torch.arange(d_out).view(1, -1)
    e = (step * ((kb + n) % 5) - 2 * step).repeat_interleave(32, dim=0)
    W = ((torch.rand(d_in, d_out, generator=g) * 5 + 1) * (torch.randint(0, 2, (d_in, d_out), generator=g) * 2 - 1)
         * torch.exp2(e.double())).to(dtype)
    return W, step


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("shape", [(160, 136), (1376, 512)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_hot_rows_return_rows_of_the_image(dt, shape):
    """B = 0, bias = 0, x[t, k_t] = 1: y[t, n] = W^[k_t, n], bit for bit (a -0 of W^ arrives as +0: the sum starts from +0).
    Row t of a call sits at offset t of its block -- offset 8 kg + 2 i + nibble: every (lane group, row pair, nibble) -- and the
    blocks are chosen so that rows d_in - 1, 0, and both sides of the slab boundary at k = 128 (127: last row of a block,
    128: first) are read; two calls with other blocks reach the other waves."""
    dtype = DT[dt]
    d_in, d_out = shape
    W, step = _staircase(dtype, d_in, d_out, seed=d_in)
    codes, scales, what = _quant(W)
    e = scales.to(torch.int64) - 127
    assert int((e[1:] - e[:-1]).abs().min()) >= step - 1 and int((e[:, 1:] - e[:, :-1]).abs().min()) >= step - 1
    nb = d_in // 32
    assert _lib.load().sow_forward_skinny_fp4_workspace_bytes(32, d_in, d_out, 8, E._dt(dtype)) > 0
    for call in range(2):
        blocks = [(7 * t + 3 * call) % nb for t in range(32)]
        blocks[31], blocks[0] = 3, 4                      # k = 127 and k = 128
        if call:
            blocks[0], blocks[31] = 0, nb - 1             # k = 0 and k = d_in - 1
        ks = [32 * b + t for t, b in enumerate(blocks)]
        x = torch.zeros(32, d_in, dtype=dtype)
        x[torch.arange(32), ks] = 1.0
        d = dict(x=x, A=(torch.randn(d_in, 8, generator=torch.Generator().manual_seed(1)) * 0.05).to(dtype),
                 B=torch.zeros(8, d_out, dtype=dtype), bias=torch.zeros(d_out, dtype=dtype), W=what, q=codes, e=scales, s=0.5)
        (y,) = _run(dtype, [d], runs=(0xFF, 0x00), what=f"one-hot call {call}")
        want = what[ks]
        want = torch.where(want == 0, torch.zeros_like(want), want)
        bad = y.view(torch.int16) != want.view(torch.int16)
        if bad.any():
            t, n = (int(v) for v in torch.nonzero(bad)[0])
            raise AssertionError(f"{int(bad.sum())} elements differ; first y[{t}, {n}] = {float(y[t, n])!r}, W^[{ks[t]}, {n}] = "
                                 f"{float(want[t, n])!r}; rows with a difference: {sorted(set(torch.nonzero(bad)[:, 0].tolist()))}")


# ---- 4. the skinny forward through the buffer protocol -----------------------------------------------------------------------------
def _off_ties(dtype, d):
    """The operands `d` (from _quantised: W = W^) with the projections that matter moved off rounding ties, decided on the CPU
    from the operands alone before anything runs.  test_gpu_skinny._reference rounds the EXACT h = s x A; the kernel rounds an
    fp32 sum, and where the exact value lies closer to a rounding midpoint than that sum's noise (test_gpu_fp8_acc._tie_margin:
    fewer than 64 fp32 roundings) the two may round apart.  Row t of y then moves by ulp(h[t, j]) B[j, n], which is no error of
    the kernel and which the comparator has no term for: with test_gpu_skinny's seed-0 operands of f16 1376 -> 512, T = 32,
    r = 50, h[25, 1] = -0.2216186 lies 0.036 noise units from a midpoint, and y[25, 250] (|y| = 1.1e-3, bound 8.1e-6) came back
    1.02e-5 = ulp(h) B[1, 250] away.  An element (t, j) MATTERS when such a move would exceed an eighth of the comparator's own
    bound somewhere in its row; while one that matters is within the noise of a tie, one more element of column j of A is moved
    by one ulp (each element at most once), which shifts the column's h by about s x[t, k] ulp(A).  Returns (d, elements moved)."""
    return SW.off_ties(dtype, d)   # (the step itself, shared with the seeded sweep: a plain W or none pass through it too)


@pytest.mark.parametrize("T", [1, 4, 17, 32])
@pytest.mark.parametrize("shape", [(32, 8), (160, 136), (512, 512), (1376, 512)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_skinny_elementwise_against_fp64(dt, shape, T):
    dtype = DT[dt]
    d_in, d_out = shape
    for r in (8, 50):
        for bias in (True, False):
            d, moved = _off_ties(dtype, _quantised(dict(S._gauss(dtype, T, d_in, d_out, r, bias, "dense"), s=0.5)))
            name = f"{dt}-{T}-{d_in}-{d_out}-{r}-{bias}"
            print(f"{name}: {moved} of {d['A'].numel()} elements of A moved by one ulp")
            assert moved <= d["A"].numel() // 100
            (y,) = _run(dtype, [d], runs=(0xFF, 0x00, 0xFF) if r == 50 and bias else (0xFF,), what=name)
            _check(name, dtype, d, y)


def _clear_of_ties(dtype, T, d_in, d_out, r, bias, s, seed):
    """test_gpu_fp8_acc's tie-clearing operands, with the condition that at most 1 % of A's elements were moved (by one ulp)."""
    d = F8._gauss_clear_of_ties(dtype, T, d_in, d_out, r, bias, s, seed)
    A0 = S._gauss(dtype, T, d_in, d_out, r, bias, "dense", seed=seed)["A"]
    moved = int((d["A"].view(torch.int16) != A0.view(torch.int16)).sum())
    print(f"{d_in}x{d_out}: {moved} of {A0.numel()} elements of A moved by one ulp")
    assert moved <= A0.numel() // 100
    return d


def test_skinny_long_k():
    """8224 -> 128 at T = 32: one 128-column range, so the >= 512-workgroup rule plans 65 slabs of 128 rows -- 64 full ones and a
    32-row tail (one block: three of the four waves idle) -- and phase B adds 65 partials, 49 of them in its second loop.
    (Slabs reach 1024 rows only where d_in * d_out / 128 exceeds 512 * 896: past 58 M elements.)"""
    lib = _lib.load()
    assert lib.sow_forward_skinny_fp4_workspace_bytes(32, 8224, 128, 8, _lib.BF16) == 256 + 65 * 32 * (128 + 64) * 4
    d = _quantised(_clear_of_ties(BF16, 32, 8224, 128, 8, True, 0.5, seed=40))
    (y,) = _run(BF16, [d], what="long k")
    _check("long_k", BF16, d, y)


def test_skinny_ring_refill():
    """4128 -> 8200 at T = 32: 65 column ranges, seven slabs of 640 (six full, one of 288 rows = two rounds and a block): a
    fifth k-step per wave refills the request-ahead ring, and the last slab ends in a partial round."""
    lib = _lib.load()
    assert lib.sow_forward_skinny_fp4_workspace_bytes(32, 4128, 8200, 8, _lib.BF16) == 256 + 7 * 32 * (8200 + 64) * 4
    d = _clear_of_ties(BF16, 32, 4128, 8200, 8, False, 1.0, seed=41)
    q, e = acc_quant.quantize_tensor(d["W"].to(DEV), "mxfp4")          # (tied to the reference by the quantiser tests)
    codes, scales = q.cpu(), e.cpu()
    d = dict(d, W=R.dequantize(codes, scales, BF16), q=codes, e=scales)
    (y,) = _run(BF16, [d], runs=(0xFF, 0x00), what="ring refill")
    _check("ring_refill", BF16, d, y)


# ---- 5. exact operands ------------------------------------------------------------------------------------------------------------
EXACT = [("bf16", 17, 288, 520, 50, True, 0.5, "dense"), ("f16", 32, 544, 264, 8, True, 0.25, "dense"),
         ("f16", 16, 160, 136, 2, True, 0.5, "dense")]


def _exact_fp4(c):
    """test_gpu_skinny's exact operands with W replaced by W^, and the proof again for W^ (float64, CPU): every sum the kernel
    forms is made of multiples of one unit with sum |terms| below 2^24 units."""
    dtype = DT[c[0]]
    d0, _ = S._exact_operands(c)
    d = _quantised(d0)
    q = {k: to64(v) for k, v in d.items() if isinstance(v, torch.Tensor) and k not in ("q", "e")}
    x, A, B, W = q["x"], q["A"], q["B"], q["W"]
    h = d["s"] * (x @ A)
    assert bool((rne(h, dtype) == h).all())
    units = [VP.lsb(h) * VP.lsb(B), VP.lsb(x) * VP.lsb(W)]
    total = h.abs() @ B.abs() + x.abs() @ W.abs()
    y = h @ B + x @ W
    if "bias" in q:
        units.append(VP.lsb(q["bias"]))
        total, y = total + q["bias"].abs(), y + q["bias"]
    assert float(total.max()) / min(units) < VP.EXACT_UNITS, "y: a partial sum may be inexact"
    assert float((y != 0).double().mean()) >= 0.5, "exactness bought with emptiness"
    assert float((W != 0).double().mean()) > 0.01, "W^ is empty"
    return d, y


@pytest.mark.parametrize("c", EXACT, ids=S._id)
def test_skinny_exact_operands_bit_for_bit(c):
    dtype = DT[c[0]]
    d, y64 = _exact_fp4(c)
    (y,) = _run(dtype, [d], what="exact " + S._id(c))
    bad = to64(y) != rne(y64, dtype)
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} elements differ from the float64 result rounded once"


# ---- 6. rows are independent -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,k,v", [("bf16", 0, "nan"), ("bf16", 159, "inf"), ("f16", 130, "nan"), ("f16", 31, "-inf")])
def test_skinny_rows_are_independent(dt, k, v):
    dtype = DT[dt]
    d = _quantised(dict(S._gauss(dtype, 3, 160, 136, 50, True, "dense", seed=3), s=0.5))
    (clean,) = _run(dtype, [d], runs=(0xFF,), what="rows clean")
    p = dict(d, x=d["x"].clone())
    p["x"][1, k] = float(v)
    (poisoned,) = _run(dtype, [p], runs=(0xFF,), what="rows poisoned")
    assert not bool(torch.isfinite(poisoned[1]).any()), "row 1 must be non-finite in every column"
    for t in (0, 2):
        assert torch.equal(E._bits(poisoned[t]), E._bits(clean[t])), f"row {t} changed"


# ---- 7. groups and refusals ---------------------------------------------------------------------------------------------------------
def test_skinny_groups_equal_single_calls():
    # three siblings on ONE x buffer: 512 -> {512, 256, 256}
    g = torch.Generator().manual_seed(9)
    x = torch.randn(5, 512, generator=g).to(BF16)
    sibs = []
    for i, d_out in enumerate((512, 256, 256)):
        d = dict(S._gauss(BF16, 5, 512, d_out, 50, i == 1, "dense", seed=20 + i), s=0.5)
        d["x"] = x
        sibs.append(_quantised(d))
    grouped = _run(BF16, sibs, x_shared=True, what="qkv group")
    for i, (d, yg) in enumerate(zip(sibs, grouped)):
        (ys,) = _run(BF16, [d], runs=(0xFF,), what=f"qkv single {i}")
        assert torch.equal(E._bits(yg), E._bits(ys)), f"sibling {i}"
        _check(f"qkv_{i}", BF16, d, yg)
    # different inputs and token counts, one layer without an accumulator sharing the call
    trio = [_quantised(dict(S._gauss(F16, 4, 160, 136, 8, True, "dense", seed=30), s=0.25)),
            dict(S._gauss(F16, 32, 520, 264, 64, False, "none", seed=31), s=1.0),
            _quantised(dict(S._gauss(F16, 17, 1376, 72, 2, False, "dense", seed=32), s=1.0))]
    grouped = _run(F16, trio, what="mixed group")
    for i, (d, yg) in enumerate(zip(trio, grouped)):
        (ys,) = _run(F16, [d], runs=(0xFF,), what=f"mixed single {i}")
        assert torch.equal(E._bits(yg), E._bits(ys)), f"layer {i}"
        if "q" in d:
            _check(f"mixed_{i}", F16, d, yg)
        else:
            (plain,) = S._run(F16, [d], runs=(0xFF,), what="the unquantised call")
            assert torch.equal(E._bits(yg), E._bits(plain)), "a layer without accumulator computes what it computes in a plain call"


def _refusal_args(T=4, d_in=160, d_out=136, r=8, kind=KIND):
    z = lambda *s: torch.zeros(*s, dtype=BF16, device=DEV)   # noqa: E731
    t = dict(x=z(T, d_in), A=z(d_in, r), B=z(r, d_out), q=torch.zeros(d_in, d_out, dtype=torch.uint8, device=DEV),
             e=torch.full((d_in // 32 + 1, d_out), 127, dtype=torch.uint8, device=DEV), bias=z(d_out), dy=z(T, d_out))
    outs = dict(y=torch.empty(T, d_out, dtype=BF16, device=DEV), h=torch.empty(T, 64, dtype=BF16, device=DEV),
                dx=torch.empty(T, d_in, dtype=BF16, device=DEV), dA=torch.empty(d_in, r, dtype=BF16, device=DEV),
                dB=torch.empty(r, d_out, dtype=BF16, device=DEV), ws=torch.empty(1 << 20, dtype=torch.uint8, device=DEV))
    for o in outs.values():
        o.view(torch.uint8).fill_(0xFF)
    arr = (_lib.LayerArgs * 1)()
    a = arr[0]
    a.x, a.A, a.B, a.acc_down, a.acc_up, a.bias, a.y, a.h_save = (v.data_ptr() for v in (
        t["x"], t["A"], t["B"], t["q"], t["e"], t["bias"], outs["y"], outs["h"]))
    a.dy, a.dx, a.dA, a.dB = t["dy"].data_ptr(), outs["dx"].data_ptr(), outs["dA"].data_ptr(), outs["dB"].data_ptr()
    a.T, a.d_in, a.d_out, a.r_live, a.r_acc, a.acc_kind, a.scale = T, d_in, d_out, r, 0, kind, 1.0
    a.workspace, a.workspace_bytes = outs["ws"].data_ptr(), outs["ws"].numel()
    return t, outs, arr


@pytest.mark.parametrize("entry", ["sow_forward", "sow_forward_group", "sow_backward_ex", "sow_backward_group", "sow_forward_shared",
                                   "sow_backward_shared"])
def test_other_entry_points_refuse_the_kind(entry):
    lib = _lib.load()
    assert KIND == 4
    t, o, arr = _refusal_args()
    p = lambda v: v.data_ptr()   # noqa: E731
    st = E._stream()
    both = _lib.BWD_DATA | _lib.BWD_WEIGHTS
    if entry == "sow_forward":
        rc = lib.sow_forward(p(t["x"]), p(t["A"]), p(t["B"]), p(t["q"]), p(t["e"]), p(t["bias"]), p(o["y"]), p(o["h"]), 4, 160, 136, 8,
                             0, KIND, 1.0, _lib.BF16, p(o["ws"]), o["ws"].numel(), st)
    elif entry == "sow_backward_ex":
        rc = lib.sow_backward_ex(p(t["dy"]), p(t["x"]), p(o["h"]), p(t["A"]), p(t["B"]), p(t["q"]), p(t["e"]), p(o["dx"]), p(o["dA"]),
                                 p(o["dB"]), None, 4, 160, 136, 8, 0, KIND, 1.0, 0.0, _lib.BF16, p(o["ws"]), o["ws"].numel(), both, st)
    elif entry in ("sow_forward_group", "sow_forward_shared"):
        rc = getattr(lib, entry)(arr, 1, _lib.BF16, st)
    else:
        rc = getattr(lib, entry)(arr, 1, _lib.BF16, both, st)
    assert rc == ERR_UNSUPPORTED, rc
    F8._untouched(o, entry)
    assert lib.sow_workspace_bytes(4, 160, 136, 8, 0, KIND, _lib.BF16) == 0
    assert lib.sow_forward_workspace_bytes(4, 160, 136, 8, 0, KIND, _lib.BF16) == 0


SKINNY_REFUSALS = [("T=33", dict(T=33)), ("r=66", dict(r=66)), ("d_in=520", dict(d_in=520)), ("d_out=524", dict(d_out=524))]


@pytest.mark.parametrize("name,kw", SKINNY_REFUSALS, ids=[r[0] for r in SKINNY_REFUSALS])
def test_skinny_refusals_touch_nothing(name, kw):
    lib = _lib.load()
    t, o, arr = _refusal_args(**kw)
    a = arr[0]
    assert lib.sow_forward_skinny_fp4_workspace_bytes(a.T, a.d_in, a.d_out, a.r_live, _lib.BF16) == 0
    assert lib.sow_forward_skinny(arr, 1, _lib.BF16, E._stream()) == ERR_UNSUPPORTED
    F8._untouched(o, name)


def test_skinny_refuses_mixed_kinds_and_missing_scales():
    lib = _lib.load()
    t, o, arr1 = _refusal_args()
    W = torch.zeros(160, 136, dtype=BF16, device=DEV)
    e8 = torch.zeros(136, dtype=torch.int8, device=DEV)
    for other, up in ((_lib.ACC_DENSE, None), (_lib.ACC_DENSE_FP8, e8), (_lib.ACC_LOWRANK, W)):
        arr = (_lib.LayerArgs * 2)()
        for i in (0, 1):
            ctypes.memmove(ctypes.addressof(arr[i]), ctypes.addressof(arr1[0]), ctypes.sizeof(_lib.LayerArgs))
        arr[1].acc_down, arr[1].acc_kind, arr[1].acc_up = W.data_ptr(), other, None if up is None else up.data_ptr()
        assert lib.sow_forward_skinny(arr, 2, _lib.BF16, E._stream()) == ERR_UNSUPPORTED, other
    arr1[0].acc_up = None
    assert lib.sow_forward_skinny(arr1, 1, _lib.BF16, E._stream()) == _lib.ERR_NULL
    with _lib.switch(NO_SKINNY=1):
        _, _, arr2 = _refusal_args()
        assert lib.sow_forward_skinny(arr2, 1, _lib.BF16, E._stream()) == ERR_UNSUPPORTED
    F8._untouched(o, "mixed kinds")


# ---- 8. the module surface -----------------------------------------------------------------------------------------------------------
def _cabi_y(m, xin):
    """The C-ABI MXFP4 skinny result of one projection from the module's own tensors."""
    assert m.acc_quantized() and m.acc_downweight.dtype == torch.uint8 and m.acc_exponent.dtype == torch.uint8
    assert tuple(m.acc_downweight.shape) == (m.in_features // 2, m.out_features)
    assert tuple(m.acc_exponent.shape) == (m.in_features // 32, m.out_features) and not m.acc_downweight.requires_grad
    d = dict(x=xin.reshape(-1, xin.shape[-1]).cpu(), A=m.downscale_weights[0].data.cpu(), B=m.upscale_weights[0].data.cpu(),
             bias=None if m.bias is None else m.bias.data.cpu(), q=m.acc_downweight.data.cpu(), e=m.acc_exponent.cpu(), s=float(m.scale))
    (y,) = _run(xin.dtype, [d], runs=(0xFF,), what="module projection")
    return y, d


@pytest.mark.parametrize("T", [4, 17])
def test_module_no_grad_generation_step(monkeypatch, T):
    net = S._stack()
    assert quantize_accumulators(net, fmt="mxfp4") == 14 and quantize_accumulators(net, fmt="mxfp4") == 0
    assert quantize_accumulators(net) == 0, "already quantised, in the other format"
    calls = S._count_skinny(monkeypatch)
    x = torch.randn(T, 1, 512, generator=torch.Generator().manual_seed(2)).to(DEV, BF16)
    rec = []
    with torch.no_grad():
        out = net(x, rec)
    assert out.shape == (T, 1, 512) and len(rec) == 14
    assert calls == [3, 1, 2, 1, 3, 1, 2, 1], calls
    for i, (m, xin, y) in enumerate(rec):
        want, d = _cabi_y(m, xin)
        assert torch.equal(E._bits(y.reshape(-1, y.shape[-1]).cpu()), E._bits(want)), f"projection {i}"
        if T == 4:
            _check(f"module_T{T}_proj{i}", BF16, dict(d, W=R.dequantize(d["q"], d["e"], BF16)), want)
    # the library's switch: the module falls back to the image and the existing path, and still answers -- on W^
    twin = copy.deepcopy(net)
    assert dequantize_accumulators(twin) == 14
    with _lib.switch(NO_SKINNY=1), torch.no_grad():
        rec2, rec3 = [], []
        net(x, rec2)
        twin(x, rec3)
    for (_, _, a), (_, _, b), (_, _, c) in zip(rec, rec2, rec3):
        assert a.shape == b.shape and torch.equal(E._bits(b), E._bits(c))


def _pair(d, r, dtype, group, seed=5, fmt="mxfp4"):
    """A quantised net and its unquantised twin whose accumulators are W^."""
    from sow_amd import group_siblings
    q = F8._Attn(d, r, dtype, group, seed)
    assert quantize_accumulators(q, fmt=fmt, strict=True) == len(q.names)
    u = copy.deepcopy(q)
    assert dequantize_accumulators(u) == len(u.names)
    for m in u.layers():
        assert not m.acc_quantized() and m.acc_downweight.dtype == dtype and "acc_exponent" not in m.state_dict()
        assert tuple(m.acc_downweight.shape) == (d, d)
    if group:
        assert group_siblings(q) == 1 and group_siblings(u) == 1
    return q, u


@pytest.mark.parametrize("sink", [False, True], ids=["autograd", "bucket"])
@pytest.mark.parametrize("group", [False, True], ids=["single", "qkv"])
@pytest.mark.parametrize("T", [64, 8193])
def test_module_training_equals_unquantised_twin(T, group, sink):
    d, r = 288, 16
    q, u = _pair(d, r, BF16, group)
    g = torch.Generator().manual_seed(T)
    x, dy = torch.randn(T, d, generator=g).to(DEV, BF16), torch.randn(T, d, generator=g).to(DEV, BF16)
    got, want = F8._train_step(q, x, dy, sink), F8._train_step(u, x, dy, sink)
    for k in want:
        assert torch.equal(E._bits(got[k]), E._bits(want[k])), f"{k} differs from the unquantised twin"
    assert float(got["dx"].float().abs().max()) > 0 and all(m.acc_downweight.dtype == torch.uint8 for m in q.layers())
    # no-grad at T > 32: the image and the existing forward
    with torch.no_grad():
        assert torch.equal(E._bits(q(x)), E._bits(u(x)))


def test_module_f16_training_equals_unquantised_twin():
    q, u = _pair(288, 16, F16, True, seed=8)
    g = torch.Generator().manual_seed(1)
    x, dy = torch.randn(64, 288, generator=g).to(DEV, F16), torch.randn(64, 288, generator=g).to(DEV, F16)
    got, want = F8._train_step(q, x, dy, False), F8._train_step(u, x, dy, False)
    for k in want:
        assert torch.equal(E._bits(got[k]), E._bits(want[k])), k


def test_siblings_of_differing_kinds_take_per_layer_calls(monkeypatch):
    """q as MXFP4, k as E4M3, v unquantised: no call of the library takes the three, each layer answers on its own."""
    from sow_amd import group_siblings
    net = F8._Attn(288, 16, BF16, True, seed=14)
    ms = net.layers()
    assert quantize_accumulators(ms[0], fmt="mxfp4") == 1
    assert quantize_accumulators(ms[1], fmt="fp8_e4m3") == 1
    twin = copy.deepcopy(net)
    assert dequantize_accumulators(twin) == 2
    assert group_siblings(net) == 1
    x = torch.randn(4, 288, generator=torch.Generator().manual_seed(2)).to(DEV, BF16)
    with torch.no_grad():
        wants = [m(x) for m in twin.layers()]
    calls = S._count_skinny(monkeypatch)
    with torch.no_grad():
        ys = [m(x) for m in ms]
    assert calls == [1, 1, 1], calls
    (y0, _), = [_cabi_y(ms[0], x)]
    assert torch.equal(E._bits(ys[0].cpu()), E._bits(y0))
    assert torch.equal(E._bits(ys[2]), E._bits(wants[2])), "the unquantised sibling computes what it computes alone"
    for a, b in zip(ys, wants):
        assert a.shape == b.shape and bool(torch.isfinite(a).all())


def test_two_layers_share_the_arena():
    """y = L2(L1(x)) with two quantised layers of one shape: L2's forward overwrites L1's image in the arena, so L1's backward
    is only right when it builds its image again (an image saved for backward would hold L2's accumulator)."""
    q1, u1 = _pair(288, 16, BF16, False, seed=11)
    q2, u2 = _pair(288, 16, BF16, False, seed=12)
    g = torch.Generator().manual_seed(3)
    x, dy = torch.randn(64, 288, generator=g).to(DEV, BF16), torch.randn(64, 288, generator=g).to(DEV, BF16)
    res = []
    for l1, l2 in ((q1, q2), (u1, u2)):
        xin = x.clone().requires_grad_(True)
        l2(l1(xin)).backward(dy)
        res.append([xin.grad.clone()] + [m.downscale_weights[0].grad.clone() for m in l1.layers() + l2.layers()])
    for a, b in zip(*res):
        assert torch.equal(E._bits(a), E._bits(b))
    assert ops._ARENAS[(x.device, BF16)].numel() >= 288 * 288 * 2      # the arena of the E4M3 images, by (device, dtype)


def test_state_dict_round_trip_and_format_changes():
    net = S._stack()
    plain_sd = {k: v.clone() for k, v in net.state_dict().items()}
    plain_keys = set(plain_sd)
    assert quantize_accumulators(net, fmt="mxfp4") == 14
    sd = net.state_dict()
    assert set(sd.keys()) == plain_keys | {k.replace("acc_downweight", "acc_exponent") for k in plain_keys if k.endswith("acc_downweight")}
    fresh = S._stack()                    # freshly prepared, unquantised; other accumulator values
    for m in fresh.modules():
        if hasattr(m, "acc_downweight"):
            m.acc_downweight.data.mul_(3)
    res = fresh.load_state_dict(sd, strict=True, assign=True)
    assert not res.missing_keys and not res.unexpected_keys
    sd2 = fresh.state_dict()
    assert list(sd2.keys()) == list(sd.keys())
    for k, v in sd.items():
        assert sd2[k].dtype == v.dtype and torch.equal(F8._raw(sd2[k]), F8._raw(v)), k
    assert sum(getattr(m, "acc_quantized", lambda: False)() for m in fresh.modules()) == 14
    x = torch.randn(4, 1, 512, generator=torch.Generator().manual_seed(2)).to(DEV, BF16)
    with torch.no_grad():
        y4 = net(x, [])
        assert torch.equal(E._bits(y4), E._bits(fresh(x, [])))
    # without assign: the codes are copied as codes; into an unquantised model and into an E4M3 one
    fp8 = S._stack()
    assert quantize_accumulators(fp8) == 14
    sd8 = {k: v.clone() for k, v in fp8.state_dict().items()}
    for other in (S._stack(), fp8):
        other.load_state_dict(sd, strict=True)
        for k, v in sd.items():
            got = other.state_dict()[k]
            assert got.dtype == v.dtype and torch.equal(F8._raw(got), F8._raw(v)), k
        with torch.no_grad():
            assert torch.equal(E._bits(other(x, [])), E._bits(y4))
    # the other directions: an E4M3 and an unquantised state dict into the MXFP4 model
    for src in (sd8, plain_sd):
        dst = copy.deepcopy(net)
        dst.load_state_dict(src, strict=True)
        for k, v in src.items():
            got = dst.state_dict()[k]
            assert got.dtype == v.dtype and got.shape == v.shape and torch.equal(F8._raw(got), F8._raw(v)), k
        assert set(dst.state_dict().keys()) == set(src.keys())
    # .half() / .bfloat16() / .to(device) keep the codes codes
    half = copy.deepcopy(net).half()
    m, m0 = half.layers[0].self_attn.q_proj, net.layers[0].self_attn.q_proj
    assert m.acc_downweight.dtype == torch.uint8 and m.acc_exponent.dtype == torch.uint8 and m.downscale_weights[0].dtype == F16
    assert torch.equal(m.acc_downweight, m0.acc_downweight) and torch.equal(m.acc_exponent, m0.acc_exponent)
    back = half.bfloat16().to("cpu").to(DEV)
    m = back.layers[0].self_attn.q_proj
    assert m.acc_downweight.dtype == torch.uint8 and m.acc_downweight.is_cuda and m.downscale_weights[0].dtype == BF16
    assert torch.equal(m.acc_downweight, m0.acc_downweight) and torch.equal(m.acc_exponent, m0.acc_exponent)
    with torch.no_grad():
        assert torch.equal(E._bits(back(x, [])), E._bits(y4))


def test_strict_and_untouched_layers():
    from sow_amd import SoWLinear
    none = SoWLinear(64, 64, bias=False, rank=8, init_method="normal", device=DEV, dtype=BF16)
    assert quantize_accumulators(none, fmt="mxfp4") == 0 and not none.acc_quantized()
    with pytest.raises(ValueError):
        quantize_accumulators(none, fmt="mxfp4", strict=True)
    for d_in, d_out in ((72, 64), (64, 60)):          # d_in % 32, d_out % 8
        odd = SoWLinear(d_in, d_out, bias=False, rank=8, init_method="normal", device=DEV, dtype=BF16)
        odd.acc_downweight = nn.Parameter(torch.randn(d_in, d_out, device=DEV, dtype=BF16), requires_grad=False)
        assert quantize_accumulators(odd, fmt="mxfp4") == 0 and odd.acc_downweight.dtype == BF16
        with pytest.raises(ValueError):
            quantize_accumulators(odd, fmt="mxfp4", strict=True)
    with pytest.raises(ValueError):
        quantize_accumulators(none, fmt="nf4")


def test_accumulate_raises_and_dequantize_returns_the_image():
    import sow_amd
    q, _ = _pair(288, 16, BF16, False, seed=21)
    (m,) = q.layers()
    codes, scales = m.acc_downweight.data.cpu(), m.acc_exponent.cpu()
    A0 = m.downscale_weights[0].data.clone()
    with pytest.raises(RuntimeError, match="dequantize_accumulators"):
        m.accumulate()
    with pytest.raises(RuntimeError, match="dequantize_accumulators"):
        sow_amd.accumulate(q)
    assert torch.equal(m.downscale_weights[0].data, A0) and m.acc_quantized()
    assert dequantize_accumulators(q) == 1 and dequantize_accumulators(q) == 0
    assert m.acc_downweight.dtype == BF16 and not m.acc_downweight.requires_grad and not m.acc_quantized()
    assert torch.equal(m.acc_downweight.data.cpu().view(torch.int16), R.dequantize_bits(codes, scales, BF16))
    m.accumulate()        # an ordinary layer again


# ---- 9. HIP graph capture and in-place replay -----------------------------------------------------------------------------------------
def test_graph_replay_skinny():
    lib = _lib.load()
    dtype, T, d_in, d_out, r = BF16, 17, 544, 264, 8
    I = [_quantised(dict(S._gauss(dtype, T, d_in, d_out, r, True, "dense", seed=60 + 7 * k), s=1.0)) for k in (0, 1)]
    I[1] = dict(I[1], x=I[1]["x"] * 0.5)
    b = GR.Bound("fp4_skinny")
    ar = b.arena(dtype)
    x, A, B, bias = (b.input(ar, (I[0][k], I[1][k])) for k in ("x", "A", "B", "bias"))
    q = b.extra(None, _guarded_bytes(I[0]["q"], 0x77), (I[0]["q"], I[1]["q"]))
    e = b.extra(None, _guarded_bytes(I[0]["e"], 254), (I[0]["e"], I[1]["e"]))
    y = b.output(ar, "y", (T, d_out))
    ws = b.workspace(ar, lib.sow_forward_skinny_fp4_workspace_bytes(T, d_in, d_out, r, E._dt(dtype)))
    arr = (_lib.LayerArgs * 1)()
    a = arr[0]
    a.x, a.A, a.B, a.acc_down, a.acc_up, a.bias, a.y = (t.data_ptr() for t in (x, A, B, q, e, bias, y))
    a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, KIND, 1.0
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    b.call = lambda rc: rc(lib.sow_forward_skinny(arr, 1, E._dt(dtype), E._stream()), "sow_forward_skinny")
    b.check = lambda k, out: _check(f"graph_I{k + 1}", dtype, I[k], out["y"])
    trace = []
    GR.replay(b, trace)
    assert GR.has_kernel(trace, "skinny_a_kernel") and GR.has_kernel(trace, "skinny_b_kernel"), sorted(set(trace))


def test_graph_replay_module_forward_backward():
    """One quantised layer's forward + backward at T = 64, captured: the image pass is part of the graph (twice: autograd saves
    the codes), so replays on x, dY, codes and scales changed in place equal the eager twins."""
    dtype, T, d = BF16, 64, 288
    nets = [_pair(d, 16, dtype, False, seed=31 + k)[0] for k in (0, 1)]
    (m,), (m2,) = nets[0].layers(), nets[1].layers()
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(T, d, generator=g).to(dtype) * s for s in (1.0, 0.5)]
    dys = [torch.randn(T, d, generator=g).to(dtype) for _ in (0, 1)]
    b = GR.Bound("fp4_module")
    ar = b.arena(dtype)
    x, dy = b.input(ar, (xs[0], xs[1])), b.input(ar, (dys[0], dys[1]))
    b.extra(None, m.acc_downweight.data, tuple(n.layers()[0].acc_downweight.data.clone() for n in nets))
    b.extra(None, m.acc_exponent, tuple(n.layers()[0].acc_exponent.clone() for n in nets))
    outs = {k: b.output(ar, k, s) for k, s in (("y", (T, d)), ("dx", (T, d)), ("dA", (d, 16)), ("dB", (16, d)), ("dbias", (d,)))}
    params = (m.downscale_weights[0], m.upscale_weights[0], m.bias)

    def call(rc):
        for p in params:
            p.grad = None
        xin = x.detach().requires_grad_(True)
        yy = nets[0](xin)
        yy.backward(dy)
        for k, v in zip(("y", "dx", "dA", "dB", "dbias"), (yy.detach(), xin.grad, *(p.grad for p in params))):
            outs[k].copy_(v)

    b.call = call

    def check(k, out):
        # the unquantised twin of input set k, eagerly
        u = copy.deepcopy(nets[k])
        dequantize_accumulators(u)
        (mu,) = u.layers()
        with torch.no_grad():
            for dst, src in zip((mu.downscale_weights[0], mu.upscale_weights[0], mu.bias), params):
                dst.copy_(src)
        want = F8._train_step(u, xs[k].to(DEV), dys[k].to(DEV), False)
        for key in ("y", "dx"):
            assert torch.equal(E._bits(out[key]), E._bits(want[key].cpu())), key
        for key, wk in (("dA", "dA0"), ("dB", "dB0"), ("dbias", "dbias0")):
            assert torch.equal(E._bits(out[key]), E._bits(want[wk].cpu())), key

    b.check = check
    trace = []
    GR.replay(b, trace)
    assert GR.has_kernel(trace, "cast_copy_kernel"), sorted(set(trace))


def test_zz_report_worst_ratios():
    worst = {k: v for k, v in S.WORST.items() if k.startswith("fp4_")}
    for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:10]:
        print(f"{k}: worst err / bound {v:.3f}")
    assert worst and all(v <= 1.0 for v in worst.values())
