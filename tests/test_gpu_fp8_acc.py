"""-m gpu: FP8 (E4M3) dense accumulators -- include/sow_amd.h SOW_ACC_DENSE_FP8, sow_acc_dequantize, sow_amd.quantize_accumulators.

The contract: a quantised layer computes what the dense-accumulator layer computes on the dequantised matrix
W^ = codes * 2^exponents, which is exactly a number of the compute dtype.  So nothing here has a tolerance of its own:
* the quantiser and the image pass are compared bit for bit with the float64 / integer reference of fp8_acc_ref.py;
* the FP8 skinny forward is held, element by element, to test_gpu_skinny._reference / numerics.bound with W := W^, through
  test_gpu_skinny's buffer protocol (NaN neighbours, sentinel guards, poisoned / zeroed / poisoned memory, three runs
  bit-identical), and bit for bit on value_plan's exact operands;
* the module paths are bit-identical to the C-ABI call (no-grad, T <= 32) or to an unquantised twin whose accumulator IS W^
  (larger T, training, FactorBucket sinks, sibling groups), and so are their HIP-graph replays.
"""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn

import fp8_acc_ref as R
import graph_replay as GR
import test_gpu_elementwise as E
import test_gpu_skinny as S
import value_plan as VP
from numerics import fp32_floor, rne, to64, ulp
from sow_amd import _lib, dequantize_accumulators, acc_quant, ops, quantize_accumulators

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
DT = S.DT
FP8 = torch.float8_e4m3fn
ERR_UNSUPPORTED = -6
KIND = _lib.ACC_DENSE_FP8
GUARD = 64
DENSE_CASES = [c for c in S.CASES if c[7] == "dense"]


def _quant(W):
    """(codes uint8, exps int8, W^ in W's dtype) on the CPU.  Small matrices through the reference; the long-slab shapes
    through the package's quantiser on the GPU, which test_quantiser_* tie to the reference bit for bit."""
    if W.numel() <= 1 << 20:
        codes, exps = R.quantize(W)
    else:
        q, e = acc_quant.quantize_tensor(W.to(DEV))
        codes, exps = q.view(torch.uint8).cpu(), e.cpu()
    img = R.dequantize(codes, exps)
    what = img.to(W.dtype)
    assert bool((what.double() == img).all()), "W^ is not a number of the compute dtype"
    return codes, exps, what


def _quantised(d):
    """The operands of a layer with W replaced by its quantisation: W = W^ (what the reference sees), q / e = what the kernel
    reads."""
    codes, exps, what = _quant(d["W"])
    return dict(d, W=what, q=codes, e=exps)


def _guarded_bytes(t, fill):
    """A uint8 / int8 operand between guards of `fill` (the NaN code 0x7F around the codes: a read past them is a NaN in y)."""
    buf = torch.full((t.numel() + 2 * GUARD,), fill, dtype=t.dtype, device=DEV)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _run(dtype, layers, x_shared=False, runs=(0xFF, 0x00, 0xFF), what="fp8 skinny"):
    """test_gpu_skinny._run for layers with an E4M3 accumulator (dicts from _quantised; "q" absent: no accumulator)."""
    lib = _lib.load()
    ar = E.Arena(dtype)
    arr = (_lib.LayerArgs * len(layers))()
    ys, keep = [], []
    x0 = None
    for i, d in enumerate(layers):
        x = x0 if (x_shared and x0 is not None) else ar.input(d["x"])
        x0 = x0 if x0 is not None else x
        A, B, bias = (ar.input(d.get(k)) for k in ("A", "B", "bias"))
        fp8 = d.get("q") is not None
        q = _guarded_bytes(d["q"], 0x7F) if fp8 else None
        e = _guarded_bytes(d["e"], 127) if fp8 else None
        T, d_in = d["x"].shape
        r, d_out = d["B"].shape
        kind = KIND if fp8 else _lib.ACC_NONE
        y = ar.output((T, d_out))
        nws = (lib.sow_forward_skinny_fp8_workspace_bytes(T, d_in, d_out, r, E._dt(dtype)) if fp8
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


def _raw(t):
    """The bits of a tensor of any of the dtypes a quantised state dict holds."""
    return t.view(torch.uint8) if t.element_size() == 1 else GR.bits(t)


def _tie_margin(dtype, d):
    """How far the projection h = s x A (float64) stays from the rounding midpoints of `dtype`, in units of the fp32 noise of
    the kernel's sum.  test_gpu_skinny._reference rounds the EXACT h; the kernel rounds an fp32 sum, and where the exact value
    lies closer to a midpoint than that sum's noise the two may round apart -- y then moves by ulp(h) B[j, n], which is no
    error of the kernel and which the comparator has no term for.  The noise: a wave adds at most 8 MFMA steps, the workgroup
    4 waves, phase B at most 29 slabs -- fewer than 64 fp32 roundings, each at most u32 of a partial sum: fp32_floor(sq, 64).
    Elements whose half-ulp is itself below that noise (small |h|, f16) do not count: their flip moves y by less than
    2 noise |B|, about 40 s |B| / sqrt(d_in) of the fp32 floor in y's own bound for these Gaussian operands -- under a fifth."""
    x, A, s = to64(d["x"]), to64(d["A"]), d["s"]
    h = s * (x @ A)
    half, noise = ulp(h, dtype) / 2, fp32_floor(s * s * (x * x) @ (A * A), 64)
    m = (half - (h - rne(h, dtype)).abs()) / noise
    return float(torch.where(half > noise, m, torch.full_like(m, float("inf"))).min())


def _gauss_clear_of_ties(dtype, T, d_in, d_out, r, bias, s, seed):
    """test_gpu_skinny's Gaussian operands with every projection clear of a rounding tie (_tie_margin > 1), decided on the CPU
    from x and A alone before anything runs: where a column of h comes too close, elements of that column of A are moved by
    one ulp, in turn, until it does not (each move shifts the column's h by about s x[t, k] ulp(A), far more than the noise)."""
    d = dict(S._gauss(dtype, T, d_in, d_out, r, bias, "dense", seed=seed), s=s)
    A = d["A"] = d["A"].clone()
    for j in range(r):
        for k in range(64):
            if _tie_margin(dtype, dict(x=d["x"], A=A[:, j:j + 1], s=s)) > 1:
                break
            A[k:k + 1, j].view(torch.int16).add_(1)
        else:
            raise AssertionError(f"column {j} of h stays on a rounding tie")
    assert _tie_margin(dtype, d) > 1
    return d


def _check(name, dtype, d, y):
    """test_gpu_skinny's comparator on W^ (d["W"]): no other tolerance."""
    return S._check("fp8_" + name, dtype, {k: v for k, v in d.items() if k not in ("q", "e")}, y)


# ---- the quantiser ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("shape", [(264, 520), (1032, 72)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_quantiser_matches_the_reference_bit_for_bit(dt, shape):
    dtype = DT[dt]
    g = torch.Generator().manual_seed(shape[0] + (1 if dt == "f16" else 0))
    W = (torch.randn(*shape, generator=g) * 0.02).to(dtype)
    tiny = float(torch.tensor([1], dtype=torch.int16).view(dtype))
    W[:, 3] = 0                                                          # a column of zeros: e = 0
    W[:, 9] = (torch.randint(-40, 41, (shape[0],), generator=g) * tiny).to(dtype)   # subnormal magnitude
    W[:, 17] = (torch.randn(shape[0], generator=g) * 8000).to(dtype)     # the f16 upper clamp ...
    W[0, 17] = 65504.0                                                   # ... past it: 65504 > 448 * 2^7
    W[:, 25] = (torch.randn(shape[0], generator=g) * 2.0 ** -18).to(dtype)          # the f16 lower clamp: e = -15 clamps amax ~ 2^-16
    W[:, 33] = (torch.randn(shape[0], generator=g).clamp(-1, 1) * 448 * 2.0 ** -15).to(dtype)
    codes, exps = R.quantize(W)
    q, e = acc_quant.quantize_tensor(W.to(DEV))
    assert q.is_cuda and q.dtype == FP8 and e.dtype == torch.int8 and q.is_contiguous()
    assert torch.equal(e.cpu(), exps), "exponents"
    bad = q.view(torch.uint8).cpu() != codes
    assert not bad.any(), f"{int(bad.sum())} codes differ from the reference; first at {tuple(int(v) for v in torch.nonzero(bad)[0])}"
    assert int(exps[3]) == 0
    if dt == "f16":
        assert int(exps[17]) == 7 and int(exps[25]) == -15 and int(exps[9]) == -15
    assert not bool(((codes & 0x7F) == 0x7F).any()), "a NaN code was emitted"


def test_quantiser_refuses_non_finite():
    W = torch.zeros(16, 16, dtype=BF16, device=DEV)
    W[3, 4] = float("inf")
    with pytest.raises(ValueError):
        acc_quant.quantize_tensor(W)


# ---- the image pass ----------------------------------------------------------------------------------------------------------
def _dequant(codes, exps, dtype, ldd=None, sentinel=-7.25):
    """sow_acc_dequantize into a [d_in, ldd] buffer full of sentinels, between guards; returns (image, whole buffer) on the CPU."""
    d_in, d_out = codes.shape
    ldd = ldd or d_out
    buf = torch.full((d_in * ldd + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
    out = buf[GUARD:GUARD + d_in * ldd].view(d_in, ldd)
    q, e = _guarded_bytes(codes, 0x7F), _guarded_bytes(exps, 127)
    rc = _lib.load().sow_acc_dequantize(q.data_ptr(), e.data_ptr(), d_in, d_out, out.data_ptr(), ldd, E._dt(dtype), E._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + d_in * ldd:] == sentinel).all()), "guards"
    return out[:, :d_out].cpu(), out.cpu()


def _same_image(got, codes, exps, dtype):
    want = (codes.view(FP8).float() * torch.exp2(exps.float())).to(dtype)        # exact at every step
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "NaN codes must give NaN and nothing else does"
    assert torch.equal(E._bits(got)[~nan], E._bits(want)[~nan])
    return nan


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_dequantise_every_code_in_every_column_position(dt):
    """256 rows x 64 columns: column j sees all 256 codes (code (row + j) mod 256), the exponent changes every 16 columns, so
    every code meets every position modulo 16 under every exponent of {-15, -9, 0, 7}."""
    dtype = DT[dt]
    rows, cols = torch.arange(256).view(-1, 1), torch.arange(64).view(1, -1)
    codes = ((rows + cols * 5) % 256).to(torch.uint8)
    for shift in range(4):
        exps = torch.tensor([-15, -9, 0, 7], dtype=torch.int8).roll(shift).repeat_interleave(16)
        got, _ = _dequant(codes, exps, dtype)
        nan = _same_image(got, codes, exps, dtype)
        assert int(nan.sum()) == 2 * 64, "each column holds the two NaN codes once"
        assert bool((got.double()[~nan] == R.dequantize(codes, exps)[~nan]).all()), "against the integer reference"


@pytest.mark.parametrize("dt,shape", [("bf16", (264, 520)), ("f16", (520, 264))])
def test_dequantise_shapes_and_row_pitch(dt, shape):
    dtype = DT[dt]
    g = torch.Generator().manual_seed(7)
    codes = torch.randint(0, 256, shape, generator=g).to(torch.uint8)
    exps = torch.randint(-15, 8, (shape[1],), generator=g).to(torch.int8)
    got, _ = _dequant(codes, exps, dtype)
    _same_image(got, codes, exps, dtype)
    # ldd > d_out: the gap keeps its sentinels
    got, whole = _dequant(codes, exps, dtype, ldd=shape[1] + 24)
    _same_image(got, codes, exps, dtype)
    assert bool((whole[:, shape[1]:] == -7.25).all()), "the gap between rows was written"
    # the wrapper
    img = ops.acc_dequantize(codes.to(DEV).view(FP8), exps.to(DEV), dtype)
    _same_image(img.cpu(), codes, exps, dtype)


def test_dequantise_refusals():
    lib = _lib.load()
    q = torch.zeros(64, 64, dtype=torch.uint8, device=DEV)
    e = torch.zeros(64, dtype=torch.int8, device=DEV)
    out = torch.full((64, 64), -7.25, dtype=BF16, device=DEV)
    call = lambda d_out, ldd, dt, qp=q.data_ptr(): lib.sow_acc_dequantize(qp, e.data_ptr(), 64, d_out, out.data_ptr(), ldd, dt, E._stream())  # noqa: E731
    assert call(60, 64, _lib.BF16) == ERR_UNSUPPORTED and call(64, 60, _lib.BF16) == _lib.ERR_SHAPE
    assert call(64, 64, _lib.F32) == _lib.ERR_DTYPE and call(56, 60, _lib.BF16) == ERR_UNSUPPORTED
    assert call(64, 64, _lib.BF16, q.data_ptr() + 4) == -4
    torch.cuda.synchronize()
    assert bool((out == -7.25).all())


# ---- the FP8 skinny forward through the C ABI --------------------------------------------------------------------------------
@pytest.mark.parametrize("c", DENSE_CASES, ids=S._id)
def test_skinny_elementwise_against_fp64(c):
    dt, T, d_in, d_out, r, bias, s, acc = c
    dtype = DT[dt]
    d = _quantised(dict(S._gauss(dtype, T, d_in, d_out, r, bias, acc), s=s))
    (y,) = _run(dtype, [d], what=S._id(c))
    _check(S._id(c), dtype, d, y)


def test_skinny_long_k_slabs():
    """3592 -> 8200 at T = 32: 65 column ranges of 128, so the plan takes eight slabs of 512 (seven full, one of 8 rows):
    four k-steps per wave, all requested before the x slab is staged.  4360 -> 8200 plans seven slabs of 640: a fifth
    k-step per wave refills the request-ahead ring, and the last slab (520 rows) ends in a partial round.
    The operands: Gaussian as everywhere, of a seed whose projections h stay clear of rounding ties (_tie_margin): with the seed
    of test_gpu_skinny's long-slab case, h[6, 5] = -0.214355430 lies 3.9e-8 (4e-5 ulp) from a bf16 midpoint, the 8 x 512 slab plan
    of the E4M3 kernel rounds it to the other side than the 4 x 1024 plan of the bf16 one, and row 6 of y moves by ulp(h) B[5, n]."""
    lib = _lib.load()
    assert lib.sow_forward_skinny_fp8_workspace_bytes(32, 3592, 8200, 8, _lib.BF16) == 256 + 8 * 32 * (8200 + 64) * 4
    d = _quantised(_gauss_clear_of_ties(BF16, 32, 3592, 8200, 8, True, 0.5, seed=40))
    (y,) = _run(BF16, [d], what="long slabs")
    _check("long_slabs", BF16, d, y)
    assert lib.sow_forward_skinny_fp8_workspace_bytes(17, 4360, 8200, 8, _lib.F16) == 256 + (7 * 17 * 8200 * 4 + 32) + 7 * 17 * 64 * 4   # (256-aligned)
    d = _quantised(_gauss_clear_of_ties(F16, 17, 4360, 8200, 8, False, 1.0, seed=41))
    (y,) = _run(F16, [d], runs=(0xFF, 0x00), what="ring refill")
    _check("ring_refill", F16, d, y)


def _exact_fp8(c):
    """test_gpu_skinny's exact operands with W replaced by W^, and the proof again for W^ (float64, CPU): every sum the kernel
    forms is made of multiples of one unit with sum |terms| below 2^24 units.  Phase A sums x . q per column, q = W^ 2^-e: the
    same terms scaled by a power of two, exact when the sums with W^ are."""
    dtype = DT[c[0]]
    d0, _ = S._exact_operands(c)
    d = _quantised(d0)
    q = {k: to64(v) for k, v in d.items() if isinstance(v, torch.Tensor) and k not in ("q", "e")}
    x, A, B, W = q["x"], q["A"], q["B"], q["W"]
    lossless = bool((W == to64(d0["W"])).all())
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
    return d, y, lossless


@pytest.mark.parametrize("c", [c for c in S.EXACT if c[7] == "dense"], ids=S._id)
def test_skinny_exact_operands_bit_for_bit(c):
    dtype = DT[c[0]]
    d, y64, lossless = _exact_fp8(c)
    print(f"{S._id(c)}: quantising W is {'lossless' if lossless else 'lossy; exactness proved again on W^'}")
    (y,) = _run(dtype, [d], what="exact " + S._id(c))
    bad = to64(y) != rne(y64, dtype)
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} elements differ from the float64 result rounded once"


@pytest.mark.parametrize("dt,k", [("bf16", 0), ("bf16", 263), ("f16", 130)])
def test_skinny_rows_are_independent(dt, k):
    dtype = DT[dt]
    d = _quantised(dict(S._gauss(dtype, 3, 264, 520, 50, True, "dense", seed=3), s=0.5))
    (clean,) = _run(dtype, [d], runs=(0xFF,), what="rows clean")
    p = dict(d, x=d["x"].clone())
    p["x"][1, k] = float("nan")
    (poisoned,) = _run(dtype, [p], runs=(0xFF,), what="rows poisoned")
    assert bool(torch.isnan(poisoned[1]).all()), "row 1 must be NaN in every column"
    for t in (0, 2):
        assert torch.equal(E._bits(poisoned[t]), E._bits(clean[t])), f"row {t} changed"


def test_skinny_groups_equal_single_calls():
    # three siblings on ONE x buffer: 512 -> {512, 256, 256}; the second has no accumulator (the kinds that mix in one call)
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
    # different inputs and token counts, one layer without an accumulator
    pair = [_quantised(dict(S._gauss(F16, 4, 264, 520, 8, True, "dense", seed=30), s=0.25)),
            dict(S._gauss(F16, 32, 520, 264, 64, False, "none", seed=31), s=1.0),
            _quantised(dict(S._gauss(F16, 17, 1032, 72, 2, False, "dense", seed=32), s=1.0))]
    grouped = _run(F16, pair, what="mixed group")
    for i, (d, yg) in enumerate(zip(pair, grouped)):
        (ys,) = _run(F16, [d], runs=(0xFF,), what=f"mixed single {i}")
        assert torch.equal(E._bits(yg), E._bits(ys)), f"layer {i}"
        if "q" in d:
            _check(f"mixed_{i}", F16, d, yg)
        else:
            (plain,) = S._run(F16, [d], runs=(0xFF,), what="the unquantised call")
            assert torch.equal(E._bits(yg), E._bits(plain)), "a layer without accumulator computes what it computes in a plain call"


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _refusal_args(T=4, d_in=264, d_out=520, r=8, kind=KIND):
    z = lambda *s: torch.zeros(*s, dtype=BF16, device=DEV)   # noqa: E731
    t = dict(x=z(T, d_in), A=z(d_in, r), B=z(r, d_out), q=torch.zeros(d_in, d_out, dtype=torch.uint8, device=DEV),
             e=torch.zeros(d_out, dtype=torch.int8, device=DEV), bias=z(d_out), dy=z(T, d_out))
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


def _untouched(outs, what):
    torch.cuda.synchronize()
    for k, o in outs.items():
        assert bool((o.view(torch.uint8) == 0xFF).all()), f"{what}: {k} was written by a refused call"


@pytest.mark.parametrize("entry", ["sow_forward", "sow_forward_group", "sow_backward_ex", "sow_backward_group", "sow_forward_shared",
                                   "sow_backward_shared"])
def test_other_entry_points_refuse_the_kind(entry):
    lib = _lib.load()
    t, o, arr = _refusal_args()
    p = lambda v: v.data_ptr()   # noqa: E731
    st = E._stream()
    both = _lib.BWD_DATA | _lib.BWD_WEIGHTS
    if entry == "sow_forward":
        rc = lib.sow_forward(p(t["x"]), p(t["A"]), p(t["B"]), p(t["q"]), p(t["e"]), p(t["bias"]), p(o["y"]), p(o["h"]), 4, 264, 520, 8,
                             0, KIND, 1.0, _lib.BF16, p(o["ws"]), o["ws"].numel(), st)
    elif entry == "sow_backward_ex":
        rc = lib.sow_backward_ex(p(t["dy"]), p(t["x"]), p(o["h"]), p(t["A"]), p(t["B"]), p(t["q"]), p(t["e"]), p(o["dx"]), p(o["dA"]),
                                 p(o["dB"]), None, 4, 264, 520, 8, 0, KIND, 1.0, 0.0, _lib.BF16, p(o["ws"]), o["ws"].numel(), both, st)
    elif entry in ("sow_forward_group", "sow_forward_shared"):
        rc = getattr(lib, entry)(arr, 1, _lib.BF16, st)
    else:
        rc = getattr(lib, entry)(arr, 1, _lib.BF16, both, st)
    assert rc == ERR_UNSUPPORTED, rc
    _untouched(o, entry)
    # the workspace queries of those entry points know no such layer
    assert lib.sow_workspace_bytes(4, 264, 520, 8, 0, KIND, _lib.BF16) == 0
    assert lib.sow_forward_workspace_bytes(4, 264, 520, 8, 0, KIND, _lib.BF16) == 0


SKINNY_REFUSALS = [("T=33", dict(T=33)), ("r=66", dict(r=66)), ("d_out=524", dict(d_out=524)), ("d_out=523", dict(d_out=523))]


@pytest.mark.parametrize("name,kw", SKINNY_REFUSALS, ids=[r[0] for r in SKINNY_REFUSALS])
def test_skinny_refusals_touch_nothing(name, kw):
    lib = _lib.load()
    t, o, arr = _refusal_args(**kw)
    a = arr[0]
    assert lib.sow_forward_skinny_fp8_workspace_bytes(a.T, a.d_in, a.d_out, a.r_live, _lib.BF16) == 0
    assert lib.sow_forward_skinny(arr, 1, _lib.BF16, E._stream()) == ERR_UNSUPPORTED
    _untouched(o, name)


def test_skinny_refuses_two_kinds_of_dense_accumulator_and_missing_exponents():
    lib = _lib.load()
    t, o, arr1 = _refusal_args()
    arr = (_lib.LayerArgs * 2)()
    ctypes.memmove(ctypes.addressof(arr[0]), ctypes.addressof(arr1[0]), ctypes.sizeof(_lib.LayerArgs))
    ctypes.memmove(ctypes.addressof(arr[1]), ctypes.addressof(arr1[0]), ctypes.sizeof(_lib.LayerArgs))
    W = torch.zeros(264, 520, dtype=BF16, device=DEV)
    arr[1].acc_down, arr[1].acc_kind = W.data_ptr(), _lib.ACC_DENSE
    assert lib.sow_forward_skinny(arr, 2, _lib.BF16, E._stream()) == ERR_UNSUPPORTED
    arr1[0].acc_up = None
    assert lib.sow_forward_skinny(arr1, 1, _lib.BF16, E._stream()) == _lib.ERR_NULL
    _untouched(o, "two kinds")


# ---- the module surface ------------------------------------------------------------------------------------------------------------
def _cabi_y(m, xin):
    """The C-ABI FP8 skinny result of one projection from the module's own tensors."""
    assert m.acc_quantized() and m.acc_downweight.dtype == FP8
    d = dict(x=xin.reshape(-1, xin.shape[-1]).cpu(), A=m.downscale_weights[0].data.cpu(), B=m.upscale_weights[0].data.cpu(),
             bias=None if m.bias is None else m.bias.data.cpu(), q=m.acc_downweight.data.view(torch.uint8).cpu(),
             e=m.acc_exponent.cpu(), s=float(m.scale))
    (y,) = _run(xin.dtype, [d], runs=(0xFF,), what="module projection")
    return y, d


@pytest.mark.parametrize("T", [4, 17])
def test_module_no_grad_generation_step(monkeypatch, T):
    net = S._stack()
    assert quantize_accumulators(net) == 14
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
            img = R.dequantize(d["q"], d["e"]).to(BF16)
            _check(f"module_T{T}_proj{i}", BF16, dict(d, W=img), want)
    # the library's switch: the module falls back to the image and the existing path, and still answers
    with _lib.switch(NO_SKINNY=1), torch.no_grad():
        rec2 = []
        net(x, rec2)
    for (_, _, a), (_, _, b) in zip(rec, rec2):
        assert a.shape == b.shape and bool(torch.isfinite(b).all())


class _Attn(nn.Module):
    """One layer (`proj`) or q / k / v siblings on one input, d -> d, biased."""

    def __init__(self, d, r, dtype, group, seed):
        super().__init__()
        from sow_amd import SoWLinear
        g = torch.Generator().manual_seed(seed)
        self.self_attn = nn.Module()
        self.names = ("q_proj", "k_proj", "v_proj") if group else ("o_proj",)
        for nm in self.names:
            m = SoWLinear(d, d, bias=True, rank=r, init_method="normal", scale=0.5, device=DEV, dtype=dtype)
            with torch.no_grad():
                m.downscale_weights[0].copy_((torch.randn(d, r, generator=g) * 0.05).to(dtype))
                m.upscale_weights[0].copy_((torch.randn(r, d, generator=g) * 0.05).to(dtype))
                m.bias.copy_((torch.randn(d, generator=g) * 0.1).to(dtype))
            m.acc_downweight = nn.Parameter((torch.randn(d, d, generator=g) * 0.02).to(DEV, dtype), requires_grad=False)
            setattr(self.self_attn, nm, m)

    def layers(self):
        return [getattr(self.self_attn, nm) for nm in self.names]

    def forward(self, x):
        ys = [m(x) for m in self.layers()]
        return ys[0] if len(ys) == 1 else ys[0] + ys[1] * 0.5 - ys[2]


def _pair(d, r, dtype, group, seed=5):
    """A quantised net and its unquantised twin whose accumulators are W^."""
    from sow_amd import group_siblings
    q = _Attn(d, r, dtype, group, seed)
    assert quantize_accumulators(q, strict=True) == len(q.names)
    u = copy.deepcopy(q)
    assert dequantize_accumulators(u) == len(u.names)
    for m in u.layers():
        assert not m.acc_quantized() and m.acc_downweight.dtype == dtype and "acc_exponent" not in m.state_dict()
    if group:
        assert group_siblings(q) == 1 and group_siblings(u) == 1
    return q, u


def _train_step(net, x, dy, sink):
    from sow_amd import FactorBucket, factor_parameters
    bucket = None
    if sink:
        bucket = FactorBucket(factor_parameters(net, biases=True))
        assert bucket.attach(net) == len(net.names)
        bucket.zero_grad()
    xin = x.clone().requires_grad_(True)
    y = net(xin)
    y.backward(dy)
    if bucket is not None:
        bucket.finalize()
    torch.cuda.synchronize()
    out = dict(y=y.detach(), dx=xin.grad)
    for i, m in enumerate(net.layers()):
        out[f"dA{i}"], out[f"dB{i}"], out[f"dbias{i}"] = (m.downscale_weights[0].grad, m.upscale_weights[0].grad, m.bias.grad)
    assert all(v is not None for v in out.values())
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("sink", [False, True], ids=["autograd", "bucket"])
@pytest.mark.parametrize("group", [False, True], ids=["single", "qkv"])
@pytest.mark.parametrize("T", [64, 8193])
def test_module_training_equals_unquantised_twin(T, group, sink):
    d, r = 264, 16
    q, u = _pair(d, r, BF16, group)
    g = torch.Generator().manual_seed(T)
    x, dy = torch.randn(T, d, generator=g).to(DEV, BF16), torch.randn(T, d, generator=g).to(DEV, BF16)
    got, want = _train_step(q, x, dy, sink), _train_step(u, x, dy, sink)
    for k in want:
        assert torch.equal(E._bits(got[k]), E._bits(want[k])), f"{k} differs from the unquantised twin"
    assert float(got["dx"].float().abs().max()) > 0 and all(m.acc_downweight.dtype == FP8 for m in q.layers())
    # no-grad at T > 32: the image and the existing forward
    with torch.no_grad():
        assert torch.equal(E._bits(q(x)), E._bits(u(x)))


def test_module_f16_training_equals_unquantised_twin():
    q, u = _pair(264, 16, F16, True, seed=8)
    g = torch.Generator().manual_seed(1)
    x, dy = torch.randn(64, 264, generator=g).to(DEV, F16), torch.randn(64, 264, generator=g).to(DEV, F16)
    got, want = _train_step(q, x, dy, False), _train_step(u, x, dy, False)
    for k in want:
        assert torch.equal(E._bits(got[k]), E._bits(want[k])), k


def test_two_layers_share_the_arena():
    """y = L2(L1(x)) with two quantised layers of one shape: L2's forward overwrites L1's image in the arena, so L1's backward
    is only right when it builds its image again (an image saved for backward would hold L2's accumulator)."""
    q1, u1 = _pair(264, 16, BF16, False, seed=11)
    q2, u2 = _pair(264, 16, BF16, False, seed=12)
    g = torch.Generator().manual_seed(3)
    x, dy = torch.randn(64, 264, generator=g).to(DEV, BF16), torch.randn(64, 264, generator=g).to(DEV, BF16)
    res = []
    for l1, l2 in ((q1, q2), (u1, u2)):
        xin = x.clone().requires_grad_(True)
        l2(l1(xin)).backward(dy)
        res.append([xin.grad.clone()] + [m.downscale_weights[0].grad.clone() for m in l1.layers() + l2.layers()])
    for a, b in zip(*res):
        assert torch.equal(E._bits(a), E._bits(b))
    key = (x.device, BF16)
    assert ops._ARENAS[key].numel() >= 264 * 264 * 2


def test_state_dict_round_trip():
    net = S._stack()
    plain_keys = set(net.state_dict().keys())
    assert not any(k.endswith("acc_exponent") for k in plain_keys)
    assert quantize_accumulators(net) == 14 and quantize_accumulators(net) == 0
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
        assert sd2[k].dtype == v.dtype and torch.equal(_raw(sd2[k]), _raw(v)), k
    assert sum(getattr(m, "acc_quantized", lambda: False)() for m in fresh.modules()) == 14
    x = torch.randn(4, 1, 512, generator=torch.Generator().manual_seed(2)).to(DEV, BF16)
    with torch.no_grad():
        assert torch.equal(E._bits(net(x, [])), E._bits(fresh(x, [])))
    # without assign: the codes are copied as codes
    other = S._stack()
    other.load_state_dict(sd, strict=True)
    for k, v in sd.items():
        assert torch.equal(_raw(other.state_dict()[k]), _raw(v)), k
    # .half() keeps the codes codes
    half = copy.deepcopy(net).half()
    m = half.layers[0].self_attn.q_proj
    assert m.acc_downweight.dtype == FP8 and m.downscale_weights[0].dtype == F16
    assert torch.equal(m.acc_downweight.view(torch.uint8), net.layers[0].self_attn.q_proj.acc_downweight.view(torch.uint8))


def test_strict_and_untouched_layers():
    from sow_amd import SoWLinear
    none = SoWLinear(64, 64, bias=False, rank=8, init_method="normal", device=DEV, dtype=BF16)
    assert quantize_accumulators(none) == 0 and not none.acc_quantized()
    with pytest.raises(ValueError):
        quantize_accumulators(none, strict=True)
    ragged = SoWLinear(60, 64, bias=False, rank=8, init_method="normal", device=DEV, dtype=BF16)
    ragged.acc_downweight = nn.Parameter(torch.randn(60, 64, device=DEV, dtype=BF16), requires_grad=False)
    assert quantize_accumulators(ragged) == 0 and ragged.acc_downweight.dtype == BF16


def test_accumulate_raises_and_dequantize_returns_the_image():
    import sow_amd
    q, _ = _pair(264, 16, BF16, False, seed=21)
    (m,) = q.layers()
    codes, exps = m.acc_downweight.data.view(torch.uint8).cpu(), m.acc_exponent.cpu()
    A0 = m.downscale_weights[0].data.clone()
    with pytest.raises(RuntimeError, match="dequantize_accumulators"):
        m.accumulate()
    with pytest.raises(RuntimeError, match="dequantize_accumulators"):
        sow_amd.accumulate(q)
    assert torch.equal(m.downscale_weights[0].data, A0) and m.acc_quantized()
    assert dequantize_accumulators(q) == 1 and dequantize_accumulators(q) == 0
    want = R.dequantize(codes, exps)
    assert m.acc_downweight.dtype == BF16 and not m.acc_downweight.requires_grad and not m.acc_quantized()
    assert bool((m.acc_downweight.data.cpu().double() == want).all())
    m.accumulate()        # an ordinary layer again


# ---- HIP graph capture and in-place replay -------------------------------------------------------------------------------------------
def test_graph_replay_skinny():
    lib = _lib.load()
    dtype, T, d_in, d_out, r = BF16, 17, 520, 264, 8
    I = [_quantised(dict(S._gauss(dtype, T, d_in, d_out, r, True, "dense", seed=60 + 7 * k), s=1.0)) for k in (0, 1)]
    I[1] = dict(I[1], x=I[1]["x"] * 0.5)
    b = GR.Bound("fp8_skinny")
    ar = b.arena(dtype)
    x, A, B, bias = (b.input(ar, (I[0][k], I[1][k])) for k in ("x", "A", "B", "bias"))
    q = b.extra(None, _guarded_bytes(I[0]["q"], 0x7F), (I[0]["q"], I[1]["q"]))
    e = b.extra(None, _guarded_bytes(I[0]["e"].view(torch.uint8), 127), (I[0]["e"].view(torch.uint8), I[1]["e"].view(torch.uint8)))
    y = b.output(ar, "y", (T, d_out))
    ws = b.workspace(ar, lib.sow_forward_skinny_fp8_workspace_bytes(T, d_in, d_out, r, E._dt(dtype)))
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
    the codes), so replays on x, dY, codes and exponents changed in place equal the eager twins."""
    dtype, T, d = BF16, 64, 264
    nets = [_pair(d, 16, dtype, False, seed=31 + k)[0] for k in (0, 1)]
    (m,), (m2,) = nets[0].layers(), nets[1].layers()
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(T, d, generator=g).to(dtype) * s for s in (1.0, 0.5)]
    dys = [torch.randn(T, d, generator=g).to(dtype) for _ in (0, 1)]
    b = GR.Bound("fp8_module")
    ar = b.arena(dtype)
    x, dy = b.input(ar, (xs[0], xs[1])), b.input(ar, (dys[0], dys[1]))
    b.extra(None, m.acc_downweight.data.view(torch.uint8), tuple(n.layers()[0].acc_downweight.data.view(torch.uint8).clone() for n in nets))
    b.extra(None, m.acc_exponent.view(torch.uint8), tuple(n.layers()[0].acc_exponent.view(torch.uint8).clone() for n in nets))
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
        want = _train_step(u, xs[k].to(DEV), dys[k].to(DEV), False)
        for key in ("y", "dx"):
            assert torch.equal(E._bits(out[key]), E._bits(want[key].cpu())), key
        for key, wk in (("dA", "dA0"), ("dB", "dB0"), ("dbias", "dbias0")):
            assert torch.equal(E._bits(out[key]), E._bits(want[wk].cpu())), key

    b.check = check
    trace = []
    GR.replay(b, trace)
    assert GR.has_kernel(trace, "cast_copy_kernel"), sorted(set(trace))


def test_arena_does_not_grow_during_capture(monkeypatch):
    """The arena is sized to the largest single call and grows only outside a capture (the capturing state is faked here: the
    refusal is a host decision taken before anything is launched)."""
    q, _ = _pair(520, 16, BF16, False, seed=41)
    (m,) = q.layers()
    x = torch.randn(64, 520, device=DEV, dtype=BF16)
    key = (x.device, BF16)
    ops._ARENAS.pop(key, None)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="graph capture"):
        ops.acc_images([(m.acc_downweight.data, m.acc_exponent)], BF16)
    assert key not in ops._ARENAS
    monkeypatch.undo()
    with torch.no_grad():
        assert bool(torch.isfinite(q(x)).all())
    assert ops._ARENAS[key].numel() == 520 * 520 * 2 + (-(520 * 520 * 2)) % 256
    small, _ = _pair(264, 16, BF16, False, seed=42)
    with torch.no_grad():
        small(x[:, :264].contiguous())
    assert ops._ARENAS[key].numel() == 520 * 520 * 2 + (-(520 * 520 * 2)) % 256, "a smaller call reuses the arena"


def test_zz_report_worst_ratios():
    worst = {k: v for k, v in S.WORST.items() if k.startswith("fp8_")}
    for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:10]:
        print(f"{k}: worst err / bound {v:.3f}")
    assert worst and all(v <= 1.0 for v in worst.values())
