"""-m gpu: the generation-sized forward for up to 64 rows (sow_forward_skinny_rows, skinny_fwd.hip: the four-row-tile forms of
phase A) through the C ABI, element by element against float64, for all four accumulator kinds and both half dtypes.

The buffer protocol and the comparator are those of test_gpu_skinny.py (its helpers are imported): NaN neighbours around every
input, guards around every output, y and the workspace filled with 0xFF / 0x00 / 0xFF bytes before three runs that must agree
bit for bit; every element of y is held to numerics.bound on W^ (the accumulator as the kernel reads it: the codes through
fp8_acc_ref.py / fp4_acc_ref.py), no other tolerance.  Gaussian operands are moved clear of the rounding ties of h first
(skinny_sweep.off_ties, decided on the CPU from the operands alone: DESIGN 4.5b).

T = 33 / 48 / 49 / 64: one row in the third 16-row tile, a full third tile, one row in the fourth, all four full.  Shapes as
in test_gpu_skinny.py ((264, 520), (520, 264), (1032, 72): partial last K-slab and column range); MXFP4 needs whole 32-row
blocks: (288, 520), (544, 264), (160, 136)."""
import random

import pytest
import torch

import fp4_acc_ref as R4
import skinny_sweep as SW
import test_gpu_elementwise as E
import test_gpu_fp4_acc as F4
import test_gpu_fp8_acc as F8
import test_gpu_skinny as S
from numerics import rne, to64
from sow_amd import _lib, acc_quant

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT = S.DT
KIND = {"none": _lib.ACC_NONE, "dense": _lib.ACC_DENSE, "fp8": _lib.ACC_DENSE_FP8, "fp4": _lib.ACC_DENSE_FP4}
GUARD_BYTES = {"fp8": (0x7F, 127), "fp4": (0x77, 254)}     # around the codes / the scales: a read past either shows in y
SHAPES = [(264, 520), (520, 264), (1032, 72)]
SHAPES_FP4 = [(288, 520), (544, 264), (160, 136)]
TS = [33, 48, 49, 64]
RS = [2, 8, 50, 64]
WORST = {}


def _cases():
    """A seeded draw: the 32 (format, dtype, r) triples in shuffled order, the 12 (T, shape) pairs dealt round over them (every
    pair at least twice), bias and scale drawn."""
    rng = random.Random(20261020)
    triples = [(f, dt, r) for f in ("none", "dense", "fp8", "fp4") for dt in ("bf16", "f16") for r in RS]
    rng.shuffle(triples)
    pairs = [(T, si) for T in TS for si in range(3)]
    rng.shuffle(pairs)
    out = []
    for i, (f, dt, r) in enumerate(triples):
        T, si = pairs[i % len(pairs)]
        d_in, d_out = (SHAPES_FP4 if f == "fp4" else SHAPES)[si]
        out.append((dt, T, d_in, d_out, r, rng.random() < 0.5, rng.choice((1.0, 0.25)), f))
    return out


CASES = _cases()
assert {(c[1], SHAPES.index((c[2], c[3])) if c[7] != "fp4" else SHAPES_FP4.index((c[2], c[3]))) for c in CASES} == \
       {(T, si) for T in TS for si in range(3)}


def _quantise(fmt, W):
    """(codes, scales, W^) on the CPU.  Small matrices through the integer references; large ones through the package's
    quantiser on the GPU, which the quantiser tests of either format tie to its reference bit for bit."""
    if fmt == "fp8":
        return F8._quant(W)
    if W.numel() <= 1 << 20:
        return F4._quant(W)
    q, e = acc_quant.quantize_tensor(W.to(DEV), "mxfp4")
    codes, scales = q.cpu(), e.cpu()
    return codes, scales, R4.dequantize(codes, scales, W.dtype)


def _layer(fmt, dtype, T, d_in, d_out, r, bias, s, seed=0, ties=True):
    """Gaussian operands of one layer (test_gpu_skinny._gauss) in format `fmt`: W = what the reference sees (W^ for codes),
    q / e = what the kernel reads.  ties: moved clear of the rounding ties of h."""
    d = dict(S._gauss(dtype, T, d_in, d_out, r, bias, "none" if fmt == "none" else "dense", seed=seed), s=s)
    if fmt in ("fp8", "fp4"):
        q, e, what = _quantise(fmt, d["W"])
        d.update(W=what, q=q, e=e)
    if ties:
        d, moved = SW.off_ties(dtype, d)      # (each element at most once, by one ulp; kernel and reference read the same A)
        print(f"{fmt} {T} x {d_in} -> {d_out}, r = {r}: {moved} of {d['A'].numel()} elements of A moved by one ulp")
    return dict(d, fmt=fmt)


def _old_query(lib, T, d_in, d_out, r, fmt, code):
    if fmt == "fp8":
        return lib.sow_forward_skinny_fp8_workspace_bytes(T, d_in, d_out, r, code)
    if fmt == "fp4":
        return lib.sow_forward_skinny_fp4_workspace_bytes(T, d_in, d_out, r, code)
    return lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, KIND[fmt], code)


def _run(dtype, layers, entry="rows", x_shared=False, runs=(0xFF, 0x00, 0xFF), flagged=False, what="rows"):
    """One call of sow_forward_skinny_rows (entry="skinny": of sow_forward_skinny) over `layers`, repeated on poisoned, zeroed
    and poisoned memory: the runs must agree bit for bit and leave every guard intact.  Returns the y of the first run (CPU).
    flagged: A, B and bias are passed as fp32 with SOW_PARAM_F32 | SOW_ACC_NATIVE.  A layer's "y_rows" allocates that many rows
    of y (rows >= T must keep the bytes every run fills them with; the returned y holds the T rows)."""
    lib = _lib.load()
    ar, arp = E.Arena(dtype), E.Arena(F32 if flagged else dtype)
    code = E._dt(dtype) | ((_lib.PARAM_F32 | _lib.ACC_NATIVE) if flagged else 0)
    arr = (_lib.LayerArgs * len(layers))()
    ys, keep = [], []
    x0 = None
    for i, d in enumerate(layers):
        fmt = d["fmt"]
        x = x0 if (x_shared and x0 is not None) else ar.input(d["x"])
        x0 = x0 if x0 is not None else x
        A, B, bias = (arp.input(d.get(k)) for k in ("A", "B", "bias"))
        W = e = None
        if fmt == "dense":
            W = ar.input(d["W"])
        elif fmt in GUARD_BYTES:
            W, e = F8._guarded_bytes(d["q"], GUARD_BYTES[fmt][0]), F8._guarded_bytes(d["e"], GUARD_BYTES[fmt][1])
        T, d_in = d["x"].shape
        r, d_out = d["B"].shape
        y = ar.output((d.get("y_rows", T), d_out))
        nws = (lib.sow_forward_skinny_rows_workspace_bytes(T, d_in, d_out, r, KIND[fmt], code) if entry == "rows"
               else _old_query(lib, T, d_in, d_out, r, fmt, code))
        assert nws > 0, (T, d_in, d_out, r, fmt)
        ws = ar.workspace(nws)
        a = arr[i]
        a.x, a.A, a.B, a.acc_down, a.acc_up, a.bias, a.y = (E._ptr(t) for t in (x, A, B, W, e, bias, y))
        a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, KIND[fmt], d["s"]
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        ys.append(y)
        keep.append((x, A, B, bias, W, e, ws))
    fn = lib.sow_forward_skinny_rows if entry == "rows" else lib.sow_forward_skinny
    outs = []
    for byte in runs:
        ar.fill(byte)
        _lib.check(fn(arr, len(layers), code, E._stream()), "sow_forward_" + ("skinny_rows" if entry == "rows" else "skinny"))
        ar.check_guards(f"{what} run {len(outs)}")
        for y, d in zip(ys, layers):      # rows past T of a larger y buffer keep the bytes they were filled with
            fill = -1 if byte == 0xFF else 0
            assert bool((E._bits(y[d["x"].shape[0]:]) == fill).all()), f"{what} run {len(outs)}: rows past T were stored"
        outs.append([y[:d["x"].shape[0]].clone() for y, d in zip(ys, layers)])
    for k in range(1, len(outs)):
        for i, (a, b) in enumerate(zip(outs[0], outs[k])):
            assert torch.equal(E._bits(a), E._bits(b)), f"{what}: y of layer {i} differs between run 0 and run {k}"
    return [y.cpu() for y in outs[0]]


def _check(name, dtype, d, y):
    """test_gpu_skinny's comparator on W^ (d["W"]): no other tolerance."""
    st = S._check("rows_" + name, dtype, {k: v for k, v in d.items() if k not in ("q", "e", "fmt", "y_rows")}, y)
    WORST[name] = st["worst"]
    return st


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(E._bits(a), E._bits(b)), f"{what}: {int((E._bits(a) != E._bits(b)).sum())} elements differ"


# ---- element-wise against float64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=S._id)
def test_elementwise_against_fp64(c):
    dt, T, d_in, d_out, r, bias, s, fmt = c
    dtype = DT[dt]
    d = _layer(fmt, dtype, T, d_in, d_out, r, bias, s)
    (y,) = _run(dtype, [d], what=S._id(c))
    _check(S._id(c), dtype, d, y)


@pytest.mark.parametrize("fmt", ["none", "dense", "fp8", "fp4"])
@pytest.mark.parametrize("dt,T", [("bf16", 49), ("f16", 64)])
def test_fp32_factors_equal_pre_rounded(dt, T, fmt):
    """cd | SOW_PARAM_F32 | SOW_ACC_NATIVE on fp32 A, B and bias: bit for bit the unflagged call on the factors rounded once."""
    dtype = DT[dt]
    d_in, d_out = (544, 264) if fmt == "fp4" else (520, 264)
    d = _layer(fmt, dtype, T, d_in, d_out, 50, True, 0.5, seed=60, ties=False)
    g = torch.Generator().manual_seed(61)
    f32 = dict(A=torch.randn(d_in, 50, generator=g) * 0.05, B=torch.randn(50, d_out, generator=g) * 0.05, bias=torch.randn(d_out, generator=g) * 0.1)
    assert all(bool((v.to(dtype).float() != v).any()) for v in f32.values()), "the fp32 factors must need rounding"
    (got,) = _run(dtype, [dict(d, **f32)], flagged=True, what=f"flagged {fmt}")
    rounded = dict(d, **{k: v.to(dtype) for k, v in f32.items()})
    (want,) = _run(dtype, [rounded], runs=(0xFF,), what=f"pre-rounded {fmt}")
    _same(got, want, f"{dt} T={T} {fmt}: fp32 factors against pre-rounded")
    assert bool(torch.isfinite(got.float()).all()) and float(got.float().abs().max()) > 0


# ---- slab regimes of the plan for T > 32 ------------------------------------------------------------------------------------
def _al256(n):
    return (n + 255) // 256 * 256


def _ws(S_, T, d_out, dense=True):
    """The workspace of S_ slabs, as the query reports it: 256 + the partials of y + the partials of x . A."""
    return 256 + (_al256(S_ * T * d_out * 4) if dense else 0) + _al256(S_ * T * 64 * 4)


# (fmt, T, d_in, d_out, slabs): 129 (65 for codes) column ranges ask for four slabs' worth of workgroups, and the slab is capped:
#   T = 48: 768 rows.  2568 = 3 x 768 + 264 (2592 = 3 x 768 + 288): six k-steps per wave -- the request-ahead ring of four
#           refilled and drained -- and a last slab that ends in a partial round (264 = 2 rounds + 8 rows; 288 = 2 rounds + 32)
#   T = 64: 512 rows, the longest slab of a 64-row x slab (four k-steps per wave: the ring is never refilled at T > 48).
#           1544 = 3 x 512 + 8, 1568 = 3 x 512 + 32
#   T = 49: 2208 -> 136 has one to three column ranges, so the plan takes the shortest slabs, 128 rows: 18 of them, two past the
#           16 that phase B requests up front (its second loop), the last one of 32 rows (three of four waves idle)
REGIMES = [("dense", 48, 2568, 8200, 4), ("fp8", 48, 2568, 8200, 4), ("fp4", 48, 2592, 8200, 4),
           ("dense", 64, 1544, 8200, 4), ("fp8", 64, 1544, 8200, 4), ("fp4", 64, 1568, 8200, 4),
           ("dense", 49, 2208, 136, 18), ("fp8", 49, 2208, 136, 18), ("fp4", 49, 2208, 136, 18), ("none", 49, 2208, 136, 18)]


@pytest.mark.parametrize("fmt,T,d_in,d_out,slabs", REGIMES, ids=lambda v: str(v))
def test_slab_regimes(fmt, T, d_in, d_out, slabs):
    lib = _lib.load()
    got = lib.sow_forward_skinny_rows_workspace_bytes(T, d_in, d_out, 8, KIND[fmt], _lib.BF16)
    assert got == _ws(slabs, T, d_out, fmt != "none"), (got, _ws(slabs, T, d_out, fmt != "none"))
    d = _layer(fmt, BF16, T, d_in, d_out, 8, d_out < 1000, 0.5, seed=40 + T)
    (y,) = _run(BF16, [d], runs=(0xFF, 0x00), what=f"regime {fmt} {T}")
    _check(f"regime_{fmt}_{T}_{d_in}", BF16, d, y)


# ---- exact operands -------------------------------------------------------------------------------------------------------
EXACT = [("bf16", 49, 264, 520, 50, True, 0.5, "dense"), ("f16", 64, 520, 264, 8, True, 0.25, "dense"),
         ("bf16", 64, 1032, 72, 64, False, 1.0, "none"), ("f16", 49, 264, 520, 2, True, 0.5, "none")]
EXACT_FP4 = [("bf16", 49, 288, 520, 50, True, 0.5, "dense"), ("f16", 64, 544, 264, 8, True, 0.25, "dense")]


def _exact(fmt, c):
    if fmt == "fp8":
        d, y64, _ = F8._exact_fp8(c)
    elif fmt == "fp4":
        d, y64 = F4._exact_fp4(c)
    else:
        d, y64 = S._exact_operands(c)
    return dict(d, fmt=fmt), y64


@pytest.mark.parametrize("fmt,c", [(c[7], c) for c in EXACT] + [("fp8", c) for c in EXACT[:2]] + [("fp4", c) for c in EXACT_FP4],
                         ids=lambda v: v if isinstance(v, str) else S._id(v))
def test_exact_operands_bit_for_bit(fmt, c):
    dtype = DT[c[0]]
    d, y64 = _exact(fmt, c)
    (y,) = _run(dtype, [d], what=f"exact {fmt} " + S._id(c))
    bad = to64(y) != rne(y64, dtype)
    assert not bad.any(), (f"{int(bad.sum())} of {bad.numel()} elements differ from the float64 result rounded once; first at "
                           f"{tuple(int(v) for v in torch.nonzero(bad)[0])}")


# ---- rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,dt,k", [("dense", "bf16", 0), ("fp8", "bf16", 263), ("fp4", "f16", 130), ("none", "f16", 287)])
def test_a_nan_in_row_40_reaches_row_40_only(fmt, dt, k):
    dtype = DT[dt]
    d = _layer(fmt, dtype, 64, 288, 520, 50, True, 0.5, seed=3)
    (clean,) = _run(dtype, [d], runs=(0xFF,), what="rows clean")
    p = dict(d, x=d["x"].clone())
    p["x"][40, k] = float("nan")
    (poisoned,) = _run(dtype, [p], runs=(0xFF,), what="rows poisoned")
    assert bool(torch.isnan(poisoned[40]).all()), "row 40 must be NaN in every column"
    keep = [t for t in range(64) if t != 40]
    _same(poisoned[keep], clean[keep], "the other rows")
    _check(f"rows_{fmt}_{dt}", dtype, d, clean)


@pytest.mark.parametrize("fmt", ["dense", "fp8", "fp4"])
def test_33_rows_store_33_rows(fmt):
    """T = 33 into a y buffer of 48 rows: row 32 is right, rows 33 .. 47 (the rest of the third tile, zeros in the x slab) keep
    the 0xFF / 0x00 / 0xFF bytes they are filled with before each of the three runs (_run asserts it)."""
    d = _layer(fmt, BF16, 33, 288, 520, 8, True, 1.0, seed=7)
    (y,) = _run(BF16, [dict(d, y_rows=48)], what=f"33 rows {fmt}")
    assert y.shape == (33, 520)
    _check(f"rows33_{fmt}", BF16, d, y)


# ---- groups, mixed T, T <= 32 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["dense", "fp8", "fp4"])
def test_groups_equal_single_calls(fmt):
    """Three siblings on ONE x buffer, the middle one without an accumulator: each y is the y of the layer's call alone."""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(49, 512, generator=g).to(BF16)
    sibs = []
    for i, d_out in enumerate((512, 256, 264)):
        d = _layer("none" if i == 1 else fmt, BF16, 49, 512, d_out, (50, 8, 64)[i], i != 2, 0.5, seed=20 + i, ties=False)
        sibs.append(dict(d, x=x))
    sibs = [dict(SW.off_ties(BF16, d)[0]) for d in sibs]
    grouped = _run(BF16, sibs, x_shared=True, what=f"group {fmt}")
    for i, (d, yg) in enumerate(zip(sibs, grouped)):
        (ys,) = _run(BF16, [d], runs=(0xFF,), what=f"single {i}")
        _same(yg, ys, f"{fmt} sibling {i}")
        _check(f"group_{fmt}_{i}", BF16, d, yg)


@pytest.mark.parametrize("fmt", ["dense", "fp8", "fp4"])
def test_mixed_row_counts_in_one_call(fmt):
    """T = 17 and T = 64 in one call: each equals its call alone, and the 17-row layer equals sow_forward_skinny."""
    pair = [_layer(fmt, F16, 17, 288, 520, 8, True, 0.25, seed=30), _layer(fmt, F16, 64, 544, 264, 64, False, 1.0, seed=31)]
    for order in (pair, pair[::-1]):
        grouped = _run(F16, order, runs=(0xFF, 0x00), what=f"mixed {fmt}")
        for d, yg in zip(order, grouped):
            T = d["x"].shape[0]
            (ys,) = _run(F16, [d], runs=(0xFF,), what=f"mixed single {T}")
            _same(yg, ys, f"{fmt} T={T} in a mixed call")
            if T == 17:
                (yo,) = _run(F16, [d], entry="skinny", runs=(0xFF,), what="mixed old entry")
                _same(yg, yo, f"{fmt} T=17 against sow_forward_skinny")
    _check(f"mixed_{fmt}", F16, pair[1], grouped[0])


@pytest.mark.parametrize("T", [1, 16, 17, 32])
def test_up_to_32_rows_the_new_entry_is_the_old_one(T):
    lib = _lib.load()
    for fmt, dt in (("none", "f16"), ("dense", "bf16"), ("fp8", "f16"), ("fp4", "bf16")):
        dtype = DT[dt]
        d_in, d_out = (544, 264) if fmt == "fp4" else (520, 264)
        assert (lib.sow_forward_skinny_rows_workspace_bytes(T, d_in, d_out, 50, KIND[fmt], E._dt(dtype))
                == _old_query(lib, T, d_in, d_out, 50, fmt, E._dt(dtype)))
        d = _layer(fmt, dtype, T, d_in, d_out, 50, True, 0.5, seed=50, ties=False)
        (new,) = _run(dtype, [d], runs=(0xFF, 0x00), what=f"new entry T={T} {fmt}")
        (old,) = _run(dtype, [d], entry="skinny", runs=(0xFF,), what=f"old entry T={T} {fmt}")
        _same(new, old, f"T={T} {fmt}")


def test_zz_report_worst_ratios():
    for k, v in sorted(WORST.items(), key=lambda kv: -kv[1])[:10]:
        print(f"{k}: worst err / bound {v:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
