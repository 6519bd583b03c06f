"""-m gpu: short batches on E4M3 / MXFP4 accumulators READ IN PLACE (sow_forward_short_codes / sow_backward_short_codes,
skinny_fwd.hip: the row-block forms on codes) through the C ABI, bf16 and f16.

One call = the forward on the codes (y, h_save), the data phase on the codes (dX; dh stays in the workspace) and the UNCHANGED
sow_backward_ex(..., SOW_BWD_WEIGHTS) with kind SOW_ACC_DENSE on the same workspace (dA, dB, dbias).  Buffer protocol, operands
and comparators are those of test_gpu_short_rows.py (imported): NaN neighbours around every input -- NaN codes and NaN scale
bytes around the codes and the scales --, sentinel guards around every output, outputs and workspace filled with 0xFF / 0x00 /
0xFF before three runs that must agree bit for bit.  The reference accumulator is W^, the value the format's record defines
(fp8_acc_ref / fp4_acc_ref), and every output is held to test_gpu_elementwise._check on a dense layer holding W^: no new tolerance.

The data phase keeps the geometry of sow_backward_short and dequantises to the exact bits of W^, so dX and dh are compared BIT FOR
BIT with sow_backward_short on the image sow_acc_dequantize / sow_acc_dequantize_fp4 write, in every case of this file.

Shapes: E4M3 264 -> 520 and 520 -> 264, MXFP4 288 -> 520 and 544 -> 264 (d_in whole MX blocks; a half-filled last 64-column range
and a partial k-step in each direction); T = 65 / 100 / 129 and one T = 1024 case per format."""
import functools
import random

import pytest
import torch

import fp4_acc_ref as R4
import fp8_acc_ref as R8
import fuzz_plan as FP
import test_gpu_elementwise as E
import test_gpu_short_rows as P
import test_gpu_skinny_rows as RW
import value_plan as VP
from numerics import rne, to64
from sow_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
DT = {"bf16": BF16, "f16": F16}
KIND = {"fp8": _lib.ACC_DENSE_FP8, "fp4": _lib.ACC_DENSE_FP4}
SHAPES = {"fp8": [(264, 520), (520, 264)], "fp4": [(288, 520), (544, 264)]}
TS = [65, 100, 129]
RS = [2, 50, 64]


def _cases():
    """A seeded draw: the 24 (format, dtype, r, bias) tuples in shuffled order, the 6 (T, shape index) pairs dealt round over them
    (every pair four times), the scale drawn; then one T = 1024 case per format."""
    rng = random.Random(20261022)
    tuples = [(f, dt, r, b) for f in ("fp8", "fp4") for dt in ("bf16", "f16") for r in RS for b in (True, False)]
    rng.shuffle(tuples)
    pairs = [(T, si) for T in TS for si in range(2)]
    rng.shuffle(pairs)
    out = []
    for i, (f, dt, r, b) in enumerate(tuples):
        T, si = pairs[i % len(pairs)]
        out.append((f, dt, T, *SHAPES[f][si], r, b, rng.choice((1.0, 0.25))))
    return out + [("fp8", "bf16", 1024, 264, 520, 50, True, 0.5), ("fp4", "f16", 1024, 544, 264, 2, False, 1.0)]


CASES = _cases()
assert {(c[0], c[2], c[3], c[4]) for c in CASES if c[2] != 1024} == {(f, T, *s) for f in SHAPES for T in TS for s in SHAPES[f]}
assert {(c[0], c[1], c[5], c[6]) for c in CASES if c[2] != 1024} == {(f, dt, r, b) for f in SHAPES for dt in DT for r in RS for b in (True, False)}


def _id(c):
    return "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def _operands(fmt, dt, T, d_in, d_out, r, bias, s, seed=0):
    """(Case, operands) of one Gaussian layer of test_gpu_short_rows (clear of the ties of h and dh, which W does not enter), its W
    quantised on the CPU: W = W^ (what the references see), q / e = what the kernels read.  Built once per case and shared."""
    c, d = P._operands(dt, T, d_in, d_out, r, bias, s, seed)
    q, e, what = RW._quantise(fmt, d["W"])
    return c, dict(d, W=what, q=q, e=e, fmt=fmt)


def _dh(ws, c):
    """dh as the data phase left it: [T][64] at the front of the 256-aligned workspace (the plan's off_dh = 0)."""
    off = -ws.data_ptr() % 256
    return ws[off:off + c.T * 64 * 2].view(c.dtype).view(c.T, 64).clone()


def _run(layers, runs=(0xFF, 0x00, 0xFF), what="codes", share_w=False, stages=("fwd", "bwd", "weights"), image=False):
    """test_gpu_short_rows._run on codes: one sow_forward_short_codes + sow_backward_short_codes call over `layers` ((Case, operands)
    pairs of one dtype and one format), then the weight phases layer by layer with kind SOW_ACC_DENSE and the codes' address;
    repeated on re-poisoned memory.  image: the SAME protocol through sow_forward_short / sow_backward_short on the image the
    library's dequantiser writes from the same codes.  Returns the outputs of the first run (CPU), one dict per layer, dh included."""
    lib = _lib.load()
    dtype = layers[0][0].dtype
    dt = E._dt(dtype)
    fmt = layers[0][1]["fmt"]
    kind = _lib.ACC_DENSE if image else KIND[fmt]
    query = lib.sow_short_workspace_bytes if image else lib.sow_short_codes_workspace_bytes
    fwd, bwd = (lib.sow_forward_short, lib.sow_backward_short) if image else (lib.sow_forward_short_codes, lib.sow_backward_short_codes)
    ar = E.Arena(dtype)
    n = len(layers)
    arr = (_lib.LayerArgs * n)()
    bufs, W0 = [], None
    for i, (c, d) in enumerate(layers):
        x, A, B, bias, dy = (ar.input(d[k]) for k in ("x", "A", "B", "bias", "dy"))
        if share_w and W0 is not None:
            W, sc = W0
        else:
            W, sc = (RW.F8._guarded_bytes(d[k].to(DEV), g) for k, g in zip(("q", "e"), RW.GUARD_BYTES[fmt]))
            if image:
                cd = W.view(torch.float8_e4m3fn) if fmt == "fp8" else W
                img = ops.acc_dequantize(cd, sc, dtype)
                assert torch.equal(E._bits(img.cpu()), E._bits(d["W"])), "the image is not W^"
                W, sc = ar.input(img), None
        W0 = W0 if W0 is not None else (W, sc)
        rows = c.T or d["rows"]              # (a T = 0 layer: test_gpu_short_rows._run)
        o = dict(y=ar.output((rows, c.d_out)), h=ar.output((rows, 64)), dx=ar.output((rows, c.d_in)), dA=ar.output((c.d_in, c.r)),
                 dB=ar.output((c.r, c.d_out)), dbias=ar.output((c.d_out,)) if c.bias else None)
        nws = query(rows, c.d_in, c.d_out, c.r, kind, dt)
        assert nws >= lib.sow_workspace_bytes(rows, c.d_in, c.d_out, c.r, 0, _lib.ACC_DENSE, dt) > 0
        ws = ar.workspace(nws + 256 * i)
        a = arr[i]
        a.x, a.A, a.B, a.acc_down, a.acc_up, a.bias, a.y, a.h_save, a.dy, a.dx = (E._ptr(t) for t in (x, A, B, W, sc, bias, o["y"], o["h"], dy, o["dx"]))
        a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = c.T, c.d_in, c.d_out, c.r, kind, c.s
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        bufs.append((x, A, B, bias, dy, W, sc, ws, o))
    outs = []
    for byte in runs:
        ar.fill(byte)
        if "fwd" in stages:
            _lib.check(fwd(arr, n, dt, E._stream()), "forward")
        dhs = [None] * n
        if "bwd" in stages:
            _lib.check(bwd(arr, n, dt, E._stream()), "data phase")
            dhs = [_dh(b[7], c) for (c, _), b in zip(layers, bufs)]
        if "weights" in stages:
            for (c, _), (x, A, B, bias, dy, W, sc, ws, o) in zip(layers, bufs):
                if c.T == 0:
                    continue
                _lib.check(lib.sow_backward_ex(E._ptr(dy), E._ptr(x), E._ptr(o["h"]), E._ptr(A), E._ptr(B), E._ptr(W), None, E._ptr(o["dx"]),
                                               E._ptr(o["dA"]), E._ptr(o["dB"]), E._ptr(o["dbias"]), c.T, c.d_in, c.d_out, c.r, 0,
                                               _lib.ACC_DENSE, c.s, 0.0, dt, ws.data_ptr(), ws.numel(), _lib.BWD_WEIGHTS, E._stream()),
                           "sow_backward_ex")
        ar.check_guards(f"{what} run {len(outs)}")
        for (c, _), b in zip(layers, bufs):
            if c.T == 0:
                P._untouched(byte, b[8], b[7], f"{what} run {len(outs)}")
        outs.append([dict({k: (None if v is None else v.clone()) for k, v in b[8].items()}, dh=dh) for b, dh in zip(bufs, dhs)])
    keys = [k for k, st in (("y", "fwd"), ("h", "fwd"), ("dx", "bwd"), ("dh", "bwd"), ("dA", "weights"), ("dB", "weights"), ("dbias", "weights"))
            if st in stages]
    for k in range(1, len(outs)):
        for i in range(n):
            for key in keys:
                if outs[0][i][key] is not None and layers[i][0].T:
                    assert torch.equal(E._bits(outs[0][i][key]), E._bits(outs[k][i][key])), f"{what}: {key} of layer {i} differs between run 0 and run {k}"
    return [{k: (None if v is None or k not in keys else v.cpu()) for k, v in o.items()} for o in outs[0]]


def _check(case, d, out):
    E._check(case, {k: v for k, v in d.items() if k not in ("q", "e", "fmt")}, {k: v for k, v in out.items() if k != "dh"})


def _identical_to_the_image(layers, outs, what):
    """dX and dh against sow_backward_short on the image, bit for bit."""
    ref = _run(layers, runs=(0xFF,), stages=("bwd",), image=True, what=what + " (image)")
    for i, (o, g) in enumerate(zip(outs, ref)):
        P._same(o["dx"], g["dx"], f"{what}: dX of layer {i} against sow_backward_short on the image")
        P._same(o["dh"], g["dh"], f"{what}: dh of layer {i} against sow_backward_short on the image")


# ---- element-wise against float64, and the bit identity with the plain pair on the image ------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_elementwise_against_fp64_and_identical_to_the_image(c):
    case, d = _operands(*c)
    (out,) = _run([(case, d)], what=_id(c))
    _check(case, d, out)
    _identical_to_the_image([(case, d)], [out], _id(c))


# ---- slab regimes -------------------------------------------------------------------------------------------------------------
# (T, d_in, d_out, forward slabs, data-phase slabs).  2208 -> 72: one 128-column range x two blocks ask for 128 slabs' worth of
# workgroups: the forward on codes takes its shortest slabs, 128 rows (18, the last one of 32 rows: one MX block).  96 -> 4360: the
# data phase keeps the plain plan, shortest slab 256: 18 slabs, the last one of 8 columns.
REGIMES = [(65, 2208, 72, 18, 1), (65, 96, 4360, 1, 18)]


@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
@pytest.mark.parametrize("T,d_in,d_out,sf,sb", REGIMES, ids=lambda v: str(v))
def test_slab_regimes(T, d_in, d_out, sf, sb, fmt):
    lib = _lib.load()
    part = lambda S, N: P._al256(S * T * N * 4) + P._al256(S * T * 64 * 4)    # noqa: E731
    assert lib.sow_forward_short_codes_workspace_bytes(T, d_in, d_out, 8, KIND[fmt], _lib.BF16) == 256 + part(sf, d_out)
    base = lib.sow_workspace_bytes(T, d_in, d_out, 8, 0, _lib.ACC_DENSE, _lib.BF16)
    assert lib.sow_short_codes_workspace_bytes(T, d_in, d_out, 8, KIND[fmt], _lib.BF16) == base + max(part(sf, d_out), part(sb, d_in))
    case, d = _operands(fmt, "bf16", T, d_in, d_out, 8, True, 0.5, 40)
    (out,) = _run([(case, d)], runs=(0xFF, 0x00), what=f"regime {fmt} {T} {d_in} {d_out}")
    _check(case, d, out)
    _identical_to_the_image([(case, d)], [out], f"regime {fmt} {d_in} {d_out}")


# ---- exact operands -------------------------------------------------------------------------------------------------------------
def _fp8_codes(v):
    """The E4M3 code bytes of float64 values that ARE code values."""
    mag = torch.searchsorted(R8.POS, v.abs())
    assert bool((R8.POS[mag.clamp(max=126)] == v.abs()).all()), "not a code value"
    return (mag + 128 * (v < 0)).to(torch.uint8)


def _fp4_codes(v):
    """The packed E2M1 bytes (row k in the low nibble, row k + 1 in the high one) of float64 values that ARE code values."""
    vals = torch.tensor(R4.VALUES_X2, dtype=torch.float64) / 2
    mag = torch.searchsorted(vals, v.abs())
    assert bool((vals[mag.clamp(max=7)] == v.abs()).all()), "not a code value"
    q = mag + 8 * (v < 0)
    return (q[0::2] + 16 * q[1::2]).to(torch.uint8)


def _as_codes(fmt, W, exps):
    """(codes, scales) with code * 2^scale = W exactly: exps int64, [d_out] (E4M3) or [d_in / 32, d_out] (MXFP4)."""
    if fmt == "fp8":
        return _fp8_codes(W * torch.exp2(-exps.double())[None, :]), exps.to(torch.int8)
    return _fp4_codes(W * torch.exp2(-exps.double()).repeat_interleave(32, dim=0)), (exps + 127).to(torch.uint8)


EXACT = [("fp8", "bf16", 100, 264, 520, 50, True, 0.5), ("fp8", "f16", 129, 520, 264, 2, True, 0.25), ("fp4", "bf16", 65, 544, 264, 64, True, 1.0),
         ("fp4", "f16", 100, 288, 520, 50, False, 0.5)]


@pytest.mark.parametrize("c", EXACT, ids=_id)
def test_exact_operands_bit_for_bit(c):
    """The proved small-integer layer of test_gpu_short_rows (W in {0, +-1, +-2}) with W stored as codes under power-of-two scales
    2^-1, 1, 2 that differ per column (E4M3) or per block and column (MXFP4): code = W / scale in {0, +-1/2, ..., +-4} is a code value
    of either format, so W^ = W and every output equals the float64 result, bit for bit."""
    fmt, dt, T, d_in, d_out, r, bias, s = c
    lc = FP.Layer(name="short_codes_exact_" + _id(c), dtype=dt, T=T, d_in=d_in, d_out=d_out, r=r, acc="dense", bias=bias, s=s, seed=11)
    d, f = VP.exact_layer_proved(lc)
    dtype = DT[dt]
    g = torch.Generator().manual_seed(12)
    exps = torch.randint(-1, 2, (d_out,) if fmt == "fp8" else (d_in // 32, d_out), generator=g)
    assert len(set(exps.flatten().tolist())) == 3
    q, e = _as_codes(fmt, d["W"], exps)
    what = (R8.dequantize(q, e) if fmt == "fp8" else R4.dequantize(q, e, dtype).double())
    assert bool((what == d["W"]).all()), "the codes do not stand for W"
    opsd = {k: (None if v is None else v.to(dtype)) for k, v in d.items()}
    case = E.Case(lc.name, dtype, T, d_in, d_out, r, acc="dense", bias=bias, s=s)
    layer = (case, dict(opsd, q=q, e=e, fmt=fmt))
    (out,) = _run([layer], what="exact " + _id(c))
    for k in ("y", "dx", "dA", "dB") + (("dbias",) if bias else ()):
        bad = to64(out[k]) != rne(f[k], dtype)
        assert not bad.any(), f"{k}: {int(bad.sum())} of {bad.numel()} elements differ from the float64 result; first at {tuple(int(v) for v in torch.nonzero(bad)[0])}"
    h = to64(out["h"])
    assert bool((h[:, :r] == f["h"]).all()), "h_save differs from the float64 projection"
    assert bool((h[:, r:63] == 0).all()) and (r == 64 or bool((h[:, 63] == 1).all())), "h_save: pad columns / the ones column"
    _identical_to_the_image([layer], [out], "exact " + _id(c))


# ---- one-hot dY: rows of W^T ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,dt,d_in,d_out", [("fp8", "bf16", 264, 520), ("fp8", "f16", 520, 264), ("fp4", "bf16", 288, 520), ("fp4", "f16", 544, 264)])
def test_one_hot_dy_reproduces_rows_of_the_image(fmt, dt, d_in, d_out):
    """dY row t = 1.0 at column k_t and B = 0 (dh = 0): dX[t] = W^[:, k_t], one exact product per element.  The k_t cover every position
    mod 32 of a column, both halves of the last (partial) k-step and every wave.  The codes are random bytes -- every code of the
    format, -0 among them, in both nibbles -- with NaN codes replaced, and the scales random over the dtype's whole clamp range with its
    largest and smallest value forced into the first columns: a wrong nibble, parity, scale index or a lost sign changes an element.
    (The sign of a ZERO cannot reach dX: the fp32 sum starts from +0, so -0 codes are held to +0, as on the image.)"""
    dtype, T = DT[dt], 100
    g = torch.Generator().manual_seed(77)
    ks = [(5 + 7 * t) % d_out for t in range(T)]
    assert {k % 32 for k in ks} == set(range(32)) and max(ks) >= d_out - 8 and {(k // 64) % 4 for k in ks} == set(range(4))
    if fmt == "fp8":
        q = torch.randint(0, 256, (d_in, d_out), generator=g).to(torch.uint8)
        q[(q & 0x7F) == 0x7F] = 0x80                               # NaN codes -> -0
        lo, hi = R8.EXP_RANGE[dtype]
        e = torch.randint(lo, hi + 1, (d_out,), generator=g)
        e[ks[0]], e[ks[1]] = lo, hi
        e = e.to(torch.int8)
        what = R8.dequantize(q, e).to(dtype)
    else:
        q = torch.randint(0, 256, (d_in // 2, d_out), generator=g).to(torch.uint8)
        lo, hi = R4.EXP_RANGE[dtype]
        e = torch.randint(lo, hi + 1, (d_in // 32, d_out), generator=g)
        e[:, ks[0]], e[:, ks[1]] = lo, hi
        e = (e + 127).to(torch.uint8)
        what = R4.dequantize(q, e, dtype)
    assert bool(torch.isfinite(what.float()).all()) and bool((E._bits(what) == -32768).any()), "finite, and -0 among the values"
    dy = torch.zeros(T, d_out, dtype=dtype)
    dy[torch.arange(T), torch.tensor(ks)] = 1.0
    d = dict(x=torch.zeros(T, d_in, dtype=dtype), A=torch.randn(d_in, 8, generator=g).to(dtype), B=torch.zeros(8, d_out, dtype=dtype),
             bias=None, dy=dy, W=what, q=q, e=e, fmt=fmt)
    case = E.Case(f"one_hot_{fmt}_{dt}", dtype, T, d_in, d_out, 8, acc="dense", bias=False, s=1.0)
    (out,) = _run([(case, d)], runs=(0xFF,), stages=("bwd",), what="one-hot")
    want = (what.double()[:, ks].t() + 0.0).to(dtype)               # (-0 + 0 = +0)
    P._same(out["dx"], want, f"{fmt} {dt}: dX against the rows of W^T")
    _identical_to_the_image([(case, d)], [out], f"one-hot {fmt} {dt}")


# ---- rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_65_rows_store_65_rows(fmt):
    """T = 65: the second block holds one row; y, h_save and dX have 65 rows and a sentinel guard right behind them."""
    case, d = _operands(fmt, "bf16", 65, *SHAPES[fmt][0], 8, True, 1.0, 7)
    (out,) = _run([(case, d)], what="65 rows")
    assert out["y"].shape == (65, 520) and out["dx"].shape == (65, case.d_in) and out["h"].shape == (65, 64)
    _check(case, d, out)


@pytest.mark.parametrize("fmt,dt", [("fp8", "bf16"), ("fp4", "f16")])
def test_swapped_rows_give_swapped_rows(fmt, dt):
    case, d = _operands(fmt, dt, 100, *SHAPES[fmt][0], 50, True, 0.5, 3)
    perm = list(range(100))
    perm[3], perm[70] = 70, 3
    (a,) = _run([(case, d)], runs=(0xFF,), stages=("fwd", "bwd"), what="rows in place")
    (b,) = _run([(case, dict(d, x=d["x"][perm].contiguous(), dy=d["dy"][perm].contiguous()))], runs=(0xFF,), stages=("fwd", "bwd"), what="rows swapped")
    for k in ("y", "h", "dx", "dh"):
        P._same(b[k], a[k][perm], f"{fmt} {dt} {k} with rows 3 and 70 swapped")


@pytest.mark.parametrize("fmt,dt,k", [("fp8", "bf16", 0), ("fp4", "f16", 263)])
def test_a_nan_in_row_70_reaches_row_70_only(fmt, dt, k):
    case, d = _operands(fmt, dt, 100, *SHAPES[fmt][0], 50, True, 0.5, 3)
    (clean,) = _run([(case, d)], runs=(0xFF,), stages=("fwd", "bwd"), what="clean")
    p = dict(d, x=d["x"].clone(), dy=d["dy"].clone())
    p["x"][70, k] = float("nan")
    p["dy"][70, 519 - k] = float("nan")
    (pois,) = _run([(case, p)], runs=(0xFF,), stages=("fwd", "bwd"), what="poisoned")
    keep = [t for t in range(100) if t != 70]
    assert bool(torch.isnan(pois["y"][70]).all()) and bool(torch.isnan(pois["dx"][70]).all()), "row 70 of y and dX must be NaN in every column"
    assert bool(torch.isnan(pois["h"][70, :50]).all()), "row 70 of h_save must be NaN in every live column"
    for key in ("y", "h", "dx"):
        P._same(pois[key][keep], clean[key][keep], f"{fmt} {dt} {key}: the other rows")


# ---- groups ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_three_layers_equal_three_single_calls(fmt):
    """65 + 129 + 100 rows = 2 + 3 + 2 row blocks in one launch group, each layer with its own plans."""
    (a, b) = SHAPES[fmt]
    layers = [_operands(fmt, "bf16", 65, *a, 2, True, 0.5, 20), _operands(fmt, "bf16", 129, *b, 64, False, 1.0, 21),
              _operands(fmt, "bf16", 100, *a, 50, True, 0.25, 22)]
    grouped = _run(layers, what="group")
    for i, (L, g) in enumerate(zip(layers, grouped)):
        (s,) = _run([L], runs=(0xFF,), what=f"single {i}")
        P._same_outs(g, s, f"layer {i}", keys=("y", "h", "dx", "dh", "dA", "dB", "dbias"))
        _check(L[0], L[1], g)


@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_seventeen_row_blocks_take_two_launch_pairs(fmt):
    """1024 + 65 rows = 18 entries: the second layer's blocks are split over two launch pairs."""
    (a, b) = SHAPES[fmt]
    layers = [_operands(fmt, "bf16", 1024, *a, 8, True, 0.5, 23), _operands(fmt, "bf16", 65, *b, 2, True, 1.0, 24)]
    grouped = _run(layers, runs=(0xFF, 0x00), what="two pairs")
    for i, (L, g) in enumerate(zip(layers, grouped)):
        (s,) = _run([L], runs=(0xFF,), what=f"single {i}")
        P._same_outs(g, s, f"layer {i}", keys=("y", "h", "dx", "dh", "dA", "dB", "dbias"))


@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_two_layers_over_one_code_matrix(fmt):
    """Two layers read ONE pair of code and scale buffers in one call (different x, factors and workspaces)."""
    a = _operands(fmt, "bf16", 100, *SHAPES[fmt][0], 50, True, 0.5, 30)
    c2, d2 = P._operands("bf16", 129, *SHAPES[fmt][0], 2, False, 1.0, 31)
    second = (c2, dict(d2, W=a[1]["W"], q=a[1]["q"], e=a[1]["e"], fmt=fmt))
    grouped = _run([a, second], share_w=True, what="one code matrix")
    for i, (L, g) in enumerate(zip([a, second], grouped)):
        (s,) = _run([L], runs=(0xFF,), what=f"single {i}")
        P._same_outs(g, s, f"layer {i} on the shared codes", keys=("y", "h", "dx", "dh", "dA", "dB", "dbias"))
        _check(L[0], L[1], g)


def test_zz_report_worst_ratios():
    names = {_operands(*c)[0].name for c in CASES}
    worst = {k: v for k, v in E.WORST.items() if k[0] in names}
    for k, v in sorted(worst.items(), key=lambda kv: -kv[1][0])[:10]:
        print(f"{k}: worst err / bound {v[0]:.3f}")
    assert worst and all(v[0] <= 1.0 for v in worst.values())
