"""-m gpu: short batches of dense-accumulator layers on the skinny kernel pair (sow_forward_short / sow_backward_short,
skinny_fwd.hip: the row-block forms) through the C ABI, element by element against float64, bf16 and f16.

One call = the new forward (writes y and h_save), the new data phase (writes dX, leaves dh in the workspace) and the UNCHANGED
sow_backward_ex(..., SOW_BWD_WEIGHTS) on the same workspace (dA, dB, dbias from that dh).  The buffer protocol is that of
test_gpu_elementwise.py / test_gpu_skinny_rows.py (imported): NaN neighbours around every input, sentinel guards around every
output, outputs and the workspace filled with 0xFF / 0x00 / 0xFF bytes before three runs that must agree bit for bit -- a
poisoned workspace changes nothing, and an output of T rows with a guard behind it shows a row stored past T.  Every output is
held to the comparators of test_gpu_elementwise._check on a dense-accumulator layer that rounds y and dX once: no new tolerance.

Gaussian operands are moved clear of rounding ties first (skinny_sweep.off_ties): elements of A by one ulp for h,
then -- with the roles swapped, dY for x and B^T for A -- elements of B for dh.  That is decided on the CPU from the operands
alone; _operands asserts that a second pass over the finished operands moves nothing before anything runs on the GPU.

T = 65 / 100 / 129 / 1024: 64 + 1 rows, 64 + 36 rows (a 48-row last block), three blocks, sixteen blocks (the entry limit);
(264, 520) and (520, 264): a ragged last k-step and a partial last column range in both directions."""
import functools
import random

import pytest
import torch

import fuzz_plan as FP
import skinny_sweep as SW
import test_gpu_elementwise as E
import value_plan as VP
from numerics import rne, to64
from sow_amd import _lib

pytestmark = pytest.mark.gpu
BF16, F16 = torch.bfloat16, torch.float16
DT = {"bf16": BF16, "f16": F16}
TS = [65, 100, 129, 1024]
SHAPES = [(264, 520), (520, 264)]
RS = [2, 8, 50, 63, 64]
# Ties are cleared up to this many rows.  A move of one element of A shifts its column of h in EVERY row, and at 1024 rows some row
# of the column is within the fp32 noise of a midpoint after every move (f16: the step never ends; it raises "column 0 of h stays
# on a rounding tie").  Nothing is lost: the comparators used here take h from the h_save the kernel wrote -- a flip of its
# rounding is judged by check_h_save's fp32-floor term, not propagated into the reference of y -- and the bound of dX carries the
# u |dh| term of the hidden rounding of dh.
TIES_MAX_T = 129


def _cases():
    """A seeded draw: the 20 (dtype, r, bias) triples in shuffled order, the 8 (T, shape) pairs dealt round over them (every
    pair at least twice), the scale drawn."""
    rng = random.Random(20261021)
    triples = [(dt, r, b) for dt in ("bf16", "f16") for r in RS for b in (True, False)]
    rng.shuffle(triples)
    pairs = [(T, s) for T in TS for s in SHAPES]
    rng.shuffle(pairs)
    return [(dt, pairs[i % len(pairs)][0], *pairs[i % len(pairs)][1], r, b, rng.choice((1.0, 0.25))) for i, (dt, r, b) in enumerate(triples)]


CASES = _cases()
assert {(c[1], c[2], c[3]) for c in CASES} == {(T, *s) for T in TS for s in SHAPES}
assert {(c[0], c[4], c[5]) for c in CASES} == {(dt, r, b) for dt in DT for r in RS for b in (True, False)}


def _id(c):
    return "-".join(str(v) for v in c)


def _off_ties(dtype, d, s):
    """(operands, elements moved): A moved clear of the ties of h = s x A, then B clear of the ties of dh = s dY B^T."""
    f, m1 = SW.off_ties(dtype, dict(x=d["x"], A=d["A"], B=d["B"], bias=d.get("bias"), W=d["W"], s=s))
    d = dict(d, A=f["A"])
    g, m2 = SW.off_ties(dtype, dict(x=d["dy"], A=d["B"].t().contiguous(), B=d["A"].t().contiguous(), bias=None,
                                    W=d["W"].t().contiguous(), s=s))
    return dict(d, B=g["A"].t().contiguous()), m1 + m2


@functools.lru_cache(maxsize=None)
def _operands(dt, T, d_in, d_out, r, bias, s, seed=0):
    """(Case, operands) of one Gaussian layer (test_gpu_elementwise._inputs), clear of ties; built once per case and shared."""
    c = E.Case(_id((dt, T, d_in, d_out, r, bias, s, seed)), DT[dt], T, d_in, d_out, r, acc="dense", bias=bias, s=s, seed=seed)
    d = E._inputs(c)
    if T > TIES_MAX_T:
        return c, d
    d, moved = _off_ties(c.dtype, d, s)
    _, again = _off_ties(c.dtype, d, s)          # the CPU check: the finished operands are clear of every tie that matters
    assert again == 0, f"{c.name}: {again} projections still lie on a rounding tie"
    # (each element at most once, by one ulp; at r = 2 every element of h matters and a fifth of A may move)
    print(f"{c.name}: {moved} of {d['A'].numel() + d['B'].numel()} elements of A and B moved by one ulp")
    return c, d


def _al256(n):
    return (n + 255) // 256 * 256


def _run(layers, runs=(0xFF, 0x00, 0xFF), what="short", share_w=False, stages=("fwd", "bwd", "weights")):
    """One sow_forward_short + sow_backward_short call over `layers` ((Case, operands) pairs of one dtype), then the weight
    phases layer by layer; repeated on re-poisoned memory.  Returns the outputs of the first run (CPU), one dict per layer.
    A layer of T = 0 (a Case of no rows over operands of d["rows"] rows; the calls skip it) has its outputs and its workspace
    allocated for d["rows"] rows: every byte of them must keep what each run fills it with (_untouched)."""
    lib = _lib.load()
    dtype = layers[0][0].dtype
    dt = E._dt(dtype)
    ar = E.Arena(dtype)
    n = len(layers)
    arr = (_lib.LayerArgs * n)()
    bufs, W0 = [], None
    for i, (c, d) in enumerate(layers):
        x, A, B, bias, dy = (ar.input(d[k]) for k in ("x", "A", "B", "bias", "dy"))
        W = W0 if (share_w and W0 is not None) else ar.input(d["W"])
        W0 = W0 if W0 is not None else W
        rows = c.T or d["rows"]
        o = dict(y=ar.output((rows, c.d_out)), h=ar.output((rows, 64)), dx=ar.output((rows, c.d_in)), dA=ar.output((c.d_in, c.r)),
                 dB=ar.output((c.r, c.d_out)), dbias=ar.output((c.d_out,)) if c.bias else None)
        nws = lib.sow_short_workspace_bytes(rows, c.d_in, c.d_out, c.r, _lib.ACC_DENSE, dt)
        assert nws >= lib.sow_workspace_bytes(rows, c.d_in, c.d_out, c.r, 0, _lib.ACC_DENSE, dt) > 0
        ws = ar.workspace(nws + 256 * i)         # (workspaces of different sizes)
        a = arr[i]
        a.x, a.A, a.B, a.acc_down, a.bias, a.y, a.h_save, a.dy, a.dx = (E._ptr(t) for t in (x, A, B, W, bias, o["y"], o["h"], dy, o["dx"]))
        a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = c.T, c.d_in, c.d_out, c.r, _lib.ACC_DENSE, c.s
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        bufs.append((x, A, B, bias, dy, W, ws, o))
    outs = []
    for byte in runs:
        ar.fill(byte)
        if "fwd" in stages:
            _lib.check(lib.sow_forward_short(arr, n, dt, E._stream()), "sow_forward_short")
        if "bwd" in stages:
            _lib.check(lib.sow_backward_short(arr, n, dt, E._stream()), "sow_backward_short")
        if "weights" in stages:
            for (c, _), (x, A, B, bias, dy, W, ws, o) in zip(layers, bufs):
                if c.T == 0:
                    continue
                _lib.check(lib.sow_backward_ex(E._ptr(dy), E._ptr(x), E._ptr(o["h"]), E._ptr(A), E._ptr(B), E._ptr(W), None, E._ptr(o["dx"]),
                                               E._ptr(o["dA"]), E._ptr(o["dB"]), E._ptr(o["dbias"]), c.T, c.d_in, c.d_out, c.r, 0,
                                               _lib.ACC_DENSE, c.s, 0.0, dt, ws.data_ptr(), ws.numel(), _lib.BWD_WEIGHTS, E._stream()),
                           "sow_backward_ex")
        ar.check_guards(f"{what} run {len(outs)}")
        for (c, _), b in zip(layers, bufs):
            if c.T == 0:
                _untouched(byte, b[7], b[6], f"{what} run {len(outs)}")
        outs.append([{k: (None if v is None else v.clone()) for k, v in b[7].items()} for b in bufs])
    keys = [k for k, st in (("y", "fwd"), ("h", "fwd"), ("dx", "bwd"), ("dA", "weights"), ("dB", "weights"), ("dbias", "weights")) if st in stages]
    for k in range(1, len(outs)):
        for i in range(n):
            for key in keys:
                if outs[0][i][key] is not None and layers[i][0].T:
                    assert torch.equal(E._bits(outs[0][i][key]), E._bits(outs[k][i][key])), f"{what}: {key} of layer {i} differs between run 0 and run {k}"
    return [{k: (None if v is None or k not in keys else v.cpu()) for k, v in o.items()} for o in outs[0]]


def _untouched(byte, outs, ws, what):
    """The outputs and the workspace of a T = 0 layer after a run on memory filled with `byte`: every byte is that byte still."""
    fill = -1 if byte == 0xFF else 0
    for k, v in outs.items():
        assert v is None or bool((E._bits(v) == fill).all()), f"{what}: {k} of a T = 0 layer was stored to"
    assert bool((ws == byte).all()), f"{what}: the workspace of a T = 0 layer was stored to"


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(E._bits(a), E._bits(b)), f"{what}: {int((E._bits(a) != E._bits(b)).sum())} elements differ"


def _same_outs(a, b, what, keys=("y", "h", "dx", "dA", "dB", "dbias")):
    for k in keys:
        if a.get(k) is not None:
            _same(a[k], b[k], f"{what}: {k}")


# ---- element-wise against float64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_elementwise_against_fp64(c):
    """y, h_save, dX, and the dA, dB, dbias of the unchanged weight phases, by test_gpu_elementwise's comparators."""
    case, d = _operands(*c)
    (out,) = _run([(case, d)], what=_id(c))
    E._check(case, d, out)


# ---- slab regimes ---------------------------------------------------------------------------------------------------------
# (T, d_in, d_out, forward slabs, data-phase slabs).  128 -> 256 at two row blocks: one slab either way.  2208 -> 72: two column
# ranges x two blocks ask for 128 slabs' worth of workgroups, so the forward takes the shortest slabs, 128 rows -- 18 of them,
# two past the 16 that phase B requests up front, the last one of 32 rows.  72 -> 4360: the same for the data phase, whose
# shortest slab is 256 (the waves take their k-steps in pairs): 18 slabs, the last one of 8 rows.  A longer contraction only
# adds slabs of the same kind: these are the most the plan makes of these widths.
REGIMES = [(100, 128, 256, 1, 1), (65, 2208, 72, 18, 1), (65, 72, 4360, 1, 18)]


@pytest.mark.parametrize("T,d_in,d_out,sf,sb", REGIMES, ids=lambda v: str(v))
def test_slab_regimes(T, d_in, d_out, sf, sb):
    lib = _lib.load()
    part = lambda S, N: _al256(S * T * N * 4) + _al256(S * T * 64 * 4)    # noqa: E731
    assert lib.sow_forward_short_workspace_bytes(T, d_in, d_out, 8, _lib.ACC_DENSE, _lib.BF16) == 256 + part(sf, d_out)
    base = lib.sow_workspace_bytes(T, d_in, d_out, 8, 0, _lib.ACC_DENSE, _lib.BF16)
    assert lib.sow_short_workspace_bytes(T, d_in, d_out, 8, _lib.ACC_DENSE, _lib.BF16) == base + max(part(sf, d_out), part(sb, d_in))
    case, d = _operands("bf16", T, d_in, d_out, 8, True, 0.5, 40)
    (out,) = _run([(case, d)], runs=(0xFF, 0x00), what=f"regime {T} {d_in} {d_out}")
    E._check(case, d, out)


# ---- exact operands -------------------------------------------------------------------------------------------------------
EXACT = [("bf16", 100, 264, 520, 50, True, 0.5), ("f16", 129, 520, 264, 8, True, 0.25), ("bf16", 65, 520, 264, 64, True, 1.0),
         ("f16", 100, 264, 520, 63, False, 0.5)]


@pytest.mark.parametrize("c", EXACT, ids=_id)
def test_exact_operands_bit_for_bit(c):
    """Small integers (value_plan.exact_layer, proved: every stored intermediate representable, every sum below 2^24 units in any
    order): every output equals the float64 result, bit for bit."""
    dt, T, d_in, d_out, r, bias, s = c
    lc = FP.Layer(name="short_exact_" + _id(c), dtype=dt, T=T, d_in=d_in, d_out=d_out, r=r, acc="dense", bias=bias, s=s, seed=11)
    d, f = VP.exact_layer_proved(lc)
    dtype = DT[dt]
    ops = {k: (None if v is None else v.to(dtype)) for k, v in d.items()}
    case = E.Case(lc.name, dtype, T, d_in, d_out, r, acc="dense", bias=bias, s=s)
    (out,) = _run([(case, ops)], what="exact " + _id(c))
    for k in ("y", "dx", "dA", "dB") + (("dbias",) if bias else ()):
        bad = to64(out[k]) != rne(f[k], dtype)
        assert not bad.any(), f"{k}: {int(bad.sum())} of {bad.numel()} elements differ from the float64 result; first at {tuple(int(v) for v in torch.nonzero(bad)[0])}"
    h = to64(out["h"])
    assert bool((h[:, :r] == f["h"]).all()), "h_save differs from the float64 projection"
    assert bool((h[:, r:63] == 0).all()) and (r == 64 or bool((h[:, 63] == 1).all())), "h_save: pad columns / the ones column"


# ---- rows -----------------------------------------------------------------------------------------------------------------
def test_65_rows_store_65_rows():
    """T = 65: the second block holds one row.  y, h_save and dX have 65 rows and a sentinel guard right behind them (_run checks
    it after each of the three runs): nothing is stored past row 64."""
    case, d = _operands("bf16", 65, 264, 520, 8, True, 1.0, 7)
    (out,) = _run([(case, d)], what="65 rows")
    assert out["y"].shape == (65, 520) and out["dx"].shape == (65, 264) and out["h"].shape == (65, 64)
    E._check(case, d, out)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_swapped_rows_give_swapped_rows(dt):
    """Rows 3 and 70 of x and dY swapped (another block, another place in it): y, h_save and dX with those rows swapped."""
    case, d = _operands(dt, 100, 264, 520, 50, True, 0.5, 3)
    perm = list(range(100))
    perm[3], perm[70] = 70, 3
    (a,) = _run([(case, d)], runs=(0xFF,), stages=("fwd", "bwd"), what="rows in place")
    (b,) = _run([(case, dict(d, x=d["x"][perm].contiguous(), dy=d["dy"][perm].contiguous()))], runs=(0xFF,), stages=("fwd", "bwd"), what="rows swapped")
    for k in ("y", "h", "dx"):
        _same(b[k], a[k][perm], f"{dt} {k} with rows 3 and 70 swapped")


@pytest.mark.parametrize("dt,k", [("bf16", 0), ("f16", 263)])
def test_a_nan_in_row_70_reaches_row_70_only(dt, k):
    case, d = _operands(dt, 100, 264, 520, 50, True, 0.5, 3)
    (clean,) = _run([(case, d)], runs=(0xFF,), stages=("fwd", "bwd"), what="clean")
    p = dict(d, x=d["x"].clone(), dy=d["dy"].clone())
    p["x"][70, k] = float("nan")
    p["dy"][70, 519 - k] = float("nan")
    (pois,) = _run([(case, p)], runs=(0xFF,), stages=("fwd", "bwd"), what="poisoned")
    keep = [t for t in range(100) if t != 70]
    assert bool(torch.isnan(pois["y"][70]).all()) and bool(torch.isnan(pois["dx"][70]).all()), "row 70 of y and dX must be NaN in every column"
    assert bool(torch.isnan(pois["h"][70, :50]).all()), "row 70 of h_save must be NaN in every live column"
    for key in ("y", "h", "dx"):
        _same(pois[key][keep], clean[key][keep], f"{dt} {key}: the other rows")


# ---- groups ---------------------------------------------------------------------------------------------------------------
def test_three_layers_equal_three_single_calls():
    """65 + 129 + 100 rows = 2 + 3 + 2 row blocks in one launch group, each layer with its own plan: every output of a layer is
    what its call alone gives."""
    layers = [_operands("bf16", 65, 264, 520, 8, True, 0.5, 20), _operands("bf16", 129, 520, 264, 64, False, 1.0, 21),
              _operands("bf16", 100, 264, 520, 50, True, 0.25, 22)]
    grouped = _run(layers, what="group")
    for i, (L, g) in enumerate(zip(layers, grouped)):
        (s,) = _run([L], runs=(0xFF,), what=f"single {i}")
        _same_outs(g, s, f"layer {i}")
        E._check(L[0], L[1], g)


def test_seventeen_row_blocks_take_two_launch_pairs():
    """1024 + 65 rows = 18 entries: the second layer's blocks are split over two launch pairs."""
    layers = [_operands("bf16", 1024, 264, 520, 8, True, 0.5, 23), _operands("bf16", 65, 520, 264, 2, True, 1.0, 24)]
    grouped = _run(layers, runs=(0xFF, 0x00), what="two pairs")
    for i, (L, g) in enumerate(zip(layers, grouped)):
        (s,) = _run([L], runs=(0xFF,), what=f"single {i}")
        _same_outs(g, s, f"layer {i}")


def test_two_layers_over_one_accumulator():
    """Two layers read ONE W buffer in one call (different x, factors and workspaces): neither disturbs the other."""
    a = _operands("bf16", 100, 264, 520, 50, True, 0.5, 30)
    c2 = E.Case("second_on_w", BF16, 129, 264, 520, 8, acc="dense", bias=False, s=1.0, seed=31)
    d2, _ = _off_ties(BF16, dict(E._inputs(c2), W=a[1]["W"]), 1.0)
    grouped = _run([a, (c2, d2)], share_w=True, what="one W")
    for i, (L, g) in enumerate(zip([a, (c2, d2)], grouped)):
        (s,) = _run([L], runs=(0xFF,), what=f"single {i}")
        _same_outs(g, s, f"layer {i} on the shared W")
        E._check(L[0], L[1], g)


def test_zz_report_worst_ratios():
    worst = {k: v for k, v in E.WORST.items() if any(k[0] == _operands(*c)[0].name for c in CASES)}
    for k, v in sorted(worst.items(), key=lambda kv: -kv[1][0])[:10]:
        print(f"{k}: worst err / bound {v[0]:.3f}")
    assert all(v[0] <= 1.0 for v in worst.values())
