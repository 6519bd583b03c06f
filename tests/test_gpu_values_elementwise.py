"""-m gpu: every kernel family on chosen operand *values* (tests/value_plan.py), through the element-wise harnesses of
tests/test_gpu_elementwise.py and tests/test_gpu_fuzz_elementwise.py (NaN-neighboured inputs, sentinel guards, three runs
-- poisoned, zeroed, poisoned -- that must be bit-identical).

A  exact operands (value_plan.exact_layer / exact_gemm, proved exact on the CPU by tests/test_value_plan_cpu.py): every
   output -- y, h_save with its padding and ones column, dX, dA, dB, dbias, GEMM C, the updated accumulator -- equals
   rne(ref64, dtype) bit for bit (_exact: no tolerance argument other than 0).  The sign of a zero is not compared: a
   sum that cancels is +0 in any order, but alpha < 0 times +0 is -0, and the float64 reference carries neither.
B  the same operands, and Gaussian ones, scaled by powers of two over value_plan.GRID: against float64 with the existing
   limits (zero tolerance for the exact operands), and bit-identical to the unscaled run after the exponent shift.
C  one NaN / +Inf / -Inf inside the data: the mask of non-finite output elements equals that of the float64 reference on
   the same operands, every other element is bit-identical to the clean run; bf16 / f16: where the reference is an Inf the
   kernel's is the same Inf (fp32 runs on the 3 x bf16 split, which turns an Inf operand into NaN: mask only).  One stated
   exception (include/sow_amd.h): a non-finite element of A may take the dX columns of the rows of A stored just before it
   along -- the kernels read a row of A with its successors against explicit zeros.
test_zz_value_coverage (last) asserts from the kernel traces that every family of fuzz_plan.FAMILIES_FIRST was reached by an
exact case and a scaled case, and the chain / GEMM / weight-gradient families by a poisoned case.
"""
import dataclasses

import pytest
import torch

import fuzz_plan as FP
import test_gpu_autocast as AC
import test_gpu_elementwise as E
import test_gpu_fuzz_elementwise as Z
import test_gpu_shared_input as S
import test_gpu_step_elementwise as ST
import value_plan as V
from numerics import check_rounded, rne, to64
from sow_amd import _lib

pytestmark = pytest.mark.gpu
DT = V.DT
CASES = V.cases()
PLANNED = len(CASES.layers) + len(CASES.groups) + len(CASES.shared) + len(CASES.gemms)
CLEAN = {}                                   # clean accumulator outputs of test_exact_accumulate_and_axpby
SEEN = {"A": {}, "B": {}, "C": {}}           # family -> label -> case names
WORST_B = {}                                 # label -> (worst err / limit of a scaled Gaussian run, case)
COUNT = {"C": 0, "B": 0, "exact_elements": 0}
RAN = set()
# B runs on every exact layer and on every n-th layer with Gaussian operands; C on the first layer of each stratum below
# (one per chain / weight-gradient family, the ragged and the misaligned ones for the wrap-around placement)
B_GAUSS_EVERY = 5
C_STRATA = ("chain2", "short", "gemm4h", "gemm2h", "dense_short", "lowrank", "wide", "ragged", "chain3f", "chain2f", "tn_f32",
            "gemm_x3", "generic")


def _note(fam, name, labels):
    for lab in labels:
        SEEN[fam].setdefault(lab, set()).add(name)


def _exact(out, ref, dtype, name):
    """Bit equality with rne(ref64, dtype) (zeros compared as zeros)."""
    check_rounded(out, ref, dtype, max_ulp=0, max_inexact=0, min_count=0, name=name)
    want = rne(ref, dtype).to(dtype)
    assert torch.equal(E._bits(out.cpu() + 0), E._bits(want + 0)), f"{name}: bits differ from rne(ref64)"
    COUNT["exact_elements"] += out.numel()


def _h_full(c, f):
    """The reference of the whole h_save buffer: [T, r] = x A for r > 64, else [T, 64] with s x A in the live columns,
    zeros up to column 62 and the ones column 63 (r <= 63)."""
    if c.r > 64:
        return f["xA"]
    h = torch.zeros(c.T, 64, dtype=torch.float64)
    h[:, :c.r] = f["h"]
    if c.r <= 63:
        h[:, 63] = 1.0
    return h


def _shifted(f, c, e):
    """References of the operands scaled by e: exact powers of two of the unscaled ones."""
    exp = e.exps()
    return {k: torch.ldexp(v, torch.tensor(exp[k])) for k, v in f.items() if isinstance(v, torch.Tensor) and k in exp}


def _check_exact_layer(c, f, out, name, e=None):
    dtype = DT[c.dtype]
    g = f if e is None else _shifted(f, c, e)
    if out.get("h") is not None:
        h = _h_full(c, g)
        if e is not None and c.r <= 63:
            h[:, 63] = 1.0
        _exact(out["h"], h, dtype, f"{name}: h_save")
    for k, o in (("y", "y"), ("dx", "dx"), ("dA", "dA"), ("dB", "dB"), ("dbias", "dbias")):
        if out.get(o) is not None:
            _exact(out[o], g[k], dtype, f"{name}: {o}")


def _shift_identity(c, out, base, e, name, skip=()):
    """Bits of the scaled run equal the unscaled run's after the exponent shift (the ones column of h_save stays 1)."""
    exp = e.exps()
    for k, ek in (("y", "y"), ("h", "h"), ("dx", "dx"), ("dA", "dA"), ("dB", "dB"), ("dbias", "dbias")):
        if out.get(k) is None or ek in skip:
            continue
        want = torch.ldexp(base[k].double(), torch.tensor(exp[ek]))
        if k == "h" and c.r <= 63:
            want[:, 63] = 1.0
        want = want.to(base[k].dtype)
        same = torch.equal(E._bits(out[k] + 0), E._bits(want + 0))
        assert same, (f"{name}: {k} differs from the unscaled run shifted by 2^{exp[ek]} in "
                      f"{int((out[k] != want).sum())} of {want.numel()} elements")


def _case(c):
    return Z._to_case(c, c.y_rounds, c.dx_rounds)


# ------------------------------------------------------------------------------------------------------------- A, B: layers
@pytest.mark.parametrize("i,c", list(enumerate(CASES.layers)), ids=lambda v: v.name if isinstance(v, FP.Layer) else "")
def test_exact_and_scaled_layer(i, c):
    """A: the exact operands, bit for bit.  B: the same operands at two grid points -- the highest the case admits (cases of
    odd index: the second highest) and the lowest; f16: the GradScaler point too where admitted -- bit for bit against the
    shifted reference and the shifted unscaled run.  The long-T 16-bit cases run A again with fp32 gradients."""
    RAN.add(c.name)
    d, f = V.exact_layer_proved(c)
    trace = {}
    base = E._run_single(_case(c), d, trace)
    seq = trace["fwd"] + trace.get("bwd", [])
    assert Z._has(seq, c.family), f"{c.name}: targets {c.family}, the trace holds {sorted(set(seq))}"
    labels = Z._labels(seq, c)
    _check_exact_layer(c, f, base, c.name)
    _note("A", c.name, labels)
    grid = V.grid_for(c, V.range_stats(c, d, f), exact=True)
    assert len(grid) >= 2, f"{c.name}: the grid admits {len(grid)} points"
    if V.f32_gradients(c):
        _check_f32_gradients(c, d, f)
    points = [grid[i % 2 if len(grid) > 2 else 0][0], grid[-1][0]]
    if c.dtype == "f16" and V.GRADSCALER in [e for e, _ in grid] and V.GRADSCALER not in points:
        points.append(V.GRADSCALER)
    for e in points:
        out = E._run_single(_case(c), V.scale_layer(d, e))
        name = f"{c.name} @ {e.tag()}"
        _check_exact_layer(c, f, out, name, e)
        _shift_identity(c, out, base, e, name)
        COUNT["B"] += 1
    _note("B", c.name, labels)


def _check_f32_gradients(c, d, f):
    """The same exact operands with fp32 parameters and gradients (SOW_PARAM_F32; the C-ABI runner of test_gpu_autocast.py,
    two bit-identical runs with intact guards): dA, dB and dbias are exact sums below 2^24 units, representable in fp32
    (value_plan.check_density), so every one of their elements must equal the reference -- no 16-bit rounding is left to
    hide a dropped token; y, h_save and dX as in the 16-bit run."""
    dtype = DT[c.dtype]
    da = dict(x=d["x"], A=d["A"], B=d["B"], bias=d.get("bias"), dy=d["dy"], acc_down=d.get("W", d.get("Q")), acc_up=d.get("R"),
              dA0=d.get("dA0"), dB0=d.get("dB0"), dbias0=d.get("dbias0"))
    with _lib.switch(**c.switches):
        out = AC._run(da, dtype, c.T, c.d_in, c.d_out, c.r, c.acc, c.r_acc, c.s, True, grad_beta=c.grad_beta)
    name = f"{c.name} fp32 gradients"
    for k in ("dA", "dB", "dbias"):
        if out.get(k) is not None:
            assert out[k].dtype == torch.float32
            _exact(out[k].cpu(), f[k], torch.float32, f"{name}: {k}")
    _exact(out["h"].cpu(), _h_full(c, f), dtype, f"{name}: h_save")
    _exact(out["y"].cpu(), f["y"], dtype, f"{name}: y")
    _exact(out["dx"].cpu(), f["dx"], dtype, f"{name}: dx")
    COUNT["f32_gradients"] = COUNT.get("f32_gradients", 0) + 1


@pytest.mark.parametrize("c", CASES.layers[1::B_GAUSS_EVERY], ids=lambda c: c.name)
def test_scaled_gaussian_layer(c):
    """Gaussian operands: the float64 limits of test_gpu_elementwise._check at every admitted grid point, and the shift
    identity wherever the reference stays in the normal range.  f16 Gaussian data reaches below 2^-14 unscaled (h and dh
    hold elements of any size): there only the upper end of the range is required and only the float64 limits asserted."""
    case = _case(c)
    d = {k: (None if v is None else to64(v)) for k, v in E._inputs(case).items()}
    trace = {}
    base = E._run_single(case, d, trace)
    labels = Z._labels(trace["fwd"] + trace.get("bwd", []), c)
    E._check(case, d, base)
    st = V.range_stats(c, d)
    grid = V.grid_for(c, st, exact=False, bottom=c.dtype != "f16")
    assert grid, f"{c.name}: the grid admits no point"
    for e, below in (grid[:1] + grid[-1:] if len(grid) > 1 else grid):
        ds = V.scale_layer(d, e)
        out = E._run_single(case, ds)
        name = f"{c.name} @ {e.tag()}"
        scaled = dataclasses.replace(case, name=name)
        E._check(scaled, ds, out)
        if c.dtype != "f16":
            _shift_identity(c, out, base, e, name, skip=below)
        w = Z._case_worst(name)
        for lab in labels:
            if w is not None and w > WORST_B.get(lab, (-1.0, ""))[0]:
                WORST_B[lab] = (w, name)
        COUNT["B"] += 1
    _note("B", c.name, labels)


# ------------------------------------------------------------------------------------------------------------- C: layers
def _poisoned_layers():
    out, seen = [], set()
    for c in CASES.layers:
        key = (c.stratum, c.dtype if c.stratum in ("chain2", "generic", "ragged") else "")
        if c.stratum in C_STRATA and key not in seen:
            seen.add(key)
            out.append(dataclasses.replace(c, save_h=True))   # (a forward-only case of the plan runs its backward here)
    return out


def _check_poisoned(c, f, out, clean, name, keys, allow=None):
    """Mask of non-finite elements as the float64 reference's; everything else bit-identical to the clean run; bf16 / f16:
    an Inf of the reference is that Inf.  `allow`: output -> mask of the elements the stated contract lets a non-finite A
    take along (value_plan.a_overlap_columns); outside it the masks are equal."""
    for k in keys:
        if out.get(k) is None:
            continue
        ref = _h_full(c, f) if k == "h" else f[k]
        o, cl = out[k].cpu(), clean[k].cpu()
        bad_ref, bad = ~torch.isfinite(ref), ~torch.isfinite(o.float())
        free = allow[k] if allow and k in allow else torch.zeros_like(bad)
        leaked, missing = bad & ~bad_ref & ~free, ~bad & bad_ref
        assert not leaked.any() and not missing.any(), (
            f"{name}: {k}: {int(bad.sum())} non-finite elements, the float64 reference has {int(bad_ref.sum())}; "
            f"{int(leaked.sum())} leaked (columns {torch.nonzero(leaked.reshape(-1, leaked.shape[-1]).any(0)).flatten().tolist()[:12]}), "
            f"{int(missing.sum())} missing")
        same = E._bits(o)[~bad] == E._bits(cl)[~bad]
        assert bool(same.all()), f"{name}: {k}: {int((~same).sum())} finite elements differ from the clean run"
        if c.dtype != "f32":
            inf = torch.isinf(ref)
            assert bool((o.double()[inf] == ref[inf]).all()), f"{name}: {k}: an Inf of the reference came out as something else"


@pytest.mark.parametrize("c", _poisoned_layers(), ids=lambda c: c.name)
def test_poisoned_layer(c):
    case = _case(c)
    d = {k: (None if v is None else to64(v)) for k, v in E._inputs(case).items()}
    trace = {}
    clean = E._run_single(case, d, trace)
    labels = Z._labels(trace["fwd"] + trace.get("bwd", []), c)
    keys = ("h", "y", "dx", "dA", "dB", "dbias")
    for tag, operand, where in V.poisons(c):
        for value in V.POISON_VALUES:   # NaN, then +Inf, then -Inf
            dp = V.poison(d, operand, where, value)
            out = E._run_single(case, dp)
            allow = None
            if operand == "A":
                allow = dict(dx=torch.zeros(c.T, c.d_in, dtype=torch.bool))
                cols = V.a_overlap_columns(c, *where[0])
                allow["dx"][:, cols.start:cols.stop] = True
            _check_poisoned(c, V.layer_refs(c, dp), out, clean, f"{c.name} {tag}={value}", keys, allow)
            COUNT["C"] += 1
    _note("C", c.name, labels)


# ------------------------------------------------------------------------------------------------------------- groups
@pytest.mark.parametrize("gp", CASES.groups, ids=lambda g: g.name)
def test_exact_and_poisoned_group(gp):
    RAN.add(gp.name)
    members = [dataclasses.replace(c, name=f"{gp.name}.{c.name}") for c in gp.layers]
    layers = [Z._to_case(c, "once", "once") for c in members]
    proved = [V.exact_layer_proved(c) for c in members]
    outs, seq = Z.run_group(gp, layers, [d for d, _ in proved])
    labels = Z._labels(seq)
    for c, (d, f), out in zip(members, proved, outs):
        _check_exact_layer(c, f, out, c.name)
    _note("A", gp.name, labels)
    # B: the whole group at one grid point (the first every member admits)
    grids = [[e for e, _ in V.grid_for(c, V.range_stats(c, d, f), exact=True)] for c, (d, f) in zip(members, proved)]
    common = [e for e in V.GRID[members[0].dtype] if all(e in g for g in grids)]
    assert common, f"{gp.name}: no grid point admitted by every member"
    e = common[-1]
    outs_s, _ = Z.run_group(gp, layers, [V.scale_layer(d, e) for d, _ in proved])
    for c, (d, f), out, base in zip(members, proved, outs_s, outs):
        _check_exact_layer(c, f, out, f"{c.name} @ {e.tag()}", e)
        _shift_identity(c, out, base, e, f"{c.name} @ {e.tag()}")
    COUNT["B"] += 1
    _note("B", gp.name, labels)
    # C: Gaussian operands, a NaN in x of the first member and a -Inf in dY of the last: the others stay bit-identical
    data = [{k: (None if v is None else to64(v)) for k, v in E._inputs(cs).items()} for cs in layers]
    clean, _ = Z.run_group(gp, layers, data)
    pd = list(data)
    first, last = members[0], members[-1]
    pd[0] = V.poison(data[0], "x", [(first.T // 2, first.d_in // 2)], float("nan"))
    pd[-1] = V.poison(data[-1], "dy", [(last.T - 1, last.d_out - 1)], float("-inf"))
    outs_p, _ = Z.run_group(gp, layers, pd)
    for c, dp, out, cl in zip(members, pd, outs_p, clean):
        _check_poisoned(c, V.layer_refs(c, dp), out, cl, f"{c.name} poisoned group", ("h", "y", "dx", "dA", "dB", "dbias"))
    COUNT["C"] += 1
    _note("C", gp.name, labels)


# ------------------------------------------------------------------------------------------------------------- shared input
def _shared_ref_dx(sp, fs, dx0):
    return sum(f["dx"] for f in fs) + (sp.grad_beta * to64(dx0) if sp.grad_beta else 0)


@pytest.mark.parametrize("sp", CASES.shared, ids=lambda s: s.name)
def test_exact_and_poisoned_shared(sp):
    RAN.add(sp.name)
    dtype = DT[sp.dtype]
    sp = dataclasses.replace(sp, sibs=[dataclasses.replace(sb, s=V._pow2(sb.s)) for sb in sp.sibs])
    st = Z.shared_set(sp)
    sibs, x, per, dx0, fs, ref_dx = V.exact_shared(sp)
    b, runs, seq = Z.run_shared(st, x, per, dx0)
    labels = Z._labels(seq)
    for c, f, out in zip(sibs, fs, runs[0][0]):
        _check_exact_layer(c, f, dict(out), c.name)
    _exact(runs[0][1], ref_dx, dtype, f"{sp.name}: dX")
    _note("A", sp.name, labels)
    _scaled_shared(sp, st, sibs, x, per, dx0, fs, ref_dx, runs)
    _note("B", sp.name, labels)
    # C: Gaussian operands; a NaN in the shared x, then a +Inf in the dY of the last sibling
    xg, perg, dx0g = S._data(st, seed=3)
    quant = lambda t: None if t is None else to64(t.to(dtype))   # noqa: E731
    xg, dx0g = quant(xg), quant(dx0g)
    perg = [{k: quant(v) for k, v in p.items()} for p in perg]
    _, clean, _ = Z.run_shared(st, xg, perg, dx0g)
    for what in ("x", "dy"):
        xp, pp = xg, [dict(p) for p in perg]
        if what == "x":
            xp = xg.clone()
            xp[sp.T // 2, sp.d_in // 2] = float("nan")
        else:
            pp[-1]["dy"] = perg[-1]["dy"].clone()
            pp[-1]["dy"][sp.T - 1, 0] = float("inf")
        _, runs_p, _ = Z.run_shared(st, xp, pp, dx0g)
        fp = [V.layer_refs(c, dict(x=xp, **p)) for c, p in zip(sibs, pp)]
        for c, f, out, cl in zip(sibs, fp, runs_p[0][0], clean[0][0]):
            _check_poisoned(c, f, out, cl, f"{c.name} poisoned {what}", ("h", "y", "dA", "dB", "dbias"))
        fdx = dict(dx=_shared_ref_dx(sp, fp, dx0g))
        _check_poisoned(sibs[0], fdx, dict(dx=runs_p[0][1]), dict(dx=clean[0][1]), f"{sp.name} poisoned {what}", ("dx",))
        COUNT["C"] += 1
    _note("C", sp.name, labels)


def _scaled_shared(sp, st, sibs, x, per, dx0, fs, ref_dx, base):
    """B for a sibling set: one grid point admitted by every sibling (the siblings share x, so one exponent for x; A, B and
    dY take the same exponents in every sibling so that the one dX is a pure shift)."""
    dtype = DT[sp.dtype]
    ds = [dict(x=x, **p) for p in per]
    grids = [[e for e, _ in V.grid_for(c, V.range_stats(c, d, f), exact=True)] for c, d, f in zip(sibs, ds, fs)]
    common = [e for e in V.GRID[sp.dtype] if all(e in g for g in grids)]
    assert common, f"{sp.name}: no grid point admitted by every sibling"
    e = common[0]
    exp = e.exps()
    sc = [V.scale_layer(d, e) for d in ds]
    dx0s = None if dx0 is None else torch.ldexp(dx0, torch.tensor(exp["dx"]))
    _, runs, _ = Z.run_shared(st, sc[0]["x"], [dict(A=d["A"], B=d["B"], bias=d["bias"], dy=d["dy"]) for d in sc], dx0s)
    for c, f, out, b0 in zip(sibs, fs, runs[0][0], base[0][0]):
        _check_exact_layer(c, f, dict(out), f"{c.name} @ {e.tag()}", e)
        _shift_identity(c, dict(out), b0, e, f"{c.name} @ {e.tag()}")
    _exact(runs[0][1], torch.ldexp(ref_dx, torch.tensor(exp["dx"])), dtype, f"{sp.name} @ {e.tag()}: dX")
    COUNT["B"] += 1


# ------------------------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("gm", CASES.gemms, ids=lambda g: g.name)
def test_exact_scaled_and_poisoned_gemm(gm):
    RAN.add(gm.name)
    dtype = DT[gm.dtype]
    a, b, bias, c0 = V.exact_gemm(gm)
    ref = V.prove_gemm(gm, a, b, bias, c0)
    out, seq = Z.run_gemm(gm, a, b, bias, c0)
    labels = Z._labels(seq)
    _exact(out, ref, dtype, gm.name)
    _note("A", gm.name, labels)
    # B: a * 2^ea, b * 2^eb, bias and C0 * 2^(ea + eb); the top and the bottom of the normal range
    for ea, eb in V.gemm_scales(gm):
        sh = lambda t, k: None if t is None else torch.ldexp(t, torch.tensor(k))   # noqa: E731
        V.prove_gemm_range(gm, a, b, bias, c0, ea, eb)
        out_s, _ = Z.run_gemm(gm, sh(a, ea), sh(b, eb), sh(bias, ea + eb), sh(c0, ea + eb))
        _exact(out_s, sh(ref, ea + eb), dtype, f"{gm.name} @ a{ea:+d} b{eb:+d}")
        want = torch.ldexp(out.double(), torch.tensor(ea + eb)).to(dtype)
        assert torch.equal(E._bits(out_s + 0), E._bits(want + 0)), f"{gm.name} @ a{ea:+d} b{eb:+d}: not the unscaled run shifted"
        COUNT["B"] += 1
    _note("B", gm.name, labels)
    # C: Gaussian operands; NaN in a, +Inf in the last row of a, -Inf in b
    g = torch.Generator().manual_seed(6000 + gm.seed)
    ag = to64(torch.randn(gm.M, gm.K, generator=g).to(dtype))
    bg = to64((torch.randn(gm.K, gm.N, generator=g) * 0.05).to(dtype))
    biasg = to64((torch.randn(gm.N, generator=g) * 0.1).to(dtype)) if gm.bias else None
    c0g = to64(torch.randn(gm.M, gm.N, generator=g).to(dtype)) if gm.beta else None
    clean, _ = Z.run_gemm(gm, ag, bg, biasg, c0g)
    fake = FP.Layer(gm.name, gm.dtype, gm.M, gm.K, gm.N, 1)
    for which, (i, j), value in (("a", (gm.M // 2, gm.K // 3), float("nan")), ("a", (gm.M - 1, gm.K - 1), float("inf")),
                                 ("b", (gm.K // 2, gm.N - 1), float("-inf"))):
        ap, bp = ag.clone(), bg.clone()
        (ap if which == "a" else bp)[i, j] = value
        out_p, _ = Z.run_gemm(gm, ap, bp, biasg, c0g)
        _check_poisoned(fake, dict(C=V.gemm_ref(gm, ap, bp, biasg, c0g)), dict(C=out_p), dict(C=clean),
                        f"{gm.name} {which}[{i}, {j}]={value}", ("C",))
        COUNT["C"] += 1
    _note("C", gm.name, labels)


# ------------------------------------------------------------------------------------------------------------- B: subnormals
SUBNORMAL = {}   # (case, stage) -> "gradual" | "flush" | "between"


def _subnormal_layers():
    out, seen = [], set()
    for c in CASES.layers:
        key = (c.stratum, c.dtype)
        if c.stratum in ("chain2", "short", "generic", "chain3f", "chain2f") and c.acc is None and c.r <= 64 and c.save_h \
                and not c.switches and key not in seen:
            seen.add(key)
            out.append(c)
    return out


def _envelope_check(out, ref, ref_flushed, env, dtype, floor, name):
    """The flush-to-zero envelope: |out - ref64| within the usual limit plus env = sum_k |flushed_k| |other_k|.  Returns
    which of the two behaviours the result shows: within the usual limit of the gradual reference, of the flushed one, or
    of neither (between them)."""
    if dtype == torch.float32:
        from numerics import bound, check_bound
        check_bound(out, ref, bound(ref, dtype, floor, env), name=name)
        check = lambda r: check_bound(out, r, bound(r, dtype, floor), name=name)   # noqa: E731
    else:
        check_rounded(out, ref, dtype, acc=floor + env, name=name)
        check = lambda r: check_rounded(out, r, dtype, acc=floor, name=name)   # noqa: E731
    for label, r in (("gradual", ref), ("flush", ref_flushed)):
        try:
            check(r)
            return label
        except AssertionError:
            pass
    return "between"


@pytest.mark.parametrize("c", _subnormal_layers(), ids=lambda c: c.name)
def test_subnormal_operands_stay_in_the_flush_envelope(c):
    """Operands below the normal range.  bf16 / fp32: x = Gaussian * 2^-127 (most elements subnormal) against A * 2^100, so
    that h = s x A is an ordinary number if the matrix pipe reads subnormal inputs and loses their terms if it flushes them.
    f16: A scaled so that h lands around 2^-16 -- h_save keeps subnormals (include/sow_amd.h); whether the second product
    reads them is what is observed.  Asserted: the envelope between the two behaviours, and for bf16 / f16 -- where
    include/sow_amd.h states it -- gradual underflow; printed: which one it was."""
    from numerics import fp32_floor
    case = _case(c)
    dtype = DT[c.dtype]
    d = {k: (None if v is None else to64(v)) for k, v in E._inputs(case).items()}
    # what a flushing matrix pipe loses: values below the normal range; on the 3 x bf16 split of fp32 also the mid / lo
    # planes of values below 2^-110, which are bf16 subnormals themselves
    lo = 2.0 ** (V.EMIN[c.dtype] + (16 if c.dtype == "f32" else 0))
    if c.dtype == "f16":
        d["A"] = to64(torch.ldexp(d["A"], torch.tensor(-16)).to(dtype))
        d["B"] = to64(torch.ldexp(d["B"], torch.tensor(12)).to(dtype))
    else:
        d["x"] = to64(torch.ldexp(d["x"], torch.tensor(-127)).to(dtype))
        d["A"] = to64(torch.ldexp(d["A"], torch.tensor(100)).to(dtype))
    trace = {}
    out = E._run_single(case, d, trace)
    fam = sorted(lab for lab in Z._labels(trace["fwd"], c) if "chain" in lab)
    x, A, B, s = d["x"], d["A"], d["B"], c.s
    bias = d["bias"] if d.get("bias") is not None else 0
    flush = lambda t: torch.where(t.abs() < lo, torch.zeros_like(t), t)   # noqa: E731
    xf, Af = flush(x), flush(A)
    h_ref, h_flushed = s * (x @ A), s * (xf @ Af)
    env_h = abs(s) * (x.abs() @ A.abs() - xf.abs() @ Af.abs())
    h = to64(out["h"])[:, :c.r]
    SUBNORMAL[(c.name, "h")] = _envelope_check(h, h_ref, h_flushed, env_h, dtype, fp32_floor(s * s * ((x * x) @ (A * A)), c.d_in),
                                               f"{c.name}: h_save")
    hf, Bf = flush(h), flush(B)
    y_ref, y_flushed = h @ B + bias, hf @ Bf + bias
    env_y = h.abs() @ B.abs() - hf.abs() @ Bf.abs()
    SUBNORMAL[(c.name, "y")] = _envelope_check(out["y"], y_ref, y_flushed, env_y, dtype,
                                               fp32_floor((h * h) @ (B * B), c.d_in + 64), f"{c.name}: y")
    if c.dtype != "f32":   # the header's contract: the bf16 / f16 matrix pipe reads subnormal operands at their value
        for stage in ("h", "y"):
            assert SUBNORMAL[(c.name, stage)] == "gradual", \
                f"{c.name}: {stage} is not within the usual limit of the gradual-underflow reference ({SUBNORMAL[(c.name, stage)]})"
    share = float(((x.abs() < lo) & (x != 0)).double().mean()), float(((h.abs() < lo) & (h != 0)).double().mean())
    print(f"subnormal {c.name} {fam}: {100 * share[0]:.0f} % of x, {100 * share[1]:.0f} % of h_save subnormal; "
          f"h_save {SUBNORMAL[(c.name, 'h')]}, y {SUBNORMAL[(c.name, 'y')]}")


# ------------------------------------------------------------------------------------------------------------- helpers
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=lambda d: str(d).split(".")[-1])
def test_exact_accumulate_and_axpby(dtype):
    """sow_accumulate_batch's rank update acc = beta acc + scale A B and sow_axpby y = a x + b y on exact operands (half-
    integers, power-of-two scalars): bit-equal to rne(ref64); one NaN in A stays in its row of the accumulator."""
    lib = _lib.load()
    items = [(259, 100, 7, 1.0, -0.5), (512, 1001, 64, 0.0, 2.0), (100, 259, 1, 1.0, 0.25)]
    for poisoned in (False, True):
        g = torch.Generator().manual_seed(9)   # the same operands in both passes
        ar = ST.Arena()
        args = (_lib.AccumulateArgs * len(items))()
        views, refs = {}, {}
        for i, (d_in, d_out, r, beta, scale) in enumerate(items):
            A0 = V._ternary(g, (d_in, r), min(1.0, 4.0 / r))
            B0 = V._ternary(g, (r, d_out), min(1.0, 4.0 / r), 0.5)
            acc0 = V._ternary(g, (d_in, d_out), 0.5, 0.5)
            if poisoned:
                A0[d_in // 2, r // 2] = float("nan")
            acc = ar.output((d_in, d_out), dtype, initial=acc0.to(dtype) if beta else None)
            A, B = ar.input(A0.to(dtype)), ar.input(B0.to(dtype))
            a = args[i]
            a.acc, a.A, a.B = ST._p(acc), ST._p(A), ST._p(B)
            a.d_in, a.d_out, a.r, a.r_new = d_in, d_out, r, r
            a.scale, a.acc_beta = scale, beta
            views[f"acc{i}"] = acc
            refs[f"acc{i}"] = (beta * acc0 if beta else 0) + scale * (A0 @ B0)
        out = ar.run3(f"accumulate values {dtype}",
                      lambda: _lib.check(lib.sow_accumulate_batch(args, len(items), ST.DT[dtype], ST._s()), "sow_accumulate_batch"),
                      views)
        for k, ref in refs.items():
            if not poisoned:
                _exact(out[k], ref, dtype, f"accumulate {k}")
                CLEAN[("acc", dtype, k)] = out[k]
            else:
                bad = ~torch.isfinite(out[k].float())
                assert torch.equal(bad, ~torch.isfinite(ref)), f"accumulate {k}: the NaN of A left its row"
                cl = CLEAN[("acc", dtype, k)]
                assert torch.equal(E._bits(out[k])[~bad], E._bits(cl)[~bad]), f"accumulate {k}: finite elements moved"
    n = 2048 * 256 + 77
    x0, y0 = V._ternary(g, (n,), 0.75, 0.5), V._ternary(g, (n,), 0.75, 0.25)
    ar = ST.Arena()
    x = ar.input(x0.to(dtype))
    y = ar.output((n,), dtype, initial=y0.to(dtype))
    out = ar.run3("axpby values", lambda: _lib.check(lib.sow_axpby(ST._p(x), ST._p(y), n, 0.5, -2.0, ST.DT[dtype], ST._s()),
                                                     "sow_axpby"), dict(y=y))["y"]
    _exact(out, 0.5 * x0 - 2.0 * y0, dtype, "axpby")


# ------------------------------------------------------------------------------------------------------------- coverage
C_FAMILIES = tuple(f for f in FP.FAMILIES_FIRST if f not in ("h_reduce_kernel", "colsum_kernel"))


def test_zz_value_coverage():
    """Every family of fuzz_plan.FAMILIES_FIRST reached by an exact case (A) and a scaled case (B), every chain / GEMM /
    weight-gradient family by a poisoned case (C); prints the counts per family (run with -s)."""
    if len(RAN) < PLANNED:   # RAN holds every case that started: one that failed leaves its family short below
        pytest.skip(f"the coverage check runs after the whole file ({len(RAN)} of {PLANNED} cases started)")
    for fam in FP.FAMILIES_FIRST:
        w, case = WORST_B.get(fam, (float("nan"), ""))
        print(f"family {fam:58s} exact {len(SEEN['A'].get(fam, ())):3d}  scaled {len(SEEN['B'].get(fam, ())):3d}  poisoned "
              f"{len(SEEN['C'].get(fam, ())):3d}  worst scaled Gaussian err/limit {w:.3f}  ({case})")
    print(f"{COUNT['exact_elements']} elements compared bit for bit, {COUNT.get('f32_gradients', 0)} runs with fp32 gradients, "
          f"{COUNT['B']} scaled runs, {COUNT['C']} poisoned placements")
    for fam_set, fams in (("A", FP.FAMILIES_FIRST), ("B", FP.FAMILIES_FIRST), ("C", C_FAMILIES)):
        missing = [f for f in fams if not SEEN[fam_set].get(f)]
        assert not missing, f"families without a case of {fam_set}: {missing}"
