"""The plan of tests/test_gpu_rows_sweep.py (tests/rows_plan.py), tested on the CPU (no `gpu` mark): deterministic; the mirrors of
the C planning functions against the library's workspace queries; every class the sweep is there for counted over the drawn cases;
the float64 reference work under what the seeded sweep of fuzz_plan needs today; the operands of every case built with the
generators the GPU tests use; and the comparators of those tests shown to REJECT a float64 result that leaves one class out -- the
proof, for the reference alone, that a kernel wrong in that class cannot pass."""
import collections
import random

import pytest
import torch

import fuzz_plan as FP
import rows_plan as RP
from numerics import rne, to64

FMT = {"dense": "dense", "e4m3": "fp8", "mxfp4": "fp4", "none": "none"}
CPU_CODES_MAX = 1 << 20     # the largest code matrix the generators quantise on the CPU (larger ones go through the GPU quantiser)


def _members(p):
    return [m for g in p.short_groups for m in g.layers]


# ---- determinism -----------------------------------------------------------------------------------------------------------------------------
def test_plan_is_deterministic():
    a, b = RP.plan(), RP.plan()
    assert a == b and RP.plan(RP.SEED + 1) != a
    names = [c.name for c in a.rows + a.short + a.short_codes + a.short_groups + _members(a)]
    assert len(set(names)) == len(names)
    for c in a.rows + a.short + a.short_codes:
        assert f"T{c.T}" in c.name and f"{c.d_in}x{c.d_out}" in c.name and f"r{c.r}" in c.name
    for c in a.rows:
        S, ks, _ = c.plan()
        assert f"_KS{ks}x{S}" in c.name
    for c in a.short + a.short_codes:
        (sf, kf, _), (sb, kb, _) = c.fwd(), c.bwd()
        assert f"_KS{kf}x{sf}_KS{kb}x{sb}" in c.name


def test_fuzz_plan_is_left_alone():
    """rows_plan draws from a generator of its own: fuzz_plan.plan() is what it is without it (its own CPU test pins the streams)."""
    before = FP.plan()
    RP.plan()
    assert FP.plan() == before and RP.SEED not in (FP.SEED, FP.SEED + 1)


# ---- the mirrors against the library --------------------------------------------------------------------------------------------------------
def _shape(g, kind, tmax):
    """A seeded shape; about a fifth of them outside the admitted set (each way of being outside in turn)."""
    step = FP.sk_step(kind)
    T, r = g.choice([g.randint(1, tmax), g.randint(max(tmax - 70, 1), tmax), g.randint(33, 64)]), g.randint(1, 64)
    d_out = 8 * g.randint(1, g.choice([16, 128, 1200]))
    d_in = step * g.randint(1, g.choice([64, 512, 32768 // step]))
    bad = g.randint(0, 24)
    if bad == 0:
        T = g.choice([0, tmax + 1, tmax + 64])
    elif bad == 1:
        r = g.choice([0, 65, 128])
    elif bad == 2:
        d_in += g.choice([1, 4, 7]) if kind != "mxfp4" else g.choice([8, 16, 24])
    elif bad == 3:
        d_out += g.choice([1, 4, 7])
    return T, d_in, d_out, r


def test_rows_plan_mirror_against_the_workspace_query():
    from sow_amd import _lib
    lib = _lib.load()
    g = random.Random(RP.SEED + 2)
    kinds = {"none": _lib.ACC_NONE, "dense": _lib.ACC_DENSE, "e4m3": _lib.ACC_DENSE_FP8, "mxfp4": _lib.ACC_DENSE_FP4}
    bad, refused, clamped = [], 0, 0
    for i in range(4000):
        kind = RP.KINDS[i % 4]
        T, d_in, d_out, r = _shape(g, kind, 64)
        dt = g.choice([_lib.BF16, _lib.F16]) | g.choice([0, _lib.PARAM_F32 | _lib.ACC_NATIVE])
        got, want = lib.sow_forward_skinny_rows_workspace_bytes(T, d_in, d_out, r, kinds[kind], dt), RP.rows_ws_bytes(T, d_in, d_out, r, kind)
        refused += want == 0
        clamped += want != 0 and T > 32 and RP.skinny_rows_plan(T, d_in, d_out, kind)[1] in (RP.KS_MAX48, RP.KS_MAX64)
        if got != want:
            bad.append((kind, T, d_in, d_out, r, got, want))
    assert not bad, bad[:5]
    assert refused >= 300 and clamped >= 100, (refused, clamped)
    # the low-rank kind, fp32 and fp32 factors without the native bit are refused
    assert lib.sow_forward_skinny_rows_workspace_bytes(48, 264, 520, 8, _lib.ACC_LOWRANK, _lib.BF16) == 0
    assert lib.sow_forward_skinny_rows_workspace_bytes(48, 264, 520, 8, _lib.ACC_DENSE, _lib.F32) == 0
    assert lib.sow_forward_skinny_rows_workspace_bytes(48, 264, 520, 8, _lib.ACC_DENSE, _lib.BF16 | _lib.PARAM_F32) == 0


def test_short_plan_mirrors_against_the_workspace_queries():
    """Both queries of the plain pair and both of the pair on codes, 3200 seeded shapes each; plan_ws(...).total is taken from
    sow_workspace_bytes.  A query of one family answers 0 for the kinds of the other, and all four for flagged dtypes."""
    from sow_amd import _lib
    lib = _lib.load()
    g = random.Random(RP.SEED + 3)
    kinds = {"dense": _lib.ACC_DENSE, "e4m3": _lib.ACC_DENSE_FP8, "mxfp4": _lib.ACC_DENSE_FP4}
    bad, refused, long_slabs = [], 0, 0
    for i in range(9600):
        kind = ("dense", "e4m3", "mxfp4")[i % 3]
        T, d_in, d_out, r = _shape(g, kind, 1024)
        dt = g.choice([_lib.BF16, _lib.F16])
        base = lib.sow_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_DENSE, dt)
        if kind == "dense":
            got = (lib.sow_forward_short_workspace_bytes(T, d_in, d_out, r, kinds[kind], dt), lib.sow_short_workspace_bytes(T, d_in, d_out, r, kinds[kind], dt))
            want = (RP.forward_short_ws_bytes(T, d_in, d_out, r), RP.short_ws_bytes(T, d_in, d_out, r, base))
            other = (lib.sow_forward_short_codes_workspace_bytes, lib.sow_short_codes_workspace_bytes)
        else:
            got = (lib.sow_forward_short_codes_workspace_bytes(T, d_in, d_out, r, kinds[kind], dt), lib.sow_short_codes_workspace_bytes(T, d_in, d_out, r, kinds[kind], dt))
            want = (RP.forward_short_codes_ws_bytes(T, d_in, d_out, r, kind), RP.short_codes_ws_bytes(T, d_in, d_out, r, kind, base))
            other = (lib.sow_forward_short_workspace_bytes, lib.sow_short_workspace_bytes)
        refused += want[0] == 0
        assert (want[0] == 0) == (want[1] == 0)
        if want[0]:
            long_slabs += RP.fwd_plan(kind, T, d_in, d_out)[1] > RP.KQ_FWD or RP.bwd_plan(T, d_in, d_out)[1] > RP.KQ_BWD
        if got != want:
            bad.append((kind, T, d_in, d_out, r, got, want))
        if i % 16 == 0:
            assert other[0](T, d_in, d_out, r, kinds[kind], dt) == 0 and other[1](T, d_in, d_out, r, kinds[kind], dt) == 0
            flagged = dt | g.choice([_lib.PARAM_F32, _lib.ACC_NATIVE, _lib.PARAM_F32 | _lib.ACC_NATIVE])
            q = (lib.sow_short_workspace_bytes, lib.sow_forward_short_workspace_bytes) if kind == "dense" else \
                (lib.sow_short_codes_workspace_bytes, lib.sow_forward_short_codes_workspace_bytes)
            assert q[0](T, d_in, d_out, r, kinds[kind], flagged) == 0 and q[1](T, d_in, d_out, r, kinds[kind], flagged) == 0
    assert not bad, bad[:5]
    assert refused >= 800 and long_slabs >= 500, (refused, long_slabs)
    # the two examples of the plan's notes
    assert RP.short_rows_plan(1024, 4232, 136, RP.KQ_FWD)[1] == 512 and RP.short_rows_plan(1024, 4104, 72, RP.KQ_BWD)[1] == 512


# ---- coverage: one assertion per class, counted over the drawn cases ------------------------------------------------------------------
def test_rows_coverage():
    rows = RP.plan().rows
    print("rows:", dict(collections.Counter(c.kind for c in rows)))
    assert [c.f32 for c in rows] == [j % 3 == 0 for j in range(len(rows))]
    assert {c.r for c in rows} >= set(FP.SK_R_EDGES) and sum(c.r % 2 for c in rows) * 3 >= len(rows)
    assert {RP.rank_tiles(c.r) for c in rows} == {1, 2, 3, 4}
    assert all(33 <= c.T <= 64 and 1 <= c.r <= 64 and c.d_in % FP.sk_step(c.kind) == 0 and c.d_out % 8 == 0 for c in rows)
    assert {c.s for c in rows} >= set(RP.SCALES) and any(c.bias for c in rows) and any(not c.bias for c in rows)
    for kind in RP.KINDS:
        mine = [c for c in rows if c.kind == kind]
        assert {c.T for c in mine} >= set(RP.ROWS_T_EDGES), kind
        assert {c.dtype for c in mine} == {"bf16", "f16"} and {c.f32 for c in mine} == {True, False}, kind
        low, high = [c for c in mine if c.T <= 48], [c for c in mine if c.T > 48]
        ks_low, ks_high = collections.Counter(c.plan()[1] for c in low), collections.Counter(c.plan()[1] for c in high)
        tails = collections.Counter(t for c in mine for t in c.tails())
        cols = collections.Counter(c.col() for c in mine)
        big = sum(c.plan()[0] > RP.SK_BS for c in mine)
        clamp = [c for c in high if RP.skinny_rows_plan(48, c.d_in, c.d_out, kind)[1] > RP.KS_MAX64]
        print(f"rows {kind}: KS at T <= 48 {dict(ks_low)}, at T > 48 {dict(ks_high)}, tails {dict(tails)}, columns {dict(cols)}, "
              f"S > 16: {big}, clamp binds: {len(clamp)}")
        assert clamp and all(c.plan()[1] == RP.KS_MAX64 for c in clamp), kind
        assert big >= 2, kind
        if kind == "none":      # (no accumulator: the slab lengths depend on d_in alone; the draw reaches the longest of either range)
            assert RP.KS_MAX48 in ks_low and RP.KS_MAX64 in ks_high
            continue
        assert set(ks_low) == set(range(128, RP.KS_MAX48 + 1, 128)), (kind, ks_low)
        assert set(ks_high) == set(range(128, RP.KS_MAX64 + 1, 128)), (kind, ks_high)
        assert all(n == 1 for ks, n in list(ks_low.items()) + list(ks_high.items()) if ks >= 256), (kind, ks_low, ks_high)
        assert all(tails[t] >= 1 for t in RP.FWD_TAILS), (kind, tails)
        assert all(">512" not in c.tails() for c in high)
        assert all(cols[k] >= 1 for k in RP.COLS), (kind, cols)


def _short_coverage(cases, kinds, tag):
    assert {c.r for c in cases} >= set(FP.SK_R_EDGES) and {RP.rank_tiles(c.r) for c in cases} == {1, 2, 3, 4}
    assert any(c.bias for c in cases) and any(not c.bias for c in cases) and {c.s for c in cases} <= set(RP.SCALES) and len({c.s for c in cases}) >= 2
    Ts = collections.Counter(c.T for c in cases)
    assert all(Ts[T] == 1 for T in RP.SHORT_T_FIXED), Ts
    blocks, last = collections.Counter(RP.block_class(c.T) for c in cases), collections.Counter(RP.last_rows(c.T) for c in cases)
    print(f"{tag}: {len(cases)} cases; row blocks {dict(blocks)}; rows of the last block {dict(sorted(last.items()))}")
    assert all(blocks[b] >= 2 for b in RP.BLOCKS), blocks
    assert all(last[n] >= 2 for n in RP.LAST_ROWS), last
    fwd = collections.Counter((c.fwd()[1], t) for c in cases for t in c.fwd_tails())
    bwd = collections.Counter((c.bwd()[1], c.bwd_tail()) for c in cases)
    print(f"{tag}: forward (KS, tail) {dict(sorted(fwd.items()))}")
    print(f"{tag}: data gradient (KS, tail) {dict(sorted(bwd.items(), key=str))}")
    assert all(fwd[(ks, t)] >= 1 for ks in (128, 256, 384, 512) for t in RP.FWD_TAILS[:3]), fwd
    assert all(bwd[(ks, t)] >= 1 for ks in (256, 512) for t in RP.BWD_TAILS), bwd
    assert sum(c.fwd()[0] > RP.SK_BS for c in cases) >= 1 and sum(c.bwd()[0] > RP.SK_BS for c in cases) >= 1
    for kind in kinds:
        mine = [c for c in cases if c.kind == kind]
        assert {c.dtype for c in mine} == {"bf16", "f16"}, kind
        cf, cb = collections.Counter(c.fwd_col() for c in mine), collections.Counter(c.bwd_col() for c in mine)
        print(f"{tag} {kind}: {len(mine)} cases; forward columns {dict(cf)}; data-gradient columns {dict(cb)}")
        assert all(cf[k] >= 1 for k in RP.COLS), (kind, cf)
        assert all(cb[k] >= 1 for k in (RP.COLS_FP4_BWD if kind == "mxfp4" else RP.COLS)), (kind, cb)
        assert {c.fwd()[1] for c in mine} == {128, 256, 384, 512} and {c.bwd()[1] for c in mine} == {256, 512}, kind
        assert {t for c in mine for t in c.fwd_tails()} >= set(RP.FWD_TAILS[:3]) and {c.bwd_tail() for c in mine} >= set(RP.BWD_TAILS), kind
        assert all(c.d_in % FP.sk_step(kind) == 0 and c.d_out % 8 == 0 and 1 <= c.T <= RP.SHORT_MAX for c in mine)


def test_short_coverage():
    _short_coverage(RP.plan().short, ("dense",), "short")


def test_short_codes_coverage():
    cases = RP.plan().short_codes
    _short_coverage(cases, RP.CODES, "short_codes")
    assert {c.d_in % 64 for c in cases if c.kind == "mxfp4"} == {0, 32}


def test_short_groups_coverage():
    gs = RP.plan().short_groups
    assert len(gs) == 8 and [g.kind for g in gs].count("dense") == 4 and [g.kind for g in gs].count("e4m3") == 2 and [g.kind for g in gs].count("mxfp4") == 2
    for kinds in (("dense",), RP.CODES):
        mine = [g for g in gs if g.kind in kinds]
        assert sorted(len(g.layers) for g in mine) == [2, 3, 5, 16]
        assert {g.pairs() for g in mine} >= {2, 3}
        # a cut inside a middle layer: neither the first nor the last of the call
        assert any(0 < i < len(g.layers) - 1 for g in mine for i in g.cuts_inside())
        idle = [g for g in mine if any(c.T == 0 for c in g.layers)]
        assert len(idle) == 1 and all(0 < i < len(g.layers) - 1 and g.layers[i - 1].T and g.layers[i + 1].T
                                      for g in idle for i, c in enumerate(g.layers) if c.T == 0)
        shared = [g for g in mine if g.share_w]
        assert len(shared) == 1 and len(shared[0].layers) == 2 and len({(c.d_in, c.d_out) for c in shared[0].layers}) == 1
    assert {g.dtype for g in gs} == {"bf16", "f16"}
    for g in gs:
        assert len(g.layers) <= RP.SK_MAXL and all(c.kind == g.kind and c.dtype == g.dtype for c in g.layers)
        assert all(c.d_in % FP.sk_step(g.kind) == 0 and c.d_out % 8 == 0 and 0 <= c.T <= RP.SHORT_MAX for c in g.layers)
        print(g.name, "entries", g.entries(), "pairs", g.pairs(), "cuts inside layers", g.cuts_inside())


# ---- reference cost ---------------------------------------------------------------------------------------------------------------------------
def test_reference_cost_under_the_old_sweep():
    fp = FP.plan()
    old = fp.layers + fp.shared + fp.gemms + [m for g in fp.groups for m in g.layers] + fp.skinny + fp.skinny_groups + fp.fused + fp.deep + fp.shared_acc
    cap = max(FP.ref_cost(c) for c in old)
    p = RP.plan()
    for fam in ("rows", "short", "short_codes", "short_groups"):
        worst = max(getattr(p, fam), key=RP.ref_cost)
        print(f"{fam}: worst float64 reference {RP.ref_cost(worst):.3g} multiply-adds ({worst.name}); the old sweep's largest {cap:.3g}")
        assert RP.ref_cost(worst) <= cap


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------
def _rows_layer(c):
    """test_gpu_skinny_rows._layer of a planned case.  A code matrix past CPU_CODES_MAX is quantised on the GPU there; here the
    tie-clearing step runs on the unquantised W (W enters it through the comparator's bound alone)."""
    import test_gpu_skinny_rows as RW
    fmt = FMT[c.kind] if c.kind not in RP.CODES or c.d_in * c.d_out <= CPU_CODES_MAX else "dense"
    return RW._layer(fmt, RW.DT[c.dtype], c.T, c.d_in, c.d_out, c.r, c.bias, c.s, seed=c.seed)


def _short_layer(c):
    import test_gpu_short_codes as C
    import test_gpu_short_rows as P
    if c.kind == "dense" or c.d_in * c.d_out > CPU_CODES_MAX:
        return P._operands(c.dtype, c.T, c.d_in, c.d_out, c.r, c.bias, c.s, c.seed)
    return C._operands(FMT[c.kind], c.dtype, c.T, c.d_in, c.d_out, c.r, c.bias, c.s, c.seed)


def test_rows_operands_clear_their_ties():
    """Every rows case: the tie-clearing step of _layer ends, each element of A moved at most once by one ulp, at most 2 % of them,
    and a second pass over the finished operands moves nothing."""
    import skinny_sweep as SW
    import test_gpu_skinny as S
    total = 0
    for c in RP.plan().rows:
        d = _rows_layer(c)
        dtype = SW.DT[c.dtype]
        A0 = S._gauss(dtype, c.T, c.d_in, c.d_out, c.r, c.bias, "dense" if c.kind != "none" else "none", seed=c.seed)["A"]
        delta = d["A"].view(torch.int16).int() - A0.view(torch.int16).int()
        assert set(delta.unique().tolist()) <= {0, 1} and int((delta != 0).sum()) <= max(d["A"].numel() // 50, 8), c.name
        _, again = SW.off_ties(dtype, {k: v for k, v in d.items() if k not in ("q", "e", "fmt")})
        assert again == 0, f"{c.name}: {again} projections still lie on a rounding tie"
        assert (d["W"] is None) == (c.kind == "none")
        total += int((delta != 0).sum())
    print(f"rows: {total} elements of A moved off rounding ties")


def test_short_operands_clear_their_ties():
    """Every short case, every case on codes and every layer of the grouped calls through _operands, which asserts that a second
    pass moves nothing; TIES_MAX_T is what test_gpu_short_rows sets."""
    import test_gpu_short_rows as P
    assert P.TIES_MAX_T == 129
    p = RP.plan()
    n = 0
    for c in p.short + p.short_codes + [m for m in _members(p) if m.T]:
        case, d = _short_layer(c)
        assert d["x"].shape == (c.T, c.d_in) and d["W"].shape == (c.d_in, c.d_out) and d["B"].shape == (c.r, c.d_out)
        assert (d.get("q") is not None) == (c.kind in RP.CODES and c.d_in * c.d_out <= CPU_CODES_MAX)
        n += 1
    print(f"short: {n} layers built")


# ---- the comparators see each class --------------------------------------------------------------------------------------------------------
def _smallest(cases, pred):
    mine = [c for c in cases if pred(c)]
    assert mine, "no planned case in the class"
    return min(mine, key=RP.ref_cost)


def _rolled(y, lo):
    """y with the columns from lo on shifted by one."""
    y = y.clone()
    y[:, lo:] = torch.roll(y[:, lo:], 1, dims=1)
    return y


def _rows_y(dtype, d):
    import test_gpu_skinny as S
    return rne(S._reference(dtype, {k: v for k, v in d.items() if k not in ("q", "e", "fmt")})[0], dtype).to(dtype)


def _rows_rejects(c, what, y_bad):
    """The comparator of the rows cases passes the float64 result of c rounded once and rejects y_bad(operands, that result)."""
    import test_gpu_skinny_rows as RW
    dtype = RW.DT[c.dtype]
    d = _rows_layer(c)
    y = _rows_y(dtype, d)
    RW._check(f"{c.name} exact", dtype, d, y)
    with pytest.raises(AssertionError):
        RW._check(f"{c.name} without {what}", dtype, d, y_bad(d, y))
    print(f"rows: a result without {what} is rejected ({c.name})")


def _cut_k(d, k0, k1):
    """The operands with the rows k0 .. k1 of the forward's contraction left out (zeros in x)."""
    x = d["x"].clone()
    x[:, k0:k1] = 0
    return dict(x=x)


def test_rows_comparator_rejects_each_class_left_out():
    rows = RP.plan().rows
    for t in RP.FWD_TAILS:          # the last k-group of the contraction
        c = _smallest(rows, lambda c: t in c.tails())
        g = FP.sk_step(c.kind)
        _rows_rejects(c, f"the last k-group (tail class {t})", y_bad=lambda d, y, c=c, g=g: _rows_y(_dt(c), dict(d, **_cut_k(d, c.d_in - g, c.d_in))))
    c = _smallest(rows, lambda c: c.plan()[0] > RP.SK_BS)   # every slab past the 16th
    _rows_rejects(c, "the slabs past the 16th", y_bad=lambda d, y, c=c: _rows_y(_dt(c), dict(d, **_cut_k(d, RP.SK_BS * c.plan()[1], c.d_in))))
    for n in (1, 2, 3, 4):          # the columns of the last rank tile
        c = _smallest(rows, lambda c: RP.rank_tiles(c.r) == n)

        def without_tile(d, y, c=c, n=n):
            B = d["B"].clone()
            B[16 * (n - 1):] = 0
            return _rows_y(_dt(c), dict(d, B=B))
        _rows_rejects(c, f"the last of {n} rank tiles", y_bad=without_tile)
    for k in RP.COLS:               # the columns of the last column range shifted by one
        c = _smallest(rows, lambda c: c.col() == k and c.kind != "none")
        cn = FP.sk_cn(c.kind)
        _rows_rejects(c, f"the last column range in place (column class {k})", y_bad=lambda d, y, c=c, cn=cn: _rolled(y, (RP.cdiv(c.d_out, cn) - 1) * cn))
    for T in RP.ROWS_T_EDGES:       # the last row, and from 49 rows on the fourth row tile, as the zero tile gives them
        c = _smallest(rows, lambda c: c.T == T)

        def zero_rows(d, y, c=c, t0=None):
            x = d["x"].clone()
            x[(c.T - 1 if t0 is None else t0):] = 0
            return _rows_y(_dt(c), dict(d, x=x))
        _rows_rejects(c, f"row {T - 1} (T = {T})", y_bad=zero_rows)
        if T > 48:
            _rows_rejects(c, f"the rows from 48 on (T = {T})", y_bad=lambda d, y, c=c, f=zero_rows: f(d, y, c, 48))


def _dt(c):
    return {"bf16": torch.bfloat16, "f16": torch.float16}[c.dtype]


def _short_exact(case, d, fwd=None, bwd=None):
    """The outputs of a short case from float64, every stored value rounded once as the contract says (h and dh rounded before
    they are used).  fwd / bwd: operands put in place of d's for the forward (y, h_save) / for dX alone."""
    dt, s, r = case.dtype, case.s, case.r
    f = {k: to64(v) for k, v in dict(d, **(fwd or {})).items() if isinstance(v, torch.Tensor)}
    b = {k: to64(v) for k, v in dict(d, **(bwd or {})).items() if isinstance(v, torch.Tensor)}
    q = {k: to64(v) for k, v in d.items() if isinstance(v, torch.Tensor)}
    h = rne(s * (f["x"] @ f["A"]), dt)
    hs = torch.zeros(case.T, 64, dtype=torch.float64)
    hs[:, :r] = h
    if r <= 63:
        hs[:, 63] = 1.0
    y = f["x"] @ f["W"] + h @ f["B"] + (f["bias"] if "bias" in f else 0)
    h0 = rne(s * (q["x"] @ q["A"]), dt)
    dh = rne(s * (q["dy"] @ q["B"].t()), dt)
    dhb = rne(s * (b["dy"] @ b["B"].t()), dt)
    out = dict(y=y, h=hs, dx=b["dy"] @ b["W"].t() + dhb @ b["A"].t(), dA=q["x"].t() @ dh, dB=h0.t() @ q["dy"], dbias=q["dy"].sum(0) if case.bias else None)
    return {k: (None if v is None else rne(v, dt).to(dt)) for k, v in out.items()}


def _short_check(c, case, d, out):
    import test_gpu_elementwise as E
    E._check(case, {k: v for k, v in d.items() if k not in ("q", "e", "fmt")}, out)


def _short_rejects(c, what, make):
    """test_gpu_elementwise._check (the comparator of both short families, on W^ for codes) passes the float64 outputs of c and
    rejects what `make(case, d, exact outputs)` returns."""
    case, d = _short_layer(c)
    good = _short_exact(case, d)
    _short_check(c, case, d, good)
    with pytest.raises(AssertionError):
        _short_check(c, case, d, dict(good, **make(case, d, good)))
    print(f"{c.kind}: a result without {what} is rejected ({c.name})")


def _zero(t, rows=None, cols=None):
    t = t.clone()
    if rows is not None:
        t[rows[0]:rows[1]] = 0
    if cols is not None:
        t[:, cols[0]:cols[1]] = 0
    return t


def _short_comparator(cases):
    def sub(out, *keys):
        return {k: out[k] for k in keys}

    for t in RP.FWD_TAILS[:3]:      # the last k-group of the forward's contraction
        c = _smallest(cases, lambda c: t in c.fwd_tails())
        g = FP.sk_step(c.kind)
        _short_rejects(c, f"the last k-group of d_in (tail class {t})",
                       lambda case, d, good, c=c, g=g: sub(_short_exact(case, d, fwd=dict(x=_zero(d["x"], cols=(c.d_in - g, c.d_in)))), "y", "h"))
    for t in RP.BWD_TAILS:          # ... of the data gradient's
        c = _smallest(cases, lambda c: c.bwd_tail() == t)
        _short_rejects(c, f"the last k-group of d_out (tail class {t})",
                       lambda case, d, good, c=c: sub(_short_exact(case, d, bwd=dict(dy=_zero(d["dy"], cols=(c.d_out - 8, c.d_out)))), "dx"))
    c = _smallest(cases, lambda c: c.fwd()[0] > RP.SK_BS)
    _short_rejects(c, "the forward's slabs past the 16th",
                   lambda case, d, good, c=c: sub(_short_exact(case, d, fwd=dict(x=_zero(d["x"], cols=(RP.SK_BS * c.fwd()[1], c.d_in)))), "y", "h"))
    c = _smallest(cases, lambda c: c.bwd()[0] > RP.SK_BS)
    _short_rejects(c, "the data gradient's slabs past the 16th",
                   lambda case, d, good, c=c: sub(_short_exact(case, d, bwd=dict(dy=_zero(d["dy"], cols=(RP.SK_BS * c.bwd()[1], c.d_out)))), "dx"))
    for n in (1, 2, 3, 4):          # the columns of the last rank tile: of h in y, of dh in dX
        c = _smallest(cases, lambda c: RP.rank_tiles(c.r) == n)
        _short_rejects(c, f"the last of {n} rank tiles in y",
                       lambda case, d, good, n=n: sub(_short_exact(case, d, fwd=dict(B=_zero(d["B"], rows=(16 * (n - 1), 64)))), "y"))
        _short_rejects(c, f"the last of {n} rank tiles in dX",
                       lambda case, d, good, n=n: sub(_short_exact(case, d, bwd=dict(A=_zero(d["A"], cols=(16 * (n - 1), 64)))), "dx"))
    for kind in sorted({c.kind for c in cases}):
        cn = FP.sk_cn(kind)
        for k in RP.COLS:           # the last column range shifted by one
            c = _smallest(cases, lambda c: c.kind == kind and c.fwd_col() == k)
            _short_rejects(c, f"the forward's last column range in place (column class {k})",
                           lambda case, d, good, c=c: dict(y=_rolled(good["y"], (RP.cdiv(c.d_out, cn) - 1) * cn)))
        for k in (RP.COLS_FP4_BWD if kind == "mxfp4" else RP.COLS):
            c = _smallest(cases, lambda c: c.kind == kind and c.bwd_col() == k)
            _short_rejects(c, f"the data gradient's last column range in place (column class {k})",
                           lambda case, d, good, c=c: dict(dx=_rolled(good["dx"], (RP.cdiv(c.d_in, 64) - 1) * 64 if kind != "mxfp4" else c.d_in - 32)))
    for n in RP.LAST_ROWS:          # the last row of the last block, and from 49 rows on its fourth row tile, as the zero tile gives them
        c = _smallest(cases, lambda c: RP.last_rows(c.T) == n)
        for t0 in (c.T - 1,) + ((c.T - n + 48,) if n > 48 else ()):
            _short_rejects(c, f"the rows from {t0 - (c.T - n)} on of a last block of {n}",
                           lambda case, d, good, t0=t0: sub(_short_exact(case, d, fwd=dict(x=_zero(d["x"], rows=(t0, case.T))),
                                                                         bwd=dict(dy=_zero(d["dy"], rows=(t0, case.T)))), "y", "h", "dx"))


def test_short_comparator_rejects_each_class_left_out():
    _short_comparator(RP.plan().short)


def test_short_codes_comparator_rejects_each_class_left_out():
    _short_comparator(RP.plan().short_codes)
