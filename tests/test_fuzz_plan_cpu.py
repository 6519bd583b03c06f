"""The generator of the element-wise random sweep (tests/fuzz_plan.py), tested on the CPU (no `gpu` mark): deterministic,
the stratum counts met, the named edges drawn, every case's float64 reference under the cost cap; for the second stream also
the first stream left unchanged, the mirrors of the C planning functions against the library, and the skinny operands."""
import collections
import hashlib
import os
import random

import fuzz_plan as FP


def test_plan_is_deterministic():
    a, b = FP.plan(), FP.plan()
    assert a == b
    assert FP.plan(FP.SEED + 1) != a


def test_stratum_counts():
    p = FP.plan()
    by = collections.Counter(c.stratum for c in p.layers)
    print(dict(by))
    assert 100 <= len(p.layers) <= 140
    assert by["chain2"] + by["short"] + by["gemm4h"] + by["gemm2h"] + by["dense_short"] + by["dense_long"] + by["lowrank"] >= 30
    assert by["wide"] >= 10 and by["ragged"] >= 14
    assert by["chain3f"] + by["chain2f"] + by["tn_f32"] + by["gemm_x3"] >= 20
    assert by["generic"] >= 12
    assert 10 <= len(p.groups) <= 14 and 10 <= len(p.shared) <= 14 and 40 <= len(p.gemms) <= 56
    assert sum(g.deferred for g in p.groups) >= 4 and sum(g.rows for g in p.groups) >= 3
    dts = collections.Counter(c.dtype for c in p.layers)
    assert min(dts.values()) >= 20, dts
    # per-case settings: bias, scales, grad_beta, h_save = NULL, a retained-kernel switch for about a fifth
    assert {c.s for c in p.layers} >= {1.0, 0.5, 2.0} and any(c.s == 1.0 / c.r and c.r > 2 for c in p.layers)
    assert {c.grad_beta for c in p.layers} == {0.0, 0.5, 1.0}
    assert any(c.bias for c in p.layers) and any(not c.bias for c in p.layers)
    assert sum(not c.save_h for c in p.layers) >= 3
    sw = [c for c in p.layers if c.switches]
    assert 0.12 <= len(sw) / len(p.layers) <= 0.3
    assert {k for c in sw for k in c.switches} == set(FP.LAYER_SWITCHES)
    for c in p.layers:
        assert c.family and c.y_rounds in ("once", "twice") and c.dx_rounds in ("once", "twice")
        assert f"T{c.T}" in c.name and f"{c.d_in}x{c.d_out}" in c.name and f"r{c.r}" in c.name


def test_named_edges_are_drawn():
    p = FP.plan()
    edges = collections.Counter(e for c in p.layers for e in c.edges)
    # chain3f at d_out % 4 != 0 (its forward) and d_in % 4 != 0 (its backward), T >= 8192
    c3f = [c for c in p.layers if c.stratum == "chain3f"]
    assert all(c.T >= 8192 for c in c3f)
    assert sum(c.d_out % 4 != 0 and c.d_in % 4 == 0 for c in c3f) >= 3
    assert sum(c.d_in % 4 != 0 and c.d_out % 4 == 0 for c in c3f) >= 3
    # every ragged residue 1 .. 7 on either side
    rag = [c for c in p.layers if c.stratum == "ragged"]
    assert {c.d_in % 8 for c in rag} >= set(range(1, 8)) and {c.d_out % 8 for c in rag} >= set(range(1, 8))
    assert all(c.r > 64 and c.r % 2 == 0 for c in rag)
    # T at slab boundaries of tnw_pick_slabs, below 64 and below 256
    wide = [c for c in p.layers if c.stratum in ("wide", "ragged")]
    for c in wide:
        ns, ln = FP.tnw_pick_slabs(c.T, c.d_in, c.d_out)
        if "slab+1" in c.edges:
            assert c.T % ln == 1 and ns >= 2, (c.name, ns, ln)
        if "slab-1" in c.edges:
            assert c.T % ln == ln - 1 and ns >= 2, (c.name, ns, ln)
    for e in ("slab+1", "slab-1", "T<64", "T<256"):
        assert edges[e] >= 4, (e, edges[e])
    assert {c.r for c in wide if c.r > 200} and all(64 < c.r <= 256 for c in wide)
    # generic edges
    gen = [c for c in p.layers if c.stratum == "generic"]
    assert any(c.r in (1, 2, 3) for c in gen) and any(c.r % 2 for c in gen) and any(c.T < 64 for c in gen)
    assert any(c.misalign for c in gen) and any(c.d_in % 8 for c in gen)
    # strided GEMM operands: ld > row in every operand, every transpose combination in every dtype
    gm = p.gemms
    rowa = lambda g: g.M if g.trans_a else g.K   # noqa: E731
    rowb = lambda g: g.K if g.trans_b else g.N   # noqa: E731
    assert all(g.ldc > g.N for g in gm)
    assert sum(g.lda > rowa(g) for g in gm) >= 20 and sum(g.ldb > rowb(g) for g in gm) >= 20
    assert {(g.dtype, g.trans_a, g.trans_b) for g in gm} >= {(d, a, b) for d in ("bf16", "f16", "f32") for a in (0, 1)
                                                             for b in (0, 1)}
    assert {g.alpha for g in gm} == {1.0, 0.5, -2.0} and {g.beta for g in gm} == {0.0, 0.5, 1.0}
    assert any(g.use_ws for g in gm) and any(g.K >= 6144 and not g.use_ws for g in gm)


def test_families_are_targeted():
    p = FP.plan()
    fams = collections.Counter([c.family for c in p.layers] + [g.family for g in p.gemms])
    print(dict(fams))
    for f in ("chain2_kernel", "chain2_f16_kernel", "h_reduce_kernel", "chain_kernel", "chain_wide_kernel", "chain3f_kernel",
              "chain2f_kernel", "tn_partial_f32_quad_kernel", "gemm4_kernel", "gemm4_f16_kernel", "gemm2h_kernel",
              "gemm2_kernel", "gemm3s_kernel", "gemm_x3_kernel", "gemm_kernel", "gemm4_splitk_reduce_kernel"):
        assert fams[f] >= 3, (f, fams[f])


def test_reference_cost_under_the_cap():
    p = FP.plan()
    cases = p.layers + p.shared + p.gemms + [m for g in p.groups for m in g.layers]
    worst = max(cases, key=FP.ref_cost)
    print(f"worst float64 reference {FP.ref_cost(worst):.3g} multiply-adds ({worst.name}); cap {FP.REF_COST_CAP:.3g}")
    assert FP.ref_cost(worst) <= FP.REF_COST_CAP


# ---- the second stream: skinny forward, fused accumulator passes, shared low-rank siblings, dense ragged layers ----------------
OLD_NAMES_SHA256 = "fa084a260e2639a674360203a3ad4f2b56926d2c3a111429ff9989768e2fcf3d"


def _second(p):
    return p.skinny + p.skinny_groups + p.fused + p.deep + p.shared_acc + p.layers[FP.N_FIRST_LAYERS:]


def test_first_stream_is_unchanged():
    """The ordered names (each names its shape and settings) of the layers, groups, shared sets and GEMMs drawn before the
    second stream existed, as a digest taken at the commit before it."""
    p = FP.plan()
    names = [c.name for c in p.layers[:FP.N_FIRST_LAYERS] + p.groups + p.shared + p.gemms]
    assert len(names) == 175 and all(c.stratum == "ragged" and c.acc == "dense" for c in p.layers[FP.N_FIRST_LAYERS:])
    assert hashlib.sha256("\n".join(names).encode()).hexdigest() == OLD_NAMES_SHA256


def test_second_stream_is_deterministic():
    a, b, other = FP.plan(), FP.plan(), FP.plan(FP.SEED + 1)
    assert _second(a) == _second(b)
    for k in ("skinny", "skinny_groups", "fused", "deep", "shared_acc"):
        assert getattr(a, k) != getattr(other, k), k
    names = [c.name for c in _second(a)] + [m.name for g in a.skinny_groups for m in g.layers]
    assert len(set(names)) == len(names)


def test_skinny_cases():
    p = FP.plan()
    sk = p.skinny
    assert collections.Counter(c.kind for c in sk) == {"dense": 16, "e4m3": 16, "mxfp4": 16, "none": 8}
    for kind in FP.SK_KINDS:
        mine = [c for c in sk if c.kind == kind]
        assert {c.dtype for c in mine} == {"bf16", "f16"}
        ks = collections.Counter(FP.skinny_plan(c.d_in, c.d_out, kind)[1] for c in mine)
        if kind == "none":
            assert set(ks) == {128, 256, 384}
            assert all(c.d_in * c.d_out <= 1.5 * 4104 * 8 for c in mine if FP.skinny_plan(c.d_in, c.d_out, kind)[1] == 256)
            assert all(c.d_in * c.d_out <= 1.5 * 8200 * 8 for c in mine if FP.skinny_plan(c.d_in, c.d_out, kind)[1] == 384)
            continue
        # every slab length; one case at each from 512 up (the issue's "768 up" would leave 512 and 640 unreached), the rest small
        assert set(ks) == set(FP.SK_KS) and all(ks[k] == 1 for k in FP.SK_KS if k >= 512), ks
        tails = collections.Counter(t for c in mine for t in FP.skinny_tail_classes(c.d_in, c.d_out, kind))
        assert all(tails[t] >= 3 for t in FP.SK_TAILS), (kind, tails)
        for c in mine:
            k = FP.skinny_plan(c.d_in, c.d_out, kind)[1]
            assert c.d_in * c.d_out <= FP.sk_w_cap(kind, k), c.name
        # the largest: inside 1.5 x the smallest W of 1024-row slabs (7176 -> 4040; 8096 -> 7176 for the code formats)
        assert max(c.d_in * c.d_out for c in mine) <= 1.5 * (7176 * 4040 if kind == "dense" else 8096 * 7176)
    for c in sk:
        assert c.d_in % FP.sk_step(c.kind) == 0 and c.d_out % 8 == 0 and 1 <= c.r <= 64 and 1 <= c.T <= 32
        assert c.s in (1.0, 0.5, 0.25, 1.0 / c.r)
        assert f"T{c.T}" in c.name and f"{c.d_in}x{c.d_out}" in c.name and f"r{c.r}" in c.name
    for cn in (64, 128):
        cols = collections.Counter(FP.skinny_col_class(c.d_out, c.kind) for c in sk if FP.sk_cn(c.kind) == cn)
        assert all(cols[k] >= 3 for k in FP.SK_COLS), (cn, cols)
    assert {c.r for c in sk} >= set(FP.SK_R_EDGES) and sum(c.r % 2 for c in sk) >= 20
    assert {c.T for c in sk} >= set(FP.SK_T_EDGES)
    assert sum(FP.skinny_plan(c.d_in, c.d_out, c.kind)[0] > 16 for c in sk) >= 4
    assert [c.f32 for c in sk] == [i % 3 == 0 for i in range(len(sk))]
    assert 0.4 <= sum(c.bias for c in sk) / len(sk) <= 0.8 and {c.s for c in sk} >= {1.0, 0.5, 0.25}
    # SOW_ACC_NONE at slabs longer than 128 rows, and fp32 factors over every kind
    assert {c.kind for c in sk if c.f32} == set(FP.SK_KINDS)


def test_skinny_groups():
    gs = FP.plan().skinny_groups
    assert len(gs) == 8 and all(len(g.layers) in (2, 3, 4, 7, 16) for g in gs) and sum(len(g.layers) == 16 for g in gs) == 1
    assert sum(g.x_shared for g in gs) == 2 and sum(g.f32 for g in gs) == 2
    assert {g.kind for g in gs} == set(FP.SK_KINDS) and {g.dtype for g in gs} == {"bf16", "f16"}
    for g in gs:
        kinds = [c.kind for c in g.layers]
        assert set(kinds) <= {g.kind, "none"} and all(c.dtype == g.dtype and c.f32 == g.f32 for c in g.layers)
        if g.kind != "none":
            assert 1 <= kinds.count("none") <= 2 and kinds.count(g.kind) >= 1
        for c in g.layers:
            assert c.d_in * c.d_out <= 1 << 20 and c.d_in % FP.sk_step(c.kind) == 0 and c.d_out % 8 == 0
        if g.x_shared:
            assert len({(c.T, c.d_in) for c in g.layers}) == 1
        if g.f32:
            assert len({c.s for c in g.layers}) == 1
    free = [g for g in gs if not g.x_shared]
    # drawn per layer: token counts on both sides of the second row tile and slab lengths that differ inside a call
    assert sum(len({c.T > 16 for c in g.layers}) == 2 for g in free) >= 3
    assert sum(len({FP.skinny_plan(c.d_in, c.d_out, c.kind)[1] for c in g.layers}) >= 2 for g in free) >= 3


def test_fused_and_deep_cases():
    p = FP.plan()
    assert len(p.fused) == 16 and len(p.deep) == 16
    for cs, deep in ((p.fused, False), (p.deep, True)):
        for c in cs:
            assert c.deep is deep and c.r % 2 == 0 and c.r_acc % 2 == 0 and 2 <= c.r <= 64
            assert c.d_in % 8 == 0 and c.d_out % 8 == 0 and 8 <= c.d_in <= 600 and 8 <= c.d_out <= 600
            assert FP.fused_acc_shape_ok(c.r, c.r_acc, c.d_in, c.d_out, c.dtype) is not deep
            assert FP.deep_acc_shape_ok(c.r, c.r_acc, c.d_in, c.d_out, c.dtype) is deep
            assert c.T <= 63 or 1000 <= c.T <= 4200 or any(abs(c.T - 64 * k) <= 1 for k in range(1, 7)), c.name
        assert {c.dtype for c in cs} == {"bf16", "f16"} and sum(c.group for c in cs) == 4
        assert sum(1000 <= c.T <= 4200 for c in cs) == 1 and any(c.T <= 63 for c in cs) and any(c.T % 64 == 0 for c in cs)
        assert any(not c.save_h for c in cs) and any(c.bias for c in cs) and any(not c.bias for c in cs)
        assert len({c.s for c in cs}) >= 3
    assert {FP.r_pad(c.r + c.r_acc) for c in p.fused} == {64, 128, 192, 256}
    assert {(c.r + c.r_acc) % 64 for c in p.fused} >= {0, 2, 62}
    assert {FP.r_pad(c.r + c.r_acc) for c in p.deep} == set(range(320, 961, 64))
    assert all(258 <= c.r + c.r_acc <= 960 for c in p.deep)
    assert sum(c.r_acc // 256 != (c.r_acc + c.r - 1) // 256 and c.r_acc % 256 != 0 for c in p.deep) >= 3    # live columns on both sides
    assert sum(c.r == 64 for c in p.deep) >= 2


def test_shared_acc_sets():
    sets = FP.plan().shared_acc
    assert len(sets) == 8 and sum(s.dtype == "f16" for s in sets) == 2 and {s.grad_beta for s in sets} <= {0.0, 0.5, 1.0}
    assert len({s.grad_beta for s in sets}) >= 2
    for s in sets:
        assert 1 <= len(s.sibs) <= 4 and 8193 <= s.T <= 8800 and s.d_in % 8 == 0 and 8 <= s.d_in <= 520
        assert all(sb.d_out % 8 == 0 and 24 <= sb.d_out <= 520 for sb in s.sibs)
        assert all(FP.fused_acc_shape_ok(sb.r, sb.r_acc, s.d_in, sb.d_out, s.dtype) for sb in s.sibs)
        assert FP.shared_acc_lds_ok([sb.r + sb.r_acc for sb in s.sibs])
    lds = [FP.shared_acc_lds_bytes([sb.r + sb.r_acc for sb in s.sibs]) for s in sets]
    assert lds.count(160 * 1024) >= 1 and sum(len(s.sibs) == 4 for s in sets) >= 1
    assert len({len(s.sibs) for s in sets}) >= 3


def test_ragged_dense_layers():
    rd = FP.plan().layers[FP.N_FIRST_LAYERS:]
    assert len(rd) == 8 and collections.Counter(c.dtype for c in rd) == {"bf16": 4, "f16": 4}
    assert sum(c.d_in % 8 != 0 and c.d_out % 8 == 0 for c in rd) == 4 and sum(c.d_out % 8 != 0 and c.d_in % 8 == 0 for c in rd) == 4
    for c in rd:
        assert 64 < c.r <= 256 and c.r % 2 == 0 and c.acc == "dense" and c.y_rounds == c.dx_rounds == "twice" and c.save_h
    assert [c.family for c in rd].count("gemm_rag_kernel") == 7
    assert [(c.family, c.switches) for c in rd if c.switches] == [("gemm_kernel", {"NO_RAGGED_GEMM": 1})]


def test_second_stream_families_are_targeted():
    """What test_zz_fuzz_coverage will count: >= 3 planned cases per family of the second stream."""
    p = FP.plan()
    sk = p.skinny + [m for g in p.skinny_groups for m in g.layers]
    n = {"skinny_a_kernel[plain]": sum(c.kind in ("dense", "none") for c in p.skinny),
         "skinny_a_kernel[e4m3]": sum(c.kind == "e4m3" for c in p.skinny), "skinny_a_kernel[mxfp4]": sum(c.kind == "mxfp4" for c in p.skinny),
         "skinny_a_kernel[fp32-factors]": sum(c.f32 for c in p.skinny), "skinny_b_kernel": len(sk),
         "chain_wide_acc_kernel": len(p.fused), "chain_deep_acc_kernel": len(p.deep), "chain_shared_acc_kernel": len(p.shared_acc),
         "gemm_rag_kernel": sum(c.family == "gemm_rag_kernel" for c in p.layers)}
    assert set(n) == set(FP.FAMILIES_SECOND) and FP.FAMILIES == FP.FAMILIES_FIRST + FP.FAMILIES_SECOND
    assert all(v >= 3 for v in n.values()), n


def test_second_stream_reference_cost_under_the_cap():
    p = FP.plan()
    cases = _second(p)
    worst = max(cases, key=FP.ref_cost)
    print(f"worst float64 reference {FP.ref_cost(worst):.3g} multiply-adds ({worst.name}); cap {FP.REF_COST_CAP:.3g}")
    assert FP.ref_cost(worst) <= FP.REF_COST_CAP
    big = max(p.skinny, key=FP.ref_cost)
    print(f"largest skinny reference {FP.ref_cost(big):.3g} multiply-adds ({big.name})")
    assert FP.ref_cost(big) <= 4e9


# ---- the mirrors against the library ---------------------------------------------------------------------------------------------
def test_skinny_plan_mirror_against_the_workspace_queries():
    """fuzz_plan.skinny_ws_bytes against the three workspace queries over 3000 seeded shapes of all four kinds (a slab count
    or a slab length that differed would show: the query is 256 + al256(S T d_out 4) + al256(S T 64 4)), fp32 factors included."""
    from sow_amd import _lib
    lib = _lib.load()
    g = random.Random(FP.SEED + 2)
    kinds = {"none": _lib.ACC_NONE, "dense": _lib.ACC_DENSE}
    bad = []
    for i in range(3000):
        kind = FP.SK_KINDS[i % 4]
        step = FP.sk_step(kind)
        T, r = g.randint(1, 32), g.randint(1, 64)
        d_out = 8 * g.randint(1, g.choice([16, 128, 1200]))
        d_in = step * g.randint(1, g.choice([64, 512, 16384 // step * 2]))
        dt = g.choice([_lib.BF16, _lib.F16]) | (g.choice([0, _lib.PARAM_F32 | _lib.ACC_NATIVE]))
        if kind == "e4m3":
            got = lib.sow_forward_skinny_fp8_workspace_bytes(T, d_in, d_out, r, dt)
        elif kind == "mxfp4":
            got = lib.sow_forward_skinny_fp4_workspace_bytes(T, d_in, d_out, r, dt)
        else:
            got = lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, kinds[kind], dt)
        if got != FP.skinny_ws_bytes(T, d_in, d_out, kind):
            bad.append((kind, T, d_in, d_out, r, got, FP.skinny_ws_bytes(T, d_in, d_out, kind)))
    assert not bad, bad[:5]
    # ... and at every drawn case
    p = FP.plan()
    assert {FP.skinny_plan(c.d_in, c.d_out, c.kind)[1] for c in p.skinny} == set(FP.SK_KS)


def test_accumulator_predicates_mirror_the_library():
    """fused_acc_shape_ok / deep_acc_shape_ok against the package's predicates (which test_host_fused_acc_cpu and
    test_host_deep_acc_cpu tie to the C ones) and against the flagged workspace plan, which grows only on the admitted set;
    the LDS rule against the package's and against the header's words."""
    import torch

    from sow_amd import _lib, ops
    lib = _lib.load()
    g = random.Random(FP.SEED + 3)
    tdt = {"bf16": torch.bfloat16, "f16": torch.float16}
    LR = _lib.ACC_LOWRANK
    for i in range(2000):
        dt = g.choice(["bf16", "f16"])
        r, r_acc = g.randint(1, 70), g.choice([g.randint(1, 300), g.randint(180, 1000)])
        if i % 3:
            r, r_acc = r // 2 * 2, r_acc // 2 * 2
        d_in, d_out = g.choice([8 * g.randint(1, 80), g.randint(1, 640)]), g.choice([8 * g.randint(1, 80), g.randint(1, 640)])
        f, dp = FP.fused_acc_shape_ok(r, r_acc, d_in, d_out, dt), FP.deep_acc_shape_ok(r, r_acc, d_in, d_out, dt)
        assert f == ops.fused_acc_admits(d_in, d_out, r, r_acc, LR, tdt[dt]), (r, r_acc, d_in, d_out)
        assert dp == ops.deep_acc_admits(d_in, d_out, r, r_acc, LR, tdt[dt]), (r, r_acc, d_in, d_out)
        assert not (f and dp)
        if r < 1 or r_acc < 1:
            continue
        code = ops._DT[tdt[dt]]
        plain = lib.sow_workspace_bytes(300, d_in, d_out, r, r_acc, LR, code)
        if not f:
            assert lib.sow_workspace_bytes(300, d_in, d_out, r, r_acc, LR, code | _lib.FUSE_ACC) == plain, (r, r_acc, d_in, d_out)
        if not dp:
            assert lib.sow_workspace_bytes(300, d_in, d_out, r, r_acc, LR, code | _lib.FUSE_ACC_DEEP) == plain, (r, r_acc, d_in, d_out)
        if dp or (f and r_acc <= 64):
            flag = _lib.FUSE_ACC_DEEP if dp else _lib.FUSE_ACC
            assert lib.sow_workspace_bytes(300, d_in, d_out, r, r_acc, LR, code | flag) > plain, (r, r_acc, d_in, d_out)
    for _ in range(2000):
        tots = [g.randint(4, 256) for _ in range(g.randint(1, 4))]
        assert FP.shared_acc_lds_bytes(tots) == ops.shared_fused_acc_lds_bytes(tots)
        assert FP.shared_acc_lds_ok(tots) == (ops.shared_fused_acc_lds_bytes(tots) <= ops.SHARED_FUSED_ACC_MAX_LDS)
    assert FP.shared_acc_lds_bytes([200, 250, 256, 192]) == 160 * 1024 and not FP.shared_acc_lds_ok([256] * 4)
    assert FP.shared_acc_lds_bytes([]) == 0 and FP.shared_acc_lds_bytes([64] * 5) == 0
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sow_amd.h")).read()
    assert "128 * sum_i r_pad_i + max(128 * max_i r_pad_i + 8192, 24576) bytes" in header


# ---- the operands of the skinny cases ------------------------------------------------------------------------------------------------
def _ref_quantise(kind):
    import fp4_acc_ref as R4
    import fp8_acc_ref as R8

    def q8(W):
        codes, exps = R8.quantize(W)
        return codes, exps, R8.dequantize(codes, exps).to(W.dtype)

    def q4(W):
        codes, scales = R4.quantize(W)
        return codes, scales, R4.dequantize(codes, scales, W.dtype)

    return {"e4m3": q8, "mxfp4": q4}.get(kind)


def test_skinny_operands_clear_their_ties_within_the_cap():
    """Every single-layer case up to 8 M elements of W and every layer of the grouped calls: the tie-clearing step ends, having
    moved at most 1 % of A's elements (skinny_sweep.operands asserts it), by one ulp each; fp32 masters round to the factors."""
    import torch

    import skinny_sweep as SW
    import test_gpu_skinny as S
    p = FP.plan()
    cases = [c for c in p.skinny if c.d_in * c.d_out <= 8 << 20] + [m for g in p.skinny_groups if not g.x_shared for m in g.layers]
    assert len(cases) >= 60
    total = 0
    for c in cases:
        d, moved = SW.operands(c, _ref_quantise(c.kind))
        A0 = S._gauss(SW.DT[c.dtype], c.T, c.d_in, c.d_out, c.r, c.bias, "dense" if c.kind != "none" else "none", seed=c.seed)["A"]
        delta = d["A"].view(torch.int16).int() - A0.view(torch.int16).int()
        assert int((delta != 0).sum()) == moved and set(delta.unique().tolist()) <= {0, 1}, c.name
        assert (d["W"] is None) == (c.kind == "none") and (d.get("q") is not None) == (c.kind in ("e4m3", "mxfp4"))
        total += moved
        if c.f32:
            for k in ("A", "B", "bias"):
                if d[k] is not None:
                    m = SW.fp32_master(d[k])
                    assert m.dtype == torch.float32 and torch.equal(m.to(d[k].dtype).view(torch.int16), d[k].view(torch.int16))
                    if d[k].numel() >= 64:
                        assert float((m != d[k].float()).float().mean()) >= 0.5, "most masters are no numbers of the compute dtype"
    print(f"{len(cases)} layers, {total} elements of A moved off rounding ties")
