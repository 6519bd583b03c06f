"""The generator of the element-wise random sweep (tests/fuzz_plan.py), tested on the CPU (no `gpu` mark): deterministic,
the stratum counts met, the named edges drawn, every case's float64 reference under the cost cap."""
import collections

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
