"""The operand generator of tests/test_gpu_values_elementwise.py (tests/value_plan.py), tested on the CPU (no `gpu` mark):
every case of family A is proved exact from its float64 reference -- stored intermediates representable, sum |terms| below
2^24 units, one 8-bit factor in every fp32 product -- and dense enough to notice a dropped token; every case admits grid
points of family B at both ends of the range; every reference stays under fuzz_plan.REF_COST_CAP."""
import math

import pytest
import torch

import fuzz_plan as FP
import value_plan as V

CASES = V.cases()
BF16 = torch.bfloat16


def test_case_list_is_deterministic_and_under_the_cost_cap():
    assert V.cases() == CASES
    every = CASES.layers + CASES.shared + CASES.gemms + [m for g in CASES.groups for m in g.layers]
    worst = max(every, key=FP.ref_cost)
    print(f"{len(CASES.layers)} layers, {len(CASES.groups)} groups, {len(CASES.shared)} shared sets, {len(CASES.gemms)} GEMMs; "
          f"worst float64 reference {FP.ref_cost(worst):.3g} multiply-adds ({worst.name})")
    assert FP.ref_cost(worst) <= FP.REF_COST_CAP
    targeted = {c.family for c in CASES.layers} | {g.family for g in CASES.gemms}
    for fam in ("chain2_kernel", "chain2_f16_kernel", "h_reduce_kernel", "chain_kernel", "chain_wide_kernel", "chain3f_kernel",
                "chain2f_kernel", "tn_partial_f32_quad_kernel", "tn_partial_dma_f32_kernel", "gemm4_kernel", "gemm4_f16_kernel",
                "gemm2h_kernel", "gemm2_kernel", "gemm3s_kernel", "gemm_x3_kernel", "gemm_kernel", "gemm4_splitk_reduce_kernel"):
        assert fam in targeted, fam
    assert any(g.rows for g in CASES.groups) and CASES.shared
    flagged = [c for c in CASES.layers if V.f32_gradients(c)]
    assert {c.stratum for c in flagged} == {"chain2", "gemm4h", "gemm2h", "lowrank"} and {c.dtype for c in flagged} == {"bf16", "f16"}
    for c in every:
        if isinstance(c, FP.Layer):
            assert math.frexp(c.s)[0] == 0.5 and c.grad_beta in (0.0, 0.5, 1.0), c.name


def test_lsb_and_sum_bound():
    t = lambda *v: torch.tensor(v, dtype=torch.float64)   # noqa: E731
    assert V.lsb(t(1.0, 0.5, 3.0, 0.0)) == 0.5 and V.lsb(t(6.0, -12.0)) == 2.0 and V.lsb(t(0.0)) == math.inf
    assert V.lsb(t(5 * 2.0 ** -6, 8.0)) == 2.0 ** -6
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(40, 30, generator=g, dtype=torch.float64), torch.randn(30, 20, generator=g, dtype=torch.float64)
    assert V.sum_abs_bound(a, b) >= V.sum_abs_bound(a, b, exact=True) == float((a.abs() @ b.abs()).max())


def test_a_case_that_is_not_exact_is_refused():
    c = CASES.layers[0]
    d, _ = V.exact_layer_proved(c)
    bad = dict(d, A=d["A"] * 1.001)                        # not representable in bf16
    with pytest.raises(V.NotExact, match="operand A"):
        V.prove_layer(c, bad)
    bad = dict(d, A=d["A"] * 129)                          # h = s x A past the integers bf16 holds
    with pytest.raises(V.NotExact, match="stored intermediate"):
        V.prove_layer(c, bad)
    g = torch.Generator().manual_seed(1)
    wide = V._wide_values(g, (8, 8))                       # both factors of a product wider than 8 bits
    with pytest.raises(V.NotExact, match="8 significant bits"):
        V._prove_sum("both wide", wide, wide.t().contiguous(), [], "f32")
    ones = torch.ones(8, 2 ** 13, dtype=torch.float64)     # 2^13 terms of 2^17 units each
    with pytest.raises(V.NotExact, match="not below 2\\^24"):
        V._prove_sum("long", ones, wide[:1, :1].expand(2 ** 13, 1).contiguous(), [], "f32")


@pytest.mark.parametrize("c", CASES.layers + [m for g in CASES.groups for m in g.layers], ids=lambda c: c.name)
def test_layer_is_exact_dense_and_scalable(c):
    d, f = V.exact_layer_proved(c)           # prove_layer + check_density, at the first level of the ladder that passes
    if c.dtype == "f32":                     # the mid and lo planes of the split are exercised: a 17-bit operand
        w = d[V.wide_operand(c)]
        wide = (w.to(BF16).double() != w)
        assert int(wide.sum()) >= 8, f"{c.name}: {int(wide.sum())} wide values"
        assert not V._fits(w, BF16) and V._fits(w, torch.float32)
    grid = [e for e, _ in V.grid_for(c, V.range_stats(c, d, f), exact=True)]
    assert len(grid) >= 2, f"{c.name}: admits {[e.tag() for e in grid]}"
    up = [e for e in grid if min(e.exps()[k] for k in ("y", "dA", "dB")) > 0]
    down = [e for e in grid if max(e.exps()[k] for k in ("y", "dA", "dB")) < 0]
    assert up and down, f"{c.name}: the admitted grid points {[e.tag() for e in grid]} do not reach both ways"
    if c.dtype == "f16":
        GRADSCALED[c.name] = V.GRADSCALER in grid
    if V.f32_gradients(c):   # the run with fp32 gradients: 0 % of dA, dB, dbias beyond what fp32 holds (check_density)
        assert all(V._fits(f[k], torch.float32) for k in ("dA", "dB") + (("dbias",) if c.bias else ()))


GRADSCALED = {}   # f16 case -> admits the GradScaler point (filled by the test above, completed by the one below)


def test_which_f16_cases_take_the_gradscaler_point():
    """dY * 2^13 -- a GradScaler's 2^16 on gradients of magnitude 2^-3 (value_plan.GRID says why not more) -- is admitted by
    exactly the f16 cases listed here: with these integer-valued operands dB and dbias, sums over all tokens, pass 65504 at
    long T, so the chain2_f16 backward, the dense and the low-rank f16 paths see the grid's other points only."""
    for c in CASES.layers:
        if c.dtype == "f16" and c.name not in GRADSCALED:
            d, f = V.exact_layer_proved(c)
            GRADSCALED[c.name] = not isinstance(V.admits(c, V.range_stats(c, d, f), V.GRADSCALER, exact=True), str)
    took = sorted(n for n, ok in GRADSCALED.items() if ok)
    print(f"the GradScaler point is admitted by {took}")
    assert took == sorted(["v_chain2_f16_T9807_424x360_r64_noh", "v_chain2_f16_T17302_320x224_r62_FORCE_CHAIN_V11",
                           "v_ragged_f16_T149_206x160_r134", "v_generic_f16_T36_464x272_r22"])


@pytest.mark.parametrize("sp", CASES.shared, ids=lambda s: s.name)
def test_shared_set_is_exact(sp):
    sibs, x, per, dx0, fs, ref_dx = V.exact_shared(sp)
    assert float((ref_dx != 0).double().mean()) >= 0.5
    assert all(p["dy"].shape == (sp.T, sb.d_out) for p, sb in zip(per, sp.sibs))


@pytest.mark.parametrize("gm", CASES.gemms, ids=lambda g: g.name)
def test_gemm_is_exact_and_scalable(gm):
    a, b, bias, c0 = V.exact_gemm(gm)
    V.prove_gemm(gm, a, b, bias, c0)
    for ea, eb in V.gemm_scales(gm):
        V.prove_gemm_range(gm, a, b, bias, c0, ea, eb)
    if gm.dtype == "f32":
        assert not (V._fits(a, BF16) and V._fits(b, BF16))


def test_poison_placements():
    for c in CASES.layers:
        tags = [t for t, _, _ in V.poisons(c)]
        assert {"x_mid", "x_last", "dy", "A"} <= set(tags)
        assert ("x_wrap" in tags) == bool((c.d_in % 8 or c.misalign) and c.T > 2)
        for _, op, where in V.poisons(c):
            rows, cols = {"x": (c.T, c.d_in), "dy": (c.T, c.d_out), "A": (c.d_in, c.r)}[op]
            assert all(0 <= i < rows and 0 <= j < cols for i, j in where)
