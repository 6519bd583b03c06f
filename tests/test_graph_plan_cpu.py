"""The plan of the graph-replay tests (tests/graph_plan.py), tested on the CPU (no `gpu` mark): every __global__ kernel of the
sources is claimed by a case or exempt with a cited host read, the case ids are unique and name their shapes, every float64
reference stays under the cost cap of the fuzz plan, and the planned shapes sit where their family's predicate puts them."""
import re

import fuzz_plan as FP
import graph_plan as GP


def test_every_kernel_is_claimed_or_exempt():
    names = GP.kernel_names()
    assert len(names) >= 70, sorted(names)                  # the scan found the sources
    assert {"chain2_kernel", "gemm4_kernel", "gemm4_f16_splitk_reduce_kernel", "qr_copy_in_kernel", "tt_adam_eval_kernel"} <= names
    assert "G4_KERNEL" not in names and "G4_REDUCE" not in names, "a macro stands for a kernel name"
    claimed = GP.claimed()
    unknown = claimed - names
    assert not unknown, f"claims that are no __global__ of the sources: {sorted(unknown)}"
    left = names - claimed - set(GP.EXEMPT)
    assert not left, f"kernels neither claimed by a case nor exempt: {sorted(left)}"
    both = claimed & set(GP.EXEMPT)
    assert not both, f"claimed and exempt: {sorted(both)}"


def test_exemptions_cite_a_host_read():
    for name, reason in GP.EXEMPT.items():
        assert name in GP.kernel_names(), name
        # the reason names the entry point and the read that its documented contract makes on the host
        assert re.search(r"sow_\w+|ops\.\w+", reason) and re.search(r"host|\.item\(\)|synchronis", reason), (name, reason)
        assert "hard to reach" not in reason.lower()


def test_ids_are_unique_and_name_their_shape():
    ids = [c.id for c in GP.CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    for c in GP.CASES:
        numbers = {int(v) for v in re.findall(r"\d+", c.id)}
        missing = [v for v in c.shape if v not in numbers]
        assert not missing, f"{c.id} does not name {missing} of its shape {c.shape}"
        assert c.claims and c.kind, c.id


def test_reference_cost_under_the_cap():
    worst = max(GP.CASES, key=lambda c: c.cost)
    print(f"worst float64 reference {worst.cost:.3g} multiply-adds ({worst.id}); cap {FP.REF_COST_CAP:.3g}")
    assert worst.cost <= FP.REF_COST_CAP
    for c in GP.CASES:
        if c.kind == "layer":
            assert c.cost == FP.ref_cost(c.p["layer"])
        elif c.kind == "group":
            assert c.cost == sum(FP.ref_cost(m) for m in c.p["layers"])


def test_shapes_select_their_families():
    """The predicates fuzz_plan.py mirrors from api.hip, at the planned shapes."""
    by = {c.id: c for c in GP.CASES}
    lay = {c.p["layer"].name: c.p["layer"] for c in GP.CASES if c.kind == "layer"}
    for c in lay.values():
        if "chain2_" in c.name and c.dtype != "f32":      # streaming chain2: no short split
            assert c.T // 64 + (c.T % 64 > 0) > 128 and c.d_in % 8 == 0 and c.d_out % 8 == 0 and c.r % 2 == 0 and 4 <= c.r <= 64
        if c.name.startswith("short"):
            assert FP.cdiv(c.T, 64) <= 128 and FP.cdiv(c.d_in, 64) + FP.cdiv(c.d_out, 64) >= 24
        if c.name.startswith("gemm4h"):
            assert FP.cdiv(c.T, 256) * FP.cdiv(c.d_out, 256) >= 120 and c.d_in <= 512 and c.d_out <= 512
        if c.name.startswith("gemm2h"):
            assert FP.cdiv(c.T, 256) * FP.cdiv(c.d_out, 256) >= 160 and c.switches == {"NO_GEMM4H": 1}
        if c.name.startswith("splitk"):
            assert FP.gemm2_ok(c.T, c.d_out, c.d_in) and c.d_in >= 96 * 64 and FP.cdiv(c.T, 256) * FP.cdiv(c.d_out, 256) <= 128
            assert FP.gemm2_ok(c.T, c.d_in, c.d_out) and FP.cdiv(c.T, 64) * 64 < c.d_in      # gemm3s backward, pad64 on its own
        if c.name.startswith(("wide", "ragged")):
            assert 64 < c.r <= 256 and c.r % 2 == 0 and FP.tnw_pick_slabs(c.T, c.d_in, c.d_out)[0] >= 2
        if c.name.startswith("ragged"):
            assert c.d_in % 8 or c.d_out % 8
        if c.name.startswith("chain3f"):
            assert c.T >= 8192 and c.dtype == "f32"
    for c in GP.GROUPS:
        ls = c.p["layers"]
        rows = c.p["dtype"] == "bf16" and FP.tn_rows_plan([ls[0].T] * 2 * len(ls), [v for m in ls for v in (m.d_in, m.d_out)])
        assert rows == c.p["rows"], c.id
        assert all(m.r <= 63 or not m.bias for m in ls)
    assert any(c.p["deferred"] for c in GP.GROUPS) and any(c.p["rows"] for c in GP.GROUPS)
    for c in GP.SHARED:
        assert c.shape[0] > 8192
    for c in GP.SKINNY:
        assert c.p["T"] <= 32
    g = {c.id: c.p for c in GP.GEMMS}
    for cid, p in g.items():
        M, N, K = p["M"], p["N"], p["K"]
        t256, t128 = FP.cdiv(M, 256) * FP.cdiv(N, 256), FP.cdiv(M, 128) * FP.cdiv(N, 128)
        fam = by[cid].claims[-1]
        if fam in ("gemm3s_kernel", "gemm2_kernel", "gemm3_kernel"):
            assert p["dtype"] == "bf16" and FP.gemm2_ok(M, N, K) and t256 < 120
        if fam == "gemm4_kernel" and not p["use_ws"]:
            assert FP.gemm2_ok(M, N, K) and t256 >= 120 and K >= 64
        if p["use_ws"]:
            assert t256 <= 128 and K >= 96 * 64
        if fam == "gemm_kernel":
            assert N % 8
    assert {m.dtype for m in lay.values()} == {"bf16", "f16", "f32"}
