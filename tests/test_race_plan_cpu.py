"""The plan of the under-load tests (tests/race_plan.py), tested on the CPU (no `gpu` mark): the ring table against the sources
and the ring-wrap condition, the multi-block condition against the resident grids of the sources, the slab plan the table rests
on against the C plan, the coverage of kernel_names(), the cost and size caps, unique ids that name their shapes, and that the
plan imports without torch."""
import ctypes
import re
import subprocess
import sys

import fuzz_plan as FP
import graph_plan as GP
import race_plan as RP


def test_plan_imports_without_torch():
    code = "import sys; sys.path.insert(0, %r); import race_plan; assert 'torch' not in sys.modules; print(len(race_plan.CASES))"
    out = subprocess.run([sys.executable, "-c", code % RP.__file__.rsplit("/", 1)[0]], capture_output=True, text=True)
    assert out.returncode == 0 and int(out.stdout) == len(RP.CASES), out.stderr


def test_ring_table_matches_the_sources_and_every_ring_wraps():
    by = {c.id: c for c in RP.CASES}
    assert set(RP.RINGS) <= set(by), sorted(set(RP.RINGS) - set(by))
    rows = [(cid, r) for cid, rs in RP.RINGS.items() for r in rs]
    for cid, r in rows:
        have = RP.constant(r.file, r.name)
        assert have == r.slots, f"{cid}: {r.file} {r.name} is {have}, the table says {r.slots}"
        assert r.trips >= 3 * r.slots, f"{cid}: {r.name} of {r.file} has {r.slots} slots, the case makes {r.trips} trips ({r.unit})"
    # every ring of the module docstring is wrapped three times by at least one case
    names = {"C2_DEPTH", "C2_NSLOT", "CS_DEPTH", "CS_NSLOT", "C3_DEPTH", "C3_NSLOT", "C4_XDEPTH", "C4_RING0", "TN_DEPTH",
             "TNW_DEPTH", "TNR_DEPTH", "TNF_DEPTH", "TNFW_DEPTH", "TNQ_DEPTH", "G2_NSLOT", "G3_NSLOT", "GH_NSLOT", "GS_NSLOT",
             "G4_LDS", "G4_PA_RING"}
    assert {r.name for _, r in rows} == names
    for n in names:
        assert n in RP.__doc__ or n in RP.LITERALS, n
    # a ring somebody deepens turns the table red: the lookup reads the sources, not a copy
    assert RP.constant("chain2.hip", "C2_DEPTH") == 4 and RP.constant("chain2.hip", "C2_NSLOT") == 6
    assert RP.constant("chain2.hip", "C2_AHEAD") == 5 and RP.constant("chain2_shared.hip", "CS_AHEAD") == 5


def test_last_trip_is_partial():
    """Widths 8 past a multiple of the stage, token counts 1 past a multiple of the block."""
    for c in RP.LAYERS:
        m = c.p["layer"]
        if c.id in RP.RINGS and any(r.file.startswith("chain") for r in RP.RINGS[c.id]):
            assert m.d_in % 64 in (8, 32) and m.d_out % 64 in (8, 32) and m.T % 64 in (1, 40), c.id     # (1000 = 15 * 64 + 40)
    for c in RP.GEMMS:
        assert c.p["K"] % 64 == 8, c.id


def test_multi_block_cases_run_two_and_three_blocks():
    assert {m.name for m in RP.MULTI.values()} == {"C2_RESIDENT", "CS_RESIDENT", "TNW_RESIDENT"}
    for cid, m in RP.MULTI.items():
        grid = RP.constant(m.file, m.name)
        assert 2 * grid < m.blocks < 3 * grid, f"{cid}: {m.blocks} blocks on {grid} resident workgroups"
        assert not RP.switches(next(c for c in RP.CASES if c.id == cid)).get("NO_PERSIST")
    # the grouped weight-gradient launch is the wide kernel's, not the row-owner plan's
    g = RP.GROUPS[0].p
    ls = g["layers"]
    assert g["deferred"] and not g["rows"]
    assert not FP.tn_rows_plan([ls[0].T] * 2 * len(ls), [v for m in ls for v in (m.d_in, m.d_out)])


def test_slab_plan_is_the_c_plan():
    """tn_slabs (the token-slab rings and the grouped launch's block count rest on it) against sow_backward_group_plan, a host
    function, for every layer of the plan with r <= 64."""
    from sow_amd import _lib
    lib = _lib.load()
    code = {"bf16": _lib.BF16, "f16": _lib.F16, "f32": _lib.F32}
    layers = [c.p["layer"] for c in RP.LAYERS] + list(RP.GROUPS[0].p["layers"])
    checked = 0
    for m in layers:
        if m.r > 64:
            continue
        arr = (_lib.LayerArgs * 1)()
        a = arr[0]
        a.x, a.A, a.B, a.y, a.h_save, a.dy, a.dx, a.dA, a.dB, a.workspace = (0x10000 * (k + 1) for k in range(10))     # never read
        a.T, a.d_in, a.d_out, a.r_live, a.scale = m.T, m.d_in, m.d_out, m.r, 1.0
        if m.acc == "dense":
            a.acc_down, a.acc_kind = 0x100000, _lib.ACC_DENSE
        slabs = (ctypes.c_int * 2)()
        with _lib.switch(**m.switches):
            rc = lib.sow_backward_group_plan(arr, 1, code[m.dtype], _lib.BWD_DATA | _lib.BWD_WEIGHTS, slabs)
            assert rc == 0, (m.name, rc)
            ns, ln = RP.tn_slabs(m.T, m.d_in, m.d_out, m.dtype, narrow=bool(m.switches.get("TN_NARROW")))
        assert slabs[0] == slabs[1] == ns, f"{m.name}: the C plan cuts {slabs[0]} slabs, tn_slabs {ns} of {ln} tokens"
        checked += 1
    assert checked >= 15


def test_every_kernel_is_claimed_or_exempt():
    names = GP.kernel_names()
    assert len(names) >= 70, sorted(names)
    claimed = RP.claimed()
    assert not claimed - names, f"claims that are no __global__ of the sources: {sorted(claimed - names)}"
    left = names - claimed - set(RP.EXEMPT)
    assert not left, f"kernels neither claimed by a case nor exempt: {sorted(left)}"
    assert not claimed & set(RP.EXEMPT)
    assert RP.EXEMPT == GP.EXEMPT


def test_ids_are_unique_and_name_their_shape():
    ids = [c.id for c in RP.CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    for c in RP.CASES:
        numbers = {int(v) for v in re.findall(r"\d+", c.id)}
        missing = [v for v in c.shape if v not in numbers]
        assert not missing, f"{c.id} does not name {missing} of its shape {c.shape}"
        assert c.claims and c.kind, c.id
    # a replaced graph_plan case is replaced by a case that claims its kernels
    gone = [c for c in GP.CASES if c.id in RP.REPLACED]
    new = {k for c in RP.LAYERS + RP.GROUPS + RP.SHARED + RP.GEMMS for k in c.claims}
    assert all(set(c.claims) <= new for c in gone), [c.id for c in gone if not set(c.claims) <= new]


def test_cost_and_size_caps():
    p = FP.plan()
    cap = max(FP.ref_cost(c) for xs in (p.layers, p.groups, p.shared, p.gemms, p.skinny, p.skinny_groups, p.fused, p.deep, p.shared_acc)
              for c in xs)
    assert cap <= FP.REF_COST_CAP
    worst = max(RP.CASES, key=lambda c: c.cost)
    big = max(RP.CASES, key=RP.case_bytes)
    print(f"worst float64 reference {worst.cost:.3g} multiply-adds ({worst.id}); the fuzz plan's most expensive case {cap:.3g}")
    print(f"largest buffers {RP.case_bytes(big) / 2 ** 20:.0f} MiB ({big.id}); cap {RP.MAX_BYTES >> 20} MiB")
    assert worst.cost <= cap
    assert RP.case_bytes(big) <= RP.MAX_BYTES
    for c in RP.CASES:
        if c.kind == "layer":
            assert c.cost == FP.ref_cost(c.p["layer"])
        elif c.kind == "group":
            assert c.cost == sum(FP.ref_cost(m) for m in c.p["layers"])


def test_dtypes_and_switches_appear():
    lay = [c.p["layer"] for c in RP.CASES if c.kind == "layer"]
    assert {m.dtype for m in lay} == {"bf16", "f16", "f32"}
    assert any(c.kind == "layer" and c.p["param_f32"] for c in RP.CASES)
    seen = {k for c in RP.CASES for k in RP.switches(c)}
    assert {"TN_NARROW", "NO_GEMM4H", "GEMM3", "GEMM3S", "NO_ROW_ALIGN", "NO_H_ROWS", "NT_LOAD", "NO_NT_STORE"} <= seen, seen
    for m in lay:
        if m.name.startswith("chain2al") and not m.switches.get("NO_ROW_ALIGN"):      # launch_chain2_group's half_off()
            assert m.d_in % 64 == 32 and m.d_out % 64 == 32 and not m.bias and not m.grad_beta
