"""The plan of the event walks (tests/train_walk_plan.py), tested on the CPU (no `gpu` mark): deterministic, every event kind
and every named transition present, the token counts and model specs the runner relies on, every walk's float64 reference
under the cost cap of the random sweep."""
import collections

import fuzz_plan as FP
import train_walk_plan as WP


def test_plan_is_deterministic():
    a, b = WP.plan(), WP.plan()
    assert a == b
    assert WP.plan(WP.SEED + 1) != a
    assert WP.plan(WP.SEED + 1)[:10] == a[:10]                      # the hand-written walks do not depend on the seed
    assert len({w.id for w in a}) == len(a)


def test_every_event_kind_and_parameter_occurs():
    p = WP.plan()
    evs = [e for w in p for e in w.events]
    assert {e.kind for e in evs} == set(WP.KINDS)
    assert {e.reentrant for e in evs if e.kind == "ckpt_step"} == {True, False}
    assert {e.drop for e in evs if e.kind == "partial_step"} == set(WP.DROPS)
    assert {e.mode for e in evs if e.kind == "regroup"} == set(WP.REGROUP_MODES)
    assert {e.on for e in evs if e.kind == "autocast"} == {True, False}
    assert {e.group for e in evs if e.kind == "reset_state"} == {0, 1}
    evals = [e.T for e in evs if e.kind == "eval"] + [e.eval_T for e in evs if e.eval_T]
    assert min(evals) <= 32 < max(evals) and {31, 32, 33} <= set(evals)
    assert any(e.eval_T and e.eval_T <= 32 for e in evs) and any(e.eval_T > 32 for e in evs)
    # accumulate(): once from no accumulator and once from an existing one
    starts = set()
    for w in p:
        n = 0
        for e in w.events:
            if e.kind == "accumulate":
                starts.add(WP.acc_after(w.model, n)[0])
                n += 1
    assert {"none", "lowrank"} <= starts


def test_every_named_transition_occurs():
    p = WP.plan()
    seen = collections.Counter(t for w in p for t in WP.transitions(w))
    print(dict(seen))
    for name in WP.TRANSITIONS:
        assert seen[name] >= 1, name
    for w in p:                                                     # a micro-batch follows a backward pass directly
        for a, b in zip(w.events, w.events[1:]):
            if b.kind == "micro":
                assert a.kind in ("step", "micro") and not a.eval_T, (w.id, str(a))


def test_token_counts_and_models():
    p = WP.plan()
    hand, seeded = p[:10], p[10:]
    assert 8 <= len(hand) <= 12 and len(seeded) == 8
    assert all(10 <= len(w.events) <= 14 for w in seeded)
    fuse = [w for w in p if any(WP.T_FUSE in (e.T, e.eval_T) for e in w.events)]
    assert len(fuse) == 1 and (fuse[0].model.hidden, fuse[0].model.inter) == (128, 264) and fuse[0].model.acc == "lowrank"
    for w in p:
        m = w.model
        assert (m.hidden, m.inter) in WP.GEOMETRIES and m.dtype in WP.DTYPES and m.grouping in WP.REGROUP_MODES
        assert m.rank <= 63 and m.bias                             # every layer's kernels can produce dbias (dp.bias_route_ok)
        for e in w.events:
            assert e.kind in WP.KINDS
            for T in (e.T, e.eval_T):
                assert T == 0 or T in WP.TS or T == WP.T_FUSE, (w.id, str(e))
            assert (e.T > 0) == (e.kind in WP.GRAD_KINDS + ("eval",)), (w.id, str(e))
            if e.kind == "autocast":
                assert m.dtype == "f32", w.id                       # the toggle belongs to fp32 walks
            if e.kind == "reset_state":
                assert e.group == 0 or m.bucket_biases, w.id
    used = {T for w in p for e in w.events for T in (e.T, e.eval_T) if T}
    assert used == set(WP.TS) | {WP.T_FUSE}
    assert {w.model.dtype for w in p} == set(WP.DTYPES)             # one dtype per walk, every dtype in some walk
    assert {w.model.acc for w in p} == {"none", "dense", "lowrank"}
    assert {w.model.bucket_biases for w in p} == {True, False}
    assert {w.model.grouping for w in p} == set(WP.REGROUP_MODES)


def test_reference_cost_under_the_cap():
    p = WP.plan()
    worst = max(p, key=WP.ref_cost)
    for w in p:
        print(f"{w.id:44s} {len(w.events):2d} events  {WP.ref_cost(w):.3g} multiply-adds")
    assert WP.ref_cost(worst) <= FP.REF_COST_CAP, (worst.id, WP.ref_cost(worst))
