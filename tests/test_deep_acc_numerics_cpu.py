"""CPU: the bound that tests/test_gpu_deep_acc.py holds the fused pass past 256 columns to (fused_acc_numerics.check on the
cases of deep_acc_numerics) admits the contract, on the very inputs of the GPU cases, and rejects the faults the column-group
code could make: a lost column of the SECOND group, a live term scaled by 1.

The contract is emulated in float64 with one-step roundings (numerics.rne) and again with fp32 products (the kernel's
accumulation noise); both must stay inside the single-rounding bound.
"""
import dataclasses

import pytest

import deep_acc_numerics as DA
import test_gpu_elementwise as E
from numerics import NumericsError

_MEMO = {}


def _case_data(c):
    if c.name not in _MEMO:
        _MEMO[c.name] = E._inputs(c)
    return _MEMO[c.name]


def _mm32(a, b):
    return (a.float() @ b.float()).double()


def test_cases_are_the_admitted_set_past_256():
    from sow_amd import _lib, ops
    for c in DA.CASES:
        assert 256 < c.r + c.r_acc <= 960 and DA.r_pad(c) // 64 <= 15
        assert ops.deep_acc_admits(c.d_in, c.d_out, c.r, c.r_acc, _lib.ACC_LOWRANK, c.dtype)
        assert not ops.fused_acc_admits(c.d_in, c.d_out, c.r, c.r_acc, _lib.ACC_LOWRANK, c.dtype)
    assert len({c.name for c in DA.CASES}) == len(DA.CASES) == 10


@pytest.mark.parametrize("c", DA.CASES, ids=lambda c: c.name)
def test_contract_emulation_stays_within_the_single_rounding_bound(c):
    d = _case_data(c)
    for what, mm in (("float64 products", None), ("fp32 products", _mm32)):
        out = DA.emulate(c, d, mm=mm)
        worst = DA.check(c, d, out)
        assert set(worst) == {"h_save", "y", "dx"}
        assert max(worst.values()) <= 1.0, (what, worst)
        DA.check(c, d, dict(y=out["y"]))   # h_save = NULL: y from a projection the test cannot see


@pytest.mark.parametrize("name", ["tot258", "straddle_256", "tot960"])
def test_bound_rejects_a_lost_column_of_a_later_group(name):
    """Column 256 is the first of the second group (an accumulator column in tot258, where the group holds two real columns,
    and in tot960; a live column in straddle_256); in tot960 the last accumulator column, 909, lies in the fourth."""
    c = DA.BY_NAME[name]
    d = dict(_case_data(c))
    good = DA.emulate(c, d)
    col = 909 if name == "tot960" else 256
    key_f, key_b = ("Q", "R") if col < c.r_acc else ("A", "B")
    k = col if col < c.r_acc else col - c.r_acc
    df = dict(d)
    df[key_f] = d[key_f].clone()
    df[key_f][:, k] = 0                  # the column never reaches y
    bad = DA.emulate(c, df)
    with pytest.raises(NumericsError, match=": (y|h_save)"):
        DA.check(c, d, dict(h=good["h"] if key_f == "Q" else bad["h"], y=bad["y"]))
    db = dict(d)
    db[key_b] = d[key_b].clone()
    db[key_b][k] = 0                     # ... nor dX
    bad = DA.emulate(c, db)
    with pytest.raises(NumericsError, match=": dx"):
        DA.check(c, d, dict(h=good["h"], y=good["y"], dx=bad["dx"]))


@pytest.mark.parametrize("name", ["straddle_256", "llama60m_racc450"])
def test_bound_rejects_a_live_term_scaled_by_one(name):
    """The per-column scale: the accumulator columns take 1, the live columns s -- also past the group boundary.  A live
    term scaled by 1 must fail (h_save shows it; with h_save = NULL, y does)."""
    c = DA.BY_NAME[name]
    d = _case_data(c)
    bad = DA.emulate(dataclasses.replace(c, s=1.0), d)
    with pytest.raises(NumericsError, match=": h_save"):
        DA.check(c, d, dict(h=bad["h"], y=bad["y"]))
    with pytest.raises(NumericsError, match=": y"):
        DA.check(c, d, dict(y=bad["y"]))


def test_bound_rejects_a_scaled_accumulator_term():
    c = DA.BY_NAME["tot258"]
    d = _case_data(c)
    good = DA.emulate(c, d)
    ds = dict(d)
    ds["Q"] = (d["Q"].double() * c.s).to(c.dtype)
    bad = DA.emulate(c, ds)
    with pytest.raises(NumericsError, match=": y"):
        DA.check(c, d, dict(h=good["h"], y=bad["y"]))


def test_h_save_contract_is_checked_where_the_live_panel_is_whole():
    c = DA.BY_NAME["tot320_r64"]
    o = DA.emulate(c, _case_data(c))
    assert not bool((o["h"][:, 63] == 1.0).all())      # r_live = 64: column 63 is data
    DA.check(c, _case_data(c), o)
    c = DA.BY_NAME["straddle_256"]
    o = DA.emulate(c, _case_data(c))
    h = o["h"].clone()
    h[5, 63] = 0.0
    with pytest.raises(NumericsError, match="column 63"):
        DA.check(c, _case_data(c), dict(o, h=h))
