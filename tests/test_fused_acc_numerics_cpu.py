"""CPU: the bound that tests/test_gpu_fused_acc.py holds the fused low-rank-accumulator pass to (fused_acc_numerics.check)
admits the contract it was written for, on the very inputs of the GPU cases, and rejects the faults it is there to catch.

The contract is emulated in float64 with one-step roundings (numerics.rne) and again with fp32 products (the kernel's
accumulation noise); both must stay inside the single-rounding bound.  A lost accumulator column, a live term that was not
scaled and an h_save that misses its ones column must fail.
"""
import pytest
import torch

import fused_acc_numerics as FA
import test_gpu_elementwise as E
from numerics import NumericsError, to64

_MEMO = {}


def _case_data(c):
    if c.name not in _MEMO:
        _MEMO[c.name] = E._inputs(c)
    return _MEMO[c.name]


def _mm32(a, b):
    return (a.float() @ b.float()).double()


@pytest.mark.parametrize("c", FA.CASES, ids=lambda c: c.name)
def test_contract_emulation_stays_within_the_single_rounding_bound(c):
    d = _case_data(c)
    for what, mm in (("float64 products", None), ("fp32 products", _mm32)):
        out = FA.emulate(c, d, mm=mm)
        worst = FA.check(c, d, out)
        assert set(worst) == {"h_save", "y", "dx"}
        # the emulation has the hidden roundings of the contract and nothing else: well inside the bound
        assert max(worst.values()) <= 1.0, (what, worst)
        # h_save = NULL: y from a projection the test cannot see
        FA.check(c, d, dict(y=out["y"]))


def test_bound_rejects_a_lost_accumulator_column():
    c = FA.CASES[0]
    d = dict(_case_data(c))
    good = FA.emulate(c, d)
    dq = dict(d)
    dq["Q"] = d["Q"].clone()
    dq["Q"][:, c.r_acc - 1] = 0          # the last accumulator column never reaches y
    bad = FA.emulate(c, dq)
    with pytest.raises(NumericsError, match=": y"):
        FA.check(c, d, dict(h=good["h"], y=bad["y"]))
    dr = dict(d)
    dr["R"] = d["R"].clone()
    dr["R"][0] = 0                       # ... nor the first one dX
    bad = FA.emulate(c, dr)
    with pytest.raises(NumericsError, match=": dx"):
        FA.check(c, d, dict(h=good["h"], y=good["y"], dx=bad["dx"]))


def test_bound_rejects_a_scaled_accumulator_term():
    """The per-column scale: the accumulator columns take 1, the live columns s.  Scaling all of them by s must fail."""
    c = FA.CASES[0]
    d = _case_data(c)
    good = FA.emulate(c, d)
    ds = dict(d)
    ds["Q"] = (to64(d["Q"]) * c.s).to(c.dtype)
    bad = FA.emulate(c, ds)
    with pytest.raises(NumericsError, match=": y"):
        FA.check(c, d, dict(h=good["h"], y=bad["y"]))


def test_h_save_contract_is_checked():
    c = FA.CASES[0]
    d = _case_data(c)
    out = FA.emulate(c, d)
    h = out["h"].clone()
    h[5, 63] = 0.0
    with pytest.raises(NumericsError, match="column 63"):
        FA.check(c, d, dict(out, h=h))
    h = out["h"].clone()
    h[7, c.r] = 1.0
    with pytest.raises(NumericsError, match="padding"):
        FA.check(c, d, dict(out, h=h))
    # r_live = 64: column 63 is data
    c64 = next(k for k in FA.CASES if k.r == 64)
    o64 = FA.emulate(c64, _case_data(c64))
    assert not bool((o64["h"][:, 63] == 1.0).all())
    FA.check(c64, _case_data(c64), o64)


def test_two_pass_emulation_also_fits_where_the_first_term_is_small():
    """What the bound does NOT claim: it has no ulp(first) term, yet a second rounding of a first term smaller than y stays
    under one ulp of y.  The fused and the two-pass result are told apart by the kernel trace, not by this bound."""
    c = FA.CASES[0]
    d = _case_data(c)
    one, two = FA.emulate(c, d), FA.emulate(c, d, rounds=2)
    assert not torch.equal(one["y"], two["y"])
