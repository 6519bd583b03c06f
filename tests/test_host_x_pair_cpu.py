"""CPU test of the X issue schedule of the chain kernel (chain2.hip: c2_x_issued, NO_X_PAIR switch).

The prologue, the stage loop and the counted wait of chain2_block all take the number of X stages issued so far from ONE
function, exported for this test as sow_debug_chain2_x_issued(st, nst, depth, paired): the stages issued when a wave reaches
the wait of stage st.  This test walks the ring of one token group with that function, for 0 ... 40 stages, depths 4, 5 and 6,
paired and one by one, and holds the three things a wrong schedule breaks silently:

  * a stage goes into slot st % depth only after the barrier that frees the slot -- the barrier of the stage AFTER the one
    that held it (at barrier s both waves of the group have finished stage s - 1);
  * the wait before barrier st counts exactly the stages issued after st (the DMA groups of a wave complete in order: a count
    too high leaves st in flight, a count too low drains the ring);
  * every stage is issued exactly once, in order.

The paired rule itself: after the prologue only the barriers of even stages issue, two stages at a time (one when the count is
odd and the last stage is left), and the look-ahead is depth - 2 stages."""
import ctypes

import pytest

from sow_amd import _lib

DEPTHS = (4, 5, 6)
NST = range(0, 41)


def issued_fn():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    f = lib.sow_debug_chain2_x_issued
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int] * 4
    return f


def walk(f, nst, depth, paired):
    """Simulate one block: returns [(stage, after_barrier)] in issue order (after_barrier = -1: prologue) and the wait counts."""
    order, waits = [], []
    issued = f(0, nst, depth, paired)
    order += [(s, -1) for s in range(issued)]
    for st in range(nst):
        assert f(st, nst, depth, paired) == issued, "the schedule is a function of the stage, not of the path to it"
        waits.append(issued - st - 1)
        upto = f(st + 1, nst, depth, paired)
        assert upto >= issued
        order += [(s, st) for s in range(issued, upto)]
        issued = upto
    return order, waits


@pytest.mark.parametrize("paired", [1, 0], ids=["paired", "one-by-one"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_ring_walk(depth, paired):
    f = issued_fn()
    for nst in NST:
        order, waits = walk(f, nst, depth, paired)
        # every stage exactly once, in order
        assert [s for s, _ in order] == list(range(nst)), (nst, depth, order)
        when = dict(order)
        for s, b in order:
            if s >= depth:
                # the slot held stage s - depth: free once barrier s - depth + 1 has been passed (a first use: any time)
                assert b >= s - depth + 1, (nst, depth, s, b)
            assert b < s, (nst, depth, s, b)               # ... and before its own wait
        for st, w in enumerate(waits):
            # stages issued after st when its wait is reached = those issued in the prologue or after a barrier before st
            newer = sum(1 for s, b in order if s > st and b < st)
            assert w == newer, (nst, depth, st, w, newer)
            assert 0 <= w <= 5, (nst, depth, st, w)         # wait_groups<2> has counted forms up to five groups
            assert when[st] < st


@pytest.mark.parametrize("depth", DEPTHS)
def test_paired_rule(depth):
    f = issued_fn()
    for nst in NST:
        order, waits = walk(f, nst, depth, 1)
        ahead = depth - 2
        assert [s for s, b in order if b == -1] == list(range(min(nst, ahead)))
        for st in range(nst):
            after = [s for s, b in order if b == st]
            if st % 2:
                assert after == [], (nst, depth, st, after)      # odd stages issue nothing
            else:
                assert after == [s for s in (st + ahead, st + ahead + 1) if s < nst], (nst, depth, st, after)
        # the wait count alternates between ahead - 1 and ahead until the tail
        for st, w in enumerate(waits):
            assert w == min(nst - 1 - st, ahead - 1 + st % 2), (nst, depth, st, w)


@pytest.mark.parametrize("depth", DEPTHS)
def test_one_by_one_rule_is_the_earlier_schedule(depth):
    f = issued_fn()
    for nst in NST:
        order, waits = walk(f, nst, depth, 0)
        assert [s for s, b in order if b == -1] == list(range(min(nst, depth - 1)))
        assert all(b == s - depth + 1 for s, b in order if b >= 0)
        assert waits == [min(nst - 1 - st, depth - 2) for st in range(nst)]


def test_build_depth_is_one_of_the_walked_ones():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.sow_debug_chain2_x_depth.restype = ctypes.c_int
    assert lib.sow_debug_chain2_x_depth() in DEPTHS
