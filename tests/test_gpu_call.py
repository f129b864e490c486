"""GPU stage test of k_call.hip through mga_call_batch: crafted walks over a crafted segment table (call_cases.py), record for record against the host instantiation of
call_core.h and the Python replay -- the winner per bubble with st, en, strand, qs, qe, glen, and the warning list in order.  What every case must produce is pinned on the
CPU by test_call_host.py::test_crafted_cases_are_what_they_claim."""
import faulthandler

import numpy as np
import pytest

import minigraph_amd as mga
import call_cases as kc

pytestmark = pytest.mark.gpu

K, GROUPS = kc.crafted()


@pytest.fixture(autouse=True)
def time_limit():
    """every test here under its own limit (the dump names the test; the process exits)"""
    faulthandler.dump_traceback_later(60, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def check(F):
    win, warns = kc.replay(**F)
    hwin, hwarn = mga.call_chains_host(**F)
    dwin, dwarn = mga.call_batch(**F)
    assert kc.win_of(hwin) == win and kc.warn_of(hwarn) == warns
    assert kc.win_of(dwin) == win, (kc.win_of(dwin), win)
    assert kc.warn_of(dwarn) == warns, (kc.warn_of(dwarn), warns)
    assert np.array_equal(dwin, hwin)   # every byte of the records, the bubbles without a winner included
    return win, warns


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_case_equals_host_and_replay(name):
    check(K.arrays(GROUPS[name]))


def test_three_chains_compete_in_any_launch_order():
    """three chains in three workgroups that all survive for bubble 7: the last in (t, i, j) order wins, whatever the order of the records in the launch"""
    want = None
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        win, _ = check(K.arrays(GROUPS["three_compete"], order))
        assert win[7][0] >> 32 == GROUPS["three_compete"][2]
        assert want is None or win == want
        want = win


def test_one_launch_holds_everything():
    """all crafted chains in one launch, in (t, i) order and in a launch order that differs from it"""
    n = len(K.chains)
    a, wa = check(K.arrays())
    b, wb = check(K.arrays(None, np.random.default_rng(5).permutation(n)))
    assert a == b and wa == wb and len(a) >= 8 and len(wa) == 4


def test_records_pointing_outside_are_refused():
    F = K.arrays(GROUPS["walk_65"])
    F["chains"]["cnt"][0] = len(F["pos"]) + 1
    with pytest.raises(RuntimeError, match="outside"):
        mga.call_batch(**F)
