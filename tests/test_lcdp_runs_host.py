"""The first chaining pass of an ultra-long -x lr read, work item by work item (rqphase.c: mga_lcdp_cut + hchain.c: mga_lchain_dp_fwd_range, what the host does with an item the
device hands back), equals the pass over the whole read (mga_lchain_dp_fwd) and, after the backtrack, the reference's mg_lchain_dp."""
import numpy as np
import pytest

import refbind as rb
import rmq_cases as rc
from test_gpu_lcdp import DIST_X, PAR, anchors, cut, host_fwd


@pytest.mark.parametrize("run_min", [1, 1024])
@pytest.mark.parametrize("seed", [11, 12])
def test_item_by_item_equals_whole_read(seed, run_min):
    """five pieces: B starts exactly dist_x behind A's last anchor (no boundary), C dist_x + 1 behind B's (boundary), D on the other strand at C's last position, E on another segment"""
    lo = lambda a, i: int(a["x"][i]) & 0xffffffff
    A, B, Cc, D, E = anchors(seed, 700, hi=2), anchors(seed + 1, 300, hi=2), anchors(seed + 2, 1500, hi=2), anchors(seed + 3, 40, hi=2 | 1 << 31), anchors(seed + 4, 900, hi=5, t0=50)
    B["x"] += np.uint64(lo(A, -1) + DIST_X - lo(B, 0))
    Cc["x"] += np.uint64(lo(B, -1) + DIST_X + 1 - lo(Cc, 0))
    D["x"] += np.uint64(lo(Cc, -1) - lo(D, 0))
    a = np.concatenate([A, B, Cc, D, E])
    want, cuts = host_fwd(a), cut(a, DIST_X, run_min)
    assert cuts[0] == 0 and cuts[-1] == len(a) and (np.diff(cuts)[:-1] >= run_min).all() and (np.diff(cuts) > 0).all()
    if run_min == 1:   # a gap of exactly dist_x is no boundary; dist_x + 1, a strand change and a segment change are
        assert {1000, 2500, 2540} <= set(cuts) and 700 not in cuts
    else:              # merged neighbours
        assert 1 < len(cuts) - 1 < 4
    got = (np.full(len(a), -7, np.int32), np.full(len(a), -7, np.int64), np.full(len(a), -7, np.int32))
    for beg, end in zip(cuts[:-1], cuts[1:]):
        host_fwd(a, rng=(beg, end), out=got)
    for g, w, name in zip(got, want, "fpv"):
        assert np.array_equal(g, w), name
    if rb.have_ref():
        u, b = rc.host_finish(a, *got, PAR["bw"], 3, 20)
        ru, rbb = rb.Ref().lchain_dp(a, max_dist_x=DIST_X, min_cnt=3, min_sc=20, **PAR)
        assert np.array_equal(u, ru) and np.array_equal(b, rbb)
