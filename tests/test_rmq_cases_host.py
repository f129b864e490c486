"""CPU: the anchor sets of rmq_cases.py are what test_gpu_rmq.py assumes -- proved with the host tree's brute-force tie counter (rmq.c: mga_rq_tie_stats_enable) and a numpy
bound of the inner walk's candidates, so that every status and flag the GPU tests assert is predicted here, without a GPU.  A random set that turns out to hold a tied
query gets another seed in rmq_cases.RANDOM_SEEDS: the GPU tests tolerate no unexpected hand-back."""
import numpy as np
import pytest

import refbind as rb
import rmq_cases as rc

GROUPS = rc.all_groups()
MIN_CNT, MIN_SC = 3, 20


@pytest.mark.parametrize("g", range(len(GROUPS)), ids=[g.name for g in GROUPS])
def test_forward_pass_sets_are_what_they_claim(g):
    grp = GROUPS[g]
    R = rb.Ref().lib if rb.have_ref() else None
    assert sum(len(c.a) for c in grp.cases) <= 8000
    for c in grp.cases:
        assert (c.a["x"][1:] >= c.a["x"][:-1]).all(), c.name
        f, p, v, ties = rc.host_fwd_runs(c.a, c.cuts, grp.par)
        for r, (beg, end) in enumerate(c.cuts):
            assert 0 < end - beg <= 4096
            bound = rc.inner_bound(c.a, beg, end, grp.par)
            want = c.expect.get(r, 0)
            if want == 0:   # no hand-back expected
                assert ties[r] == 0, (c.name, r, "tied queries: another seed")
                assert bound.max() <= rc.RQ_CAND_MAX, (c.name, r, int(bound.max()))
            elif want == 1:
                assert ties[r] >= 1, (c.name, r)
            else:
                assert bound.max() == rc.RQ_CAND_MAX + 1 and ties[r] == 0, (c.name, r, int(bound.max()))
        if "count" in c.probe:
            i, n = c.probe["count"]
            beg, end = c.cuts[0]
            assert rc.inner_bound(c.a, beg, end, grp.par)[i - beg] == n, c.name
        for i, want_p in c.probe.get("p", {}).items():
            assert p[i] == want_p, (c.name, i, int(p[i]))
        if "tie_run" in c.probe:   # in exactly the intended run
            assert [r for r in range(len(c.cuts)) if ties[r]] == [c.probe["tie_run"]], (c.name, ties)
        if "no_tie_run" in c.probe:
            assert not any(ties), (c.name, ties)
        # the runs are whole groups: run by run equals the read in one piece, and the reference where it is built
        u1, b1 = rc.host_finish(c.a, f, p, v, grp.par.bw, MIN_CNT, MIN_SC)
        u2, b2 = rc.host_chain(c.a, grp.par, MIN_CNT, MIN_SC)
        assert np.array_equal(u1, u2) and np.array_equal(b1, b2), c.name
        if R is not None:
            u3, b3 = rc.ref_chain(R, c.a, grp.par, MIN_CNT, MIN_SC)
            assert np.array_equal(u2, u3) and np.array_equal(b2, b3), c.name


def test_window_lengths_and_equal_x_groups():
    w = rc.window_case()
    for (beg, end), want in zip(w.cuts, rc.WINDOW_LENGTHS):
        ln = rc.outer_window(w.a, beg, end, rc.WIN)
        assert ln.max() == want and ln[-1] == want, (want, int(ln.max()))
    e = rc.equal_x_cases()
    sizes = []
    for beg, end in e.cuts:
        x = e.a["x"][beg:end]
        sizes.append(int(np.unique(x, return_counts=True)[1].max()))
    assert sizes == [1, 2, 64, 65, 200, 70, 1, 1]
    assert [end - beg for beg, end in e.cuts][5:] == [70, 1, 2]
    f, p, v, _ = rc.host_fwd_runs(e.a, e.cuts, rc.WIN, count_ties=False)
    beg, end = e.cuts[5]
    assert (p[beg:end] == -1).all()   # one equal-x group from start to end: no predecessor is ever available
    g = rc.group_boundary_case()
    assert len(g.cuts) == 2 and len(rc.group_cuts(g.a)) == 6
    assert (g.a["x"] >> np.uint64(32) & np.uint64(1)).any() and (g.a["y"] >> np.uint64(40)).any()


def test_skip_cut_and_late_winner_sets_replayed():
    """the inner walk of each purpose-built set's last anchor, replayed in Python (rc.walk_replay) from the host's f and p.  The replay is first proved on every anchor of
    these sets -- it must give the host's f and p -- and then says where the walk is cut (first block, last lane of it, first lane of the second block, later blocks), that
    a non-zero skip counter crosses a block boundary, and that a candidate at position 64 or beyond raises max_f: what k_rmq_fwd carries from block to block"""
    seen_cut, seen_carry, seen_improve = {}, set(), set()
    for grp in rc.cand_groups():
        ms = grp.par.max_skip
        for c in grp.cases:
            if not ({"cut", "improve"} & set(c.probe)):
                continue
            (beg, end), = c.cuts
            f, p, v, ties = rc.host_fwd_runs(c.a, c.cuts, grp.par)
            assert ties == [0]
            for i in range(beg, end):
                w = rc.walk_replay(c.a, f, p, beg, i, grp.par)
                assert (w["f"], w["p"]) == (int(f[i]), int(p[i])), (grp.name, c.name, i)
            assert w["n"] <= rc.RQ_CAND_MAX
            if "cut" in c.probe:
                assert w["cut"] == c.probe["cut"], (grp.name, c.name, w["cut"])
                seen_cut.setdefault(ms, set()).add(w["cut"])
                # the result depends on the cut: the host stops in front of an unmarked, better chain (f = q_span, no predecessor); a walk without the cut takes its top
                z = end - 1
                top = int(np.nonzero((c.a["x"] & np.uint64(0xffffffff)) == np.uint64(8070))[0][0])
                assert (int(f[z]), int(p[z])) == (17, -1), (grp.name, c.name)
                late = rc.walk_replay(c.a, f, p, beg, z, grp.par, drop_cut=True)
                assert late["p"] == top and late["f"] > 17, (grp.name, c.name, late)
                if c.probe["carry"]:   # ... and on the skip counter carried over the block boundary the marked candidates straddle
                    b = c.probe["cut"] - 1 if c.probe["cut"] == 64 else 127
                    assert 0 < w["carry"][b] <= ms, (grp.name, c.name, w["carry"])
                    lost = rc.walk_replay(c.a, f, p, beg, z, grp.par, reset_carry=True)
                    assert lost["p"] == top and lost["f"] > 17, (grp.name, c.name, lost)
                    seen_carry.add((ms, c.probe["cut"]))
            else:
                top = int(np.nonzero((c.a["x"] & np.uint64(0xffffffff)) == np.uint64(8190))[0][0])   # the top of the chain on Z's diagonal
                assert c.probe["improve"] in w["improves"] and int(p[end - 1]) == top, (c.name, w)
                assert w["p"] >= 0 and w["improves"][-1] == c.probe["improve"] >= 64
                seen_improve.add((ms, c.probe["improve"] // 64))
    for ms in rc.CAND_SKIPS:
        assert {63, 64} <= seen_cut[ms] and min(seen_cut[ms]) < 63 and max(seen_cut[ms]) >= 100, (ms, seen_cut)
        assert {(ms, 1), (ms, 2)} <= seen_improve
    assert seen_carry == {(ms, c) for ms in (1, 3, 25) for c in (64, 128)}


def test_cap_sets_bite_the_windows_they_name():
    """window lengths with the cap and without it: cap60_both cuts both windows, cap200_between cuts the outer window and leaves every inner window whole,
    no_inner_cap300 cuts the outer window and has no inner one"""
    free = 1 << 30
    for grp in rc.random_groups():
        name = grp.name.split("/")[1]
        if name not in ("cap60_both", "cap200_between", "no_inner_cap300"):
            continue
        par, cap = grp.par, grp.par.cap
        for c in grp.cases:
            o_free = max(int(rc.outer_window(c.a, b, e, par._replace(cap=free)).max()) for b, e in c.cuts)
            i_free = max(int(rc.inner_window(c.a, b, e, par._replace(cap=free)).max()) for b, e in c.cuts)
            o_cap = max(int(rc.outer_window(c.a, b, e, par).max()) for b, e in c.cuts)
            i_cap = max(int(rc.inner_window(c.a, b, e, par).max()) for b, e in c.cuts)
            jumps = c.name.endswith("/jumps")   # (its windows are cut short by the jumps in x: only cap60 is below them)
            assert (o_free > cap or jumps) and o_cap <= cap + 1, (c.name, o_free, o_cap)
            if name == "cap60_both":
                assert i_free > cap and o_free > cap and i_cap <= cap + 1, (c.name, i_free, i_cap)
            elif name == "cap200_between":
                assert 0 < i_free < cap and i_cap == i_free, (c.name, i_free, i_cap)
            else:
                assert i_free == 0


def test_outer_only_cap_changes_the_result():
    """cap_evicts_the_answer: the cap leaves every inner window whole, cuts the outer one, and the last anchor's predecessor depends on it"""
    grp = rc.cap_evict_group()
    c = grp.cases[1]
    z = c.probe["cap_changes"]
    free = grp.par._replace(cap=1 << 30)
    (beg, end), = c.cuts
    assert rc.inner_window(c.a, beg, end, free).max() < grp.par.cap < rc.outer_window(c.a, beg, end, free).max()
    assert np.array_equal(rc.inner_window(c.a, beg, end, free), rc.inner_window(c.a, beg, end, grp.par))
    f1, p1, _, _ = rc.host_fwd_runs(c.a, c.cuts, grp.par, count_ties=False)
    f0, p0, _, _ = rc.host_fwd_runs(c.a, c.cuts, free, count_ties=False)
    assert (int(p0[z]), int(p1[z])) == (9, -1) and f0[z] > f1[z] == 17


@pytest.fixture(scope="module")
def ora():
    return rb.Oracle()


def test_rescue_sets_are_what_they_claim(ora):
    R = rb.Ref().lib if rb.have_ref() else None
    seen = set()
    for c in rc.rescue_cases(ora):
        u, b, due, u1, b1, s = rc.rescue_recipe(ora, c)
        n_v = int((u1 & np.uint64(0xffffffff)).sum())
        assert due == (c.flag != 0), c.name
        if c.n_v is not None:
            assert n_v == c.n_v and len(u1) > 1, (c.name, n_v)
        if not due:
            continue
        assert n_v <= 4096
        seen.add(n_v <= rc.LC_RQ_LDS)
        par = rc.rescue_par(c.rescue)
        _, _, _, ties = rc.host_fwd_runs(s, [(0, len(s))], par)
        bound = rc.inner_bound(s, 0, len(s), par, with_cap=False)
        if "count" in c.probe:
            (xz, yz), n = c.probe["count"]
            i = int(np.nonzero(((s["x"] & np.uint64(0xffffffff)) == np.uint64(xz)) & ((s["y"] & np.uint64(0xffffffff)) == np.uint64(yz)))[0][0])
            assert bound[i] == n, (c.name, int(bound[i]))
        if c.flag == 1:
            assert ties[0] == 0 and bound.max() <= rc.LC_CAND_MAX and n_v <= par.cap, (c.name, ties, int(bound.max()))
        elif "tie" in c.probe:
            assert ties[0] >= 1, c.name
        elif "count" in c.probe:
            assert c.probe["count"][1] == rc.LC_CAND_MAX + 1 and ties[0] == 0
        else:
            assert n_v == par.cap + 1
        if R is not None and c.flag == 1:
            u3, b3 = rc.ref_chain(R, s, par, c.rescue["min_cnt"], c.rescue["min_sc"])
            assert np.array_equal(u, u3) and np.array_equal(b, b3), c.name
    assert seen == {True, False}
