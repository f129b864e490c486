"""GPU stage tests of the three device forms of the RMQ chainer's forward pass -- k_rmq_fwd (k_rmq.hip), lc_dp_rmq_lds and lc_dp_rmq (the long-join rescue inside
k_lchain) -- and of their hand-backs, through the C ABI on the seeded sets of rmq_cases.py, bit for bit against the host tree of rmq.c (pinned to the reference's
mg_lchain_rmq by test_host_rmq.py).  Every status and flag asserted here is predicted on the CPU by test_rmq_cases_host.py."""
import faulthandler
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import minigraph_amd as mga
import refbind as rb
import rmq_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def time_limit():
    """every test here under its own limit: a persistent-wavefront kernel that never ends would otherwise hold the whole run (the dump names the test; the process exits)"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()

GROUPS = rc.all_groups()
MIN_CNT, MIN_SC = 3, 20


@functools.lru_cache(maxsize=None)
def host_of(g):
    """the host's forward pass over every read of a group, computed once"""
    return [rc.host_fwd_runs(c.a, c.cuts, GROUPS[g].par, count_ties=False)[:3] for c in GROUPS[g].cases]


def check_launch(g, f, p, v, status, where):
    grp = GROUPS[g]
    for (c, r0, abs0), (hf, hp, hv) in zip(where, host_of(g)):
        for r, (beg, end) in enumerate(c.cuts):
            st = int(status[r0 + r])
            assert st != 4, (c.name, r, "the kernel never took this run")
            assert st == c.expect.get(r, 0), (grp.name, c.name, r, st)
            if st == 0:
                s = slice(abs0 + beg, abs0 + end)
                assert np.array_equal(f[s], hf[beg:end]), (grp.name, c.name, r, "f")
                assert np.array_equal(p[s], hp[beg:end]), (grp.name, c.name, r, "p")   # relative to the read's first anchor
                assert np.array_equal(v[s], hv[beg:end]), (grp.name, c.name, r, "v")


@pytest.mark.parametrize("g", range(len(GROUPS)), ids=[g.name for g in GROUPS])
def test_rmq_fwd_equals_host_tree_and_hands_back_what_it_must(g):
    """one launch per group, many runs of several reads each: status 0 and f / p / v equal to the host wherever no tie at a minimum and at most 512 inner candidates are
    predicted, 1 for the forced ties, 2 for 513 candidates, never 4; the neighbours of a handed-back run -- same read and other reads -- are untouched.  Then the pipeline's
    recipe: the handed-back runs redone by the host inside the device's arrays, backtracked: the read's chains equal mga_lchain_rmq's (and the reference's)."""
    grp = GROUPS[g]
    a, runs, where = rc.launch(grp)
    f, p, v, status = mga.rmq_fwd_batch(a, runs, **grp.par._asdict())
    check_launch(g, f, p, v, status, where)
    R = rb.Ref().lib if rb.have_ref() else None
    for c, r0, abs0 in where:
        n = len(c.a)
        df, dp, dv = f[abs0:abs0 + n].copy(), p[abs0:abs0 + n].copy(), v[abs0:abs0 + n].copy()
        redo = {r for r in range(len(c.cuts)) if status[r0 + r] != 0}
        if redo:
            rc.host_fwd_runs(c.a, c.cuts, grp.par, df, dp, dv, only=redo, count_ties=False)
        u1, b1 = rc.host_finish(c.a, df, dp, dv, grp.par.bw, MIN_CNT, MIN_SC)
        u2, b2 = rc.host_chain(c.a, grp.par, MIN_CNT, MIN_SC)
        assert np.array_equal(u1, u2) and np.array_equal(b1, b2), (grp.name, c.name)
        if R is not None:
            u3, b3 = rc.ref_chain(R, c.a, grp.par, MIN_CNT, MIN_SC)
            assert np.array_equal(u1, u3) and np.array_equal(b1, b3), (grp.name, c.name)


def test_rmq_fwd_launch_order_does_not_matter():
    """table order (order = NULL), longest first as the pipeline lists them, reversed: identical results"""
    g = 0
    a, runs, where = rc.launch(GROUPS[g])
    par = GROUPS[g].par._asdict()
    base = mga.rmq_fwd_batch(a, runs, **par)
    check_launch(g, *base, where)
    longest = np.argsort(-(runs[:, 1] - runs[:, 0]), kind="stable").astype(np.int32)
    for order in (longest, np.arange(len(runs), dtype=np.int32)[::-1].copy()):
        got = mga.rmq_fwd_batch(a, runs, order=order, **par)
        handed = np.repeat(base[3] != 0, runs[:, 1] - runs[:, 0]) if len(runs) else np.zeros(0, bool)   # (what a handed-back run left behind is nobody's result)
        assert np.array_equal(got[3], base[3])
        for x, y in zip(got[:3], base[:3]):
            assert np.array_equal(x[~handed], y[~handed])


def test_rmq_fwd_empty_chunk_and_untouched_runs():
    f, p, v, status = mga.rmq_fwd_batch(np.zeros(0, rc.M128), np.zeros((0, 3), np.int64))
    assert len(f) == 0 and len(status) == 0
    a, runs, where = rc.launch(GROUPS[0])
    f, p, v, status = mga.rmq_fwd_batch(a, runs, order=np.array([1, 0], dtype=np.int32), **GROUPS[0].par._asdict())
    assert (status[:2] != 4).all() and (status[2:] == 4).all()   # a run the launch did not list is visible as such


def test_rmq_fwd_queue_refill():
    """MGA_RMQ_WAVES=3: about 40 runs through three persistent wavefronts -- every wave refills many times, the queue runs dry"""
    env = dict(os.environ, MGA_RMQ_WAVES="3")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "rmq_waves_child.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    assert p.returncode == 0 and b"REFILL-OK" in p.stdout, (p.stdout[-500:], p.stderr[-2000:])


# ---------------------------------------------------------------- the long-join rescue inside k_lchain

@pytest.fixture(scope="module")
def ora():
    return rb.Oracle()


@pytest.fixture(scope="module")
def rescue(ora):
    """the reads and, once, what the host recipe makes of each"""
    cs = rc.rescue_cases(ora)
    return cs, [rc.rescue_recipe(ora, c) for c in cs]


def check_rescue(c, want, got):
    u, b, flag = got
    wu, wb, due, u1, b1, _ = want
    assert flag == c.flag, (c.name, flag)
    if flag == 2:   # handed back: the first pass's chains, bit for bit (the keep / keep_u restore, n_u included)
        wu, wb = u1, b1
    assert len(u) == len(wu) and np.array_equal(u, wu), (c.name, "u")
    assert np.array_equal(b, wb), (c.name, "b")


@pytest.mark.parametrize("win", ["0", "1"])
def test_lchain_rescue_read_by_read(rescue, win, monkeypatch):
    """chained-anchor counts around both forms of the rescue's DP and their seam, the condition's boundaries, and every hand-back (tie, 65 candidates, n_v = cap + 1) in
    both forms: the flag, and (u, b) equal to the host recipe -- or, handed back, to the first pass"""
    monkeypatch.setenv("MGA_LC_WIN", win)
    cs, want = rescue
    for c, w in zip(cs, want):
        got = mga.lchain_batch([c.a], rescue=c.rescue, qlens=[c.qlen], **rc.first_kw(c))
        check_rescue(c, w, got[0])


@pytest.mark.parametrize("win", ["0", "1"])
def test_lchain_rescue_mixed_batch(rescue, ora, win, monkeypatch):
    """reads that share the parameters in one launch: the default parameters hold every n_v, the tie and the 64 / 65-candidate reads of both forms and a read with one
    chain -- flags 0, 1 and 2 of every kind side by side; every read has its own flag and its own result"""
    monkeypatch.setenv("MGA_LC_WIN", win)
    cs, want = rescue
    key = lambda c: (tuple(sorted(c.rescue.items())), tuple(sorted(rc.first_kw(c).items())))
    n_batches = 0
    for k in sorted({key(c) for c in cs}):
        idx = [i for i, c in enumerate(cs) if key(c) == k]
        if len(idx) < 2:
            continue
        n_batches += 1
        got = mga.lchain_batch([cs[i].a for i in idx], rescue=cs[idx[0]].rescue, qlens=[cs[i].qlen for i in idx], **rc.first_kw(cs[idx[0]]))
        for i, gt in zip(idx, got):
            check_rescue(cs[i], want[i], gt)
    assert n_batches >= 1
    dflt = [c for c in cs if c.rescue == rc.RESCUE]
    assert {c.flag for c in dflt} == {0, 1, 2} and sum("tie" in c.probe for c in dflt) == 2 and sum("count" in c.probe for c in dflt) == 4
    # a read handed back for its size (n_v = cap + 1) between reads the same cap lets through and a read with one chain
    by = {c.name: i for i, c in enumerate(cs)}
    idx = [by["n_v=63"], by["cap=n_v-1/n_v=120"], by["condition/one_chain"], by["n_v=65"], by["cap=n_v-1/n_v=120"]]
    got = mga.lchain_batch([cs[i].a for i in idx], rescue=cs[idx[1]].rescue, qlens=[cs[i].qlen for i in idx], **rc.FIRST)
    assert [gt[2] for gt in got] == [1, 2, 0, 1, 2]
    for i, gt in zip(idx, got):
        check_rescue(cs[i], want[i], gt)
