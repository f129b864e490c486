"""CPU-only checks behind the low-memory WFA rung (k_wfa_seg.hip).

* The premise: the unmodified reference's mwf_wfa_exact() gives the score and CIGAR of its full mode (step = 0) for EVERY step, so the device
  may choose its own step and the oracle's exact WFA is the expected value of the device tests.
* mga.wfa_seg_bytes(): the workspace formula of include/minigraph_amd.h, restated here part by part.
"""
import ctypes as C

import numpy as np
import pytest

import minigraph_amd as mga
import refbind as rb
import wfa_seg_cases as wc


def _ref_exact():
    lib = C.CDLL(rb.REF_SO)
    libc = C.CDLL(None)
    lib.mwf_opt_init.argtypes = [C.POINTER(rb.mwf_opt_t)]
    lib.mwf_wfa_exact.argtypes = [C.c_void_p, C.POINTER(rb.mwf_opt_t), C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, C.POINTER(rb.mwf_rst_t)]
    lib.mwf_wfa_exact.restype = None
    libc.free.argtypes = [C.c_void_p]

    def run(ts, qs, step):
        opt = rb.mwf_opt_t()
        lib.mwf_opt_init(C.byref(opt))
        opt.flag |= 1  # MWF_F_CIGAR
        opt.step, opt.max_iter = step, -1
        r = rb.mwf_rst_t()
        lib.mwf_wfa_exact(None, C.byref(opt), len(ts), ts, len(qs), qs, C.byref(r))
        cig = np.ctypeslib.as_array(r.cigar, shape=(r.n_cigar,)).astype("<u4") if r.n_cigar else np.zeros(0, "<u4")
        if r.cigar:
            libc.free(r.cigar)
        return r.s, cig

    return run


@pytest.mark.skipif(not rb.have_ref(), reason="oracle/_ref/libmgref.so is not built")
def test_reference_low_memory_mode_equals_full_mode_for_every_step():
    run = _ref_exact()
    T, Q = wc.base_pairs()
    full = [run(t, q, 0) for t, q in zip(T, Q)]
    for step in wc.STEPS:
        for i, (t, q) in enumerate(zip(T, Q)):
            s, c = run(t, q, step)
            assert s == full[i][0], (step, i)
            assert np.array_equal(c, full[i][1]), (step, i)
        for t, q, target in wc.checkpoint_pairs(step):
            s0, c0 = run(t, q, 0)
            s, c = run(t, q, step)
            assert s0 == target and s == s0 and np.array_equal(c, c0), (step, target)


# ---- the workspace formula (include/minigraph_amd.h), with miniwfa's default penalties x = 4, o1 = 4, e1 = 2, o2 = 15, e2 = 1 ----

def _parts(tl, ql, step):
    W = tl + ql + 1
    mn, g = min(tl, ql), abs(tl - ql)
    S = min(2 * 15 + (tl + ql), 4 * mn + (0 if g == 0 else min(4 + 2 * g, 15 + g)))

    def B(s):
        return min(W, 2 * s + 1)

    n = S // step
    snap = 0
    for j in range(n):
        top = (j + 1) * step - 1
        snap += sum(B(s) for s in range(max(0, top - 16), top + 1))
    s = np.arange(1, S + 1, dtype=np.int64)
    T = np.minimum(W, 2 * s + 1)
    if step >= 17:
        T = np.where(s >= step, np.minimum(T, 2 * (s % step + 17) + 1), T)
    return {"rows": 12 * (S + 1), "rings": 2 * 340 * B(S), "cigar": 4 * (W + 1), "headers": 160 * n, "snapshots": 20 * snap, "traceback": 1 + int(T.sum())}


@pytest.mark.parametrize("tl,ql", [(1, 1), (1, 300), (300, 1), (1500, 1500), (100, 1500), (9000, 12000), (150000, 150000)])
def test_wfa_seg_bytes_is_the_sum_of_its_documented_parts(tl, ql):
    for step in (5000, 17, 16, 256):
        if step < 256 and tl + ql > 30000:
            continue  # (tens of thousands of snapshots: slow to restate in Python, nothing new)
        want = (sum(_parts(tl, ql, step).values()) + 255) // 256 * 256
        assert mga.wfa_seg_bytes(tl, ql, step) == want, (tl, ql, step)


def test_wfa_seg_bytes_grows_with_the_problem_and_stays_below_the_old_tier():
    sizes = [(1, 1), (1, 2), (2, 2), (10, 10), (10, 300), (300, 300), (300, 2000), (2000, 2000), (2000, 30000), (30000, 30000), (30000, 200000), (200000, 200000),
             (200000, 400000), (400000, 400000)]
    for step in (0, 5000):
        got = [mga.wfa_seg_bytes(tl, ql, step) for tl, ql in sizes]
        assert all(b > 0 for b in got)
        assert all(x <= y for x, y in zip(got, got[1:])), (step, got)
    same = [mga.wfa_seg_bytes(n, n, 0) for n in (100, 1000, 10000, 100000, 400000)]  # along tl = ql, tl + ql alone orders the problems
    assert all(x <= y for x, y in zip(same, same[1:]))
    # the host's step is the one of least memory: never worse than the reference's 5000, and a 400 kb x 400 kb gap stays under the 32 GiB the last HBM tier holds
    assert mga.wfa_seg_bytes(400000, 400000, 0) <= mga.wfa_seg_bytes(400000, 400000, 5000)
    assert mga.wfa_seg_bytes(400000, 400000, 0) < 32 << 30
    assert mga.wfa_seg_step(400000, 400000) >= 17
    assert mga.wfa_seg_bytes(0, 5, 0) < 0
