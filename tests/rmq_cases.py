"""Seeded anchor sets for the device forms of the RMQ chainer's forward pass (k_rmq.hip: k_rmq_fwd; k_lchain.hip: lc_dp_rmq_lds, lc_dp_rmq) and the host-side
predictors that say, without a GPU, what each set makes the kernels do: test_rmq_cases_host.py proves the sets are what test_gpu_rmq.py assumes.

A `Case` is one read: its x-sorted anchors, its runs (whole (segment, strand) groups) and, per run, the status the kernel must report (0 unless listed).  A `Group` is
one launch: reads that share the chainer's parameters.  The reference of every comparison is the host tree of rmq.c (mga_lchain_rmq_fwd, mga_lchain_rmq), which
test_host_rmq.py pins to the reference's mg_lchain_rmq."""
import ctypes as C
from collections import namedtuple

import numpy as np

import minigraph_amd as mga

M128 = mga.m128
Par = namedtuple("Par", "max_dist max_dist_inner bw max_skip cap pen_gap pen_skip")
RQ_CAND_MAX, LC_CAND_MAX, LC_RQ_LDS = 512, 64, 336

# the six parameter tuples of test_host_rmq.py and the window parameters the issue lists
PARS = {
    "asm": Par(10000, 1000, 2000, 25, 100000, 0.8, 0.05),
    "lr_rescue": Par(5000, 1000, 20000, 25, 100000, 0.8, 0.05),
    "no_inner_cap300": Par(3000, 0, 500, 5, 300, 0.8, 0.05),            # max_dist_inner = 0; a cap that bites the outer window only
    "cap60_both": Par(10000, 1000, 2000, 25, 60, 0.8, 0.05),            # a cap that bites both windows
    "cap200_between": Par(4000, 600, 2000, 3, 200, 0.8, 0.05),          # a cap between the two windows' sizes: it bites the outer window, the inner one stays whole
    "narrow_inner": Par(10000, 150, 2000, 25, 100000, 0.8, 0.05),
    "inner_eq_outer": Par(2000, 2000, 1000, 25, 100000, 0.8, 0.05),     # max_dist_inner >= max_dist: no inner window
    "inner_gt_outer": Par(2000, 5000, 1000, 1, 100000, 0.8, 0.05),
    "dist_lt_bw": Par(300, 100, 2000, 25, 100000, 0.8, 0.05),           # max_dist < bw: the band is the distance
}
WIN = Par(3000, 300, 1000, 25, 100000, 0.8, 0.05)                      # window lengths, equal-x groups, keys, ties
WINDOW_LENGTHS = (1, 63, 64, 65, 191, 192, 193, 255, 256, 257, 300, 1000)
CAND_COUNTS = (0, 1, 63, 64, 65, 128, 129, 511, 512, 513)
CAND_SKIPS = (0, 1, 3, 25)


def cand_par(max_skip):
    return Par(10000, 4000, 2000, max_skip, 100000, 0.8, 0.05)


class Case:
    def __init__(self, name, a, cuts=None, expect=None, merge=1, probe=None):
        self.name, self.a = name, np.ascontiguousarray(a, dtype=M128)
        self.cuts = group_cuts(self.a, merge) if cuts is None else cuts
        self.expect = expect or {}   # run index -> status
        self.probe = probe or {}     # what the host test looks at: {"count": (anchor, n)}, {"p": {anchor: p}}, {"tie_run": run}


Group = namedtuple("Group", "name par cases")


def mk(x, y, span=17, seg=0, strand=0, flags=None):
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    assert (x >= 0).all() and (x < 2 ** 31).all() and (y >= 0).all() and (y < 2 ** 31).all()
    a = np.zeros(len(x), dtype=M128)
    a["x"] = (np.uint64(seg) << np.uint64(33)) | (np.uint64(strand) << np.uint64(32)) | x.astype(np.uint64)
    a["y"] = (np.uint64(span) << np.uint64(32)) | y.astype(np.uint64)
    if flags is not None:   # seed flag bits above bit 40: the chainers only ever read (int32_t)y and y >> 32 & 0xff
        a["y"] |= np.asarray(flags, dtype=np.uint64) << np.uint64(40)
    return a


def xsort(a):
    return a[np.argsort(a["x"], kind="stable")]


def group_cuts(a, merge=1):
    """runs of `merge` whole (segment, strand) groups each"""
    if len(a) == 0:
        return []
    g = a["x"] >> np.uint64(32)
    b = [0] + [int(i) for i in np.nonzero(g[1:] != g[:-1])[0] + 1] + [len(a)]
    b = b[:-1][::merge] + [len(a)]
    return [(b[i], b[i + 1]) for i in range(len(b) - 1)]


# ---------------------------------------------------------------- the host side: reference and predictors

def _lib():
    L = mga.load()
    L.mga_lchain_rmq_fwd.restype = None
    L.mga_lchain_rmq_fwd.argtypes = [C.c_int] * 5 + [C.c_float, C.c_float, C.c_int64, C.c_int64] + [C.c_void_p] * 5
    L.mga_lchain_rmq_finish2.restype = C.c_void_p
    L.mga_lchain_rmq_finish2.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64] + [C.c_void_p] * 5 + [C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_int]
    L.mga_lchain_rmq.restype = C.c_void_p
    L.mga_lchain_rmq.argtypes = [C.c_int] * 7 + [C.c_float, C.c_float, C.c_int64, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
    L.mga_rq_tie_stats_enable.argtypes = [C.c_int]
    L.mga_rq_tie_stats_enable.restype = None
    L.mga_rq_tie_stats.argtypes = [C.c_void_p, C.c_int]
    L.mga_rq_tie_stats.restype = None
    L.mga_ksort_128x.argtypes = [C.c_int64, C.c_void_p]
    L.mga_ksort_128x.restype = None
    return L


def _take_chains(r, u, nu):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    uu = np.ctypeslib.as_array(C.cast(u, C.POINTER(C.c_uint64)), shape=(nu,)).copy() if nu else np.zeros(0, np.uint64)
    n_b = int((uu & np.uint64(0xffffffff)).sum())
    b = np.frombuffer(C.string_at(r, n_b * 16), dtype=M128).copy() if n_b else np.zeros(0, M128)
    libc.free(r)
    libc.free(u)
    return uu, b


def host_fwd_runs(a, cuts, par, f=None, p=None, v=None, only=None, count_ties=True):
    """mga_lchain_rmq_fwd over each run of one read (its own t slice zeroed, as rq_dev_worker does) -> f, p (absolute in the read), v and the host's tied-query count per run.
    only: redo these runs inside the arrays given (the pipeline's recipe for what the device handed back)."""
    L = _lib()
    n = len(a)
    f = np.zeros(n, np.int32) if f is None else f
    p = np.full(n, -1, np.int64) if p is None else p
    v = np.zeros(n, np.int32) if v is None else v
    t = np.zeros(n, np.int32)
    ties = []
    out = np.zeros(8, np.int64)
    for r, (beg, end) in enumerate(cuts):
        if only is not None and r not in only:
            ties.append(None)
            continue
        t[beg:end] = 0
        if count_ties:
            L.mga_rq_tie_stats_enable(1)
            L.mga_rq_tie_stats(out.ctypes.data, 1)
        L.mga_lchain_rmq_fwd(par.max_dist, par.max_dist_inner, par.bw, par.max_skip, par.cap, par.pen_gap, par.pen_skip, beg, end,
                             a.ctypes.data, f.ctypes.data, p.ctypes.data, v.ctypes.data, t.ctypes.data)
        if count_ties:
            L.mga_rq_tie_stats(out.ctypes.data, 1)
            L.mga_rq_tie_stats_enable(0)
            ties.append(int(out[5]))
        else:
            ties.append(None)
    return f, p, v, ties


def host_finish(a, f, p, v, bw, min_cnt, min_sc):
    """backtrack + compaction over the whole read (mga_lchain_rmq_finish2; the arrays stay the caller's) -> (u, b)"""
    L = _lib()
    f, p, v = f.copy(), p.copy(), v.copy()
    t = np.zeros(len(a), np.int32)
    nu, u = C.c_int(0), C.c_void_p()
    r = L.mga_lchain_rmq_finish2(bw, min_cnt, min_sc, len(a), a.ctypes.data, f.ctypes.data, p.ctypes.data, v.ctypes.data, t.ctypes.data, C.byref(nu), C.byref(u), 1)
    return _take_chains(r, u, nu.value)


def host_chain(a, par, min_cnt, min_sc):
    """mga_lchain_rmq over one read -> (u, b)"""
    L = _lib()
    if len(a) == 0:
        return np.zeros(0, np.uint64), np.zeros(0, M128)
    nu, u = C.c_int(0), C.c_void_p()
    r = L.mga_lchain_rmq(par.max_dist, par.max_dist_inner, par.bw, par.max_skip, par.cap, min_cnt, min_sc, par.pen_gap, par.pen_skip, len(a), a.ctypes.data,
                         C.byref(nu), C.byref(u))
    return _take_chains(r, u, nu.value)


def ref_chain(R, a, par, min_cnt, min_sc):
    """the reference's mg_lchain_rmq (it frees its input: a malloc'ed copy)"""
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    buf = libc.malloc(max(len(a), 1) * 16)
    C.memmove(buf, a.ctypes.data, len(a) * 16)
    R.mg_lchain_rmq.restype = C.c_void_p
    R.mg_lchain_rmq.argtypes = [C.c_int] * 7 + [C.c_float, C.c_float, C.c_int64, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_void_p]
    nu, u = C.c_int(0), C.c_void_p()
    r = R.mg_lchain_rmq(par.max_dist, par.max_dist_inner, par.bw, par.max_skip, par.cap, min_cnt, min_sc, par.pen_gap, par.pen_skip, len(a), buf, C.byref(nu), C.byref(u), None)
    return _take_chains(r, u, nu.value)


def ksort(a):
    a = np.ascontiguousarray(a.copy())
    _lib().mga_ksort_128x(len(a), a.ctypes.data)
    return a


def inner_bound(a, beg, end, par, with_cap=True):
    """upper bound of the inner walk's candidates per anchor of the run [beg, end): the j in [st_in, i0) with y_i - inner <= y_j <= y_i - 1 (the walk itself only happens
    when the range-minimum query has an inexact answer).  The windows move as in lchain.c:279-312; with_cap=False: without the size clause (the rescue in k_lchain)."""
    max_dist, inner = max(par.max_dist, par.bw), par.max_dist_inner
    if inner <= 0 or inner >= max_dist:
        return np.zeros(end - beg, np.int64)
    x, y = a["x"], a["y"].astype(np.int64).astype(np.int32).astype(np.int64)   # (int32_t)y
    hi = a["x"] >> np.uint64(32)
    out = np.zeros(end - beg, np.int64)
    i0 = st_in = beg
    for i in range(beg, end):
        if i0 < i and x[i0] != x[i]:
            i0 = i
        while st_in < i and (hi[i] != hi[st_in] or int(x[i]) > int(x[st_in]) + inner or (with_cap and max(i0 - st_in, 0) > par.cap)):
            st_in += 1
        if st_in < i0:
            w = y[st_in:i0]
            out[i - beg] = int(((w <= y[i] - 1) & (w >= y[i] - inner)).sum())
    return out


def outer_window(a, beg, end, par):
    """length of the range-minimum query's window [st, i0) per anchor of the run (lchain.c:279-302)"""
    max_dist = max(par.max_dist, par.bw)
    x, hi = a["x"], a["x"] >> np.uint64(32)
    out = np.zeros(end - beg, np.int64)
    i0 = st = beg
    for i in range(beg, end):
        if i0 < i and x[i0] != x[i]:
            i0 = i
        while st < i and (hi[i] != hi[st] or int(x[i]) > int(x[st]) + max_dist or max(i0 - st, 0) > par.cap):
            st += 1
        out[i - beg] = max(i0 - st, 0)
    return out


def inner_window(a, beg, end, par):
    """length of the inner walk's window [st_in, i0) per anchor of the run (lchain.c:303-312); 0 where there is no inner window"""
    max_dist, inner = max(par.max_dist, par.bw), par.max_dist_inner
    out = np.zeros(end - beg, np.int64)
    if inner <= 0 or inner >= max_dist:
        return out
    x, hi = a["x"], a["x"] >> np.uint64(32)
    i0 = st_in = beg
    for i in range(beg, end):
        if i0 < i and x[i0] != x[i]:
            i0 = i
        while st_in < i and (hi[i] != hi[st_in] or int(x[i]) > int(x[st_in]) + inner or max(i0 - st_in, 0) > par.cap):
            st_in += 1
        out[i - beg] = max(i0 - st_in, 0)
    return out


def _log2f(x):
    """mga_log2f (mga_host.h; the reference's mg_log2), operation for operation in single precision"""
    z = np.array([x], dtype=np.float32).view(np.uint32)
    r = np.float32(int(z[0] >> 23 & 255) - 128)
    z[0] = (z[0] & np.uint32(0x807fffff)) + np.uint32(127 << 23)
    zf = z.view(np.float32)[0]
    return r + ((np.float32(-0.34484843) * zf + np.float32(2.02466578)) * zf - np.float32(0.67487759))


def score_simple(xi, yi, xj, yj, span_j, par):
    """lchain.c:234-250 -> (score, exact, width); positions are the 32-bit ones"""
    dq, dr = yi - yj, xi - xj
    dd = abs(dr - dq)
    dg = min(dr, dq)
    sc = min(span_j, dg)
    if dd or dq > span_j:
        lin = np.float32(par.pen_gap) * np.float32(dd) + np.float32(par.pen_skip) * np.float32(dg)
        lg = _log2f(np.float32(dd + 1)) if dd >= 1 else np.float32(0)
        sc -= int(lin + np.float32(.5) * lg)
    return sc, dd == 0 and dg <= span_j, dd


def walk_replay(a, f, p, beg, i, par, drop_cut=False, reset_carry=False):
    """the chaining of anchor i of the run that starts at beg, replayed from the host's f and p of the anchors before it: the range-minimum query by brute force (its
    minimum must be unique), then the inner walk in descending (y, index) order with the skip heuristic (lchain.c:313-350).  Positions count the candidates of the inner
    window in visiting order, as the kernels' blocks of 64 do.  -> dict(f, p: the result for anchor i; n: candidates; cut: position where the walk was cut (None: never);
    improves: positions that raised max_f; carry: {position: n_skip} after the last candidate of each block the walk went past).
    Two deliberately wrong walks show that a set's RESULT depends on the cut: drop_cut never cuts, reset_carry forgets the skip counter at every block boundary."""
    max_dist, inner = max(par.max_dist, par.bw), par.max_dist_inner
    if inner <= 0 or inner >= max_dist:
        inner = 0
    x64, hi = a["x"], a["x"] >> np.uint64(32)
    x = (a["x"] & np.uint64(0xffffffff)).astype(np.int64)
    y = a["y"].astype(np.int64).astype(np.int32).astype(np.int64)
    span = (a["y"] >> np.uint64(32) & np.uint64(0xff)).astype(np.int64)
    i0 = st = st_in = beg
    for k in range(beg, i + 1):
        if i0 < k and x64[i0] != x64[k]:
            i0 = k
        while st < k and (hi[k] != hi[st] or int(x64[k]) > int(x64[st]) + max_dist or max(i0 - st, 0) > par.cap):
            st += 1
        while inner and st_in < k and (hi[k] != hi[st_in] or int(x64[k]) > int(x64[st_in]) + inner or max(i0 - st_in, 0) > par.cap):
            st_in += 1
    out = dict(f=int(span[i]), p=-1, n=0, cut=None, improves=[], carry={})
    q = [j for j in range(st, i0) if (y[i] - max_dist < y[j] < y[i] - 1) or (j == 0 and y[j] == y[i] - 1)]
    if not q:
        return out
    half = 0.5 * float(np.float32(par.pen_gap))
    pri = [-(float(f[j]) + half * float(int(np.int32(x[j])) + int(y[j]))) for j in q]
    assert pri.count(min(pri)) == 1, "tied minimum"
    jq = q[pri.index(min(pri))]
    sc, exact, width = score_simple(x[i], y[i], x[jq], y[jq], span[jq], par)
    sc += int(f[jq])
    if width <= par.bw and sc > out["f"]:
        out["f"], out["p"] = sc, jq
    if exact or not inner or not st_in < i0 or y[i] <= 0:
        return out
    cand = sorted((j for j in range(st_in, i0) if y[i] - inner <= y[j] <= y[i] - 1), key=lambda j: (-y[j], -j))
    out["n"] = len(cand)
    mark, n_skip = set(), 0
    for k, j in enumerate(cand):
        sc, _, width = score_simple(x[i], y[i], x[j], y[j], span[j], par)
        sc += int(f[j])
        if width <= par.bw:
            if sc > out["f"]:
                out["f"], out["p"] = sc, j
                out["improves"].append(k)
                if n_skip > 0:
                    n_skip -= 1
            elif j in mark:
                n_skip += 1
                if n_skip > par.max_skip and not drop_cut:
                    out["cut"] = k
                    break
            if p[j] >= 0:
                mark.add(int(p[j]))
        if k % 64 == 63 and k + 1 < len(cand):
            out["carry"][k] = n_skip
            if reset_carry:
                n_skip = 0
    return out


# ---------------------------------------------------------------- sets for k_rmq_fwd

def random_anchors(rng, n, kind):
    """the four kinds of test_host_rmq.py, a few hundred anchors each; "jumps" changes the (segment, strand) group every few hundred anchors"""
    gaps = rng.integers(1, 12, n).astype(np.int64)
    x = np.cumsum(gaps) + 17
    if kind == "colinear":
        y = x + 100 + np.cumsum((rng.random(n) < 0.01) * rng.integers(-30, 30, n))
    elif kind == "noisy":
        y = x + 100 + np.cumsum((rng.random(n) < 0.03) * rng.integers(-200, 200, n))
        y = np.where(rng.random(n) < 0.1, rng.integers(20, x[-1] + 1000, n), y)
        x = np.where(rng.random(n) < 0.05, np.roll(x, 1), x)
        x[0] = 17
        x = np.sort(x)
    elif kind == "dense":
        x = np.sort(rng.integers(17, 4 * n, n))
        y = x + 100 + np.where(rng.random(n) < 0.5, rng.integers(-400, 400, n), 0)
    else:
        y = x + 100 + np.cumsum((rng.random(n) < 0.01) * rng.integers(-3000, 3000, n))
        x = x + np.cumsum((rng.random(n) < 0.01) * rng.integers(0, 9000, n))
        x = x + (np.cumsum(rng.random(n) < 0.004).astype(np.int64) << 32)   # strand and segment bits
    y = np.clip(y, 17, None)
    seen = set()   # equal x + y with equal f is a tie of priorities: off-diagonal hits move up until their x + y is theirs alone
    for i in range(n):
        while int(x[i] & 0xffffffff) + int(y[i]) in seen:
            y[i] += 1
        seen.add(int(x[i] & 0xffffffff) + int(y[i]))
    a = np.zeros(n, dtype=M128)
    a["x"] = x.astype(np.uint64)
    a["y"] = (np.uint64(17) << np.uint64(32)) | y.astype(np.uint64)
    if kind == "noisy":
        a["y"] |= rng.integers(0, 1 << 20, n).astype(np.uint64) << np.uint64(40)
    return xsort(a)


RANDOM_SEEDS = {}   # (parameter set, kind) -> seed, where the default seed gave a set with a tied query (test_rmq_cases_host.py says so)


def random_groups():
    out = []
    for k, (pname, par) in enumerate(PARS.items()):
        cases = []
        for q, kind in enumerate(("colinear", "noisy", "jumps", "dense")):
            rng = np.random.default_rng(RANDOM_SEEDS.get((pname, kind), 1000 + 10 * k + q))
            a = random_anchors(rng, int(rng.integers(250, 700)), kind)
            cases.append(Case("%s/%s" % (pname, kind), a, merge=2 if kind == "jumps" else 1))
        out.append(Group("random/" + pname, par, cases))
    return out


def _diag(rng, x0, y0, n, step=(1, 3), indel=0.05):
    """n anchors along a diagonal with distinct x, small steps and a few indels"""
    x = x0 + np.cumsum(rng.integers(step[0], step[1], n))
    y = y0 + (x - x0) + np.cumsum((rng.random(n) < indel) * rng.integers(-20, 20, n))
    return x, np.clip(y, 1, None)


def window_case():
    """one (segment, strand) group = one run per length L: L + 1 anchors with distinct x inside max_dist of each other, so the window [st, i0) of its last anchor is L long and
    those of the anchors before it are 1 .. L - 1"""
    rng = np.random.default_rng(21)
    parts = []
    for g, Lw in enumerate(WINDOW_LENGTHS):
        x, y = _diag(rng, 50, 400, Lw + 1)
        assert x[-1] - x[0] <= WIN.max_dist
        parts.append(mk(x, y, seg=g))
    return Case("window_lengths", np.concatenate(parts))


def equal_x_cases():
    rng = np.random.default_rng(22)
    parts = []
    for g, m in enumerate((1, 2, 64, 65, 200)):   # a group of m anchors with one x between two diagonals: i0 lags i inside it
        x1, y1 = _diag(rng, 100, 300, 12)
        xe = np.full(m, x1[-1] + 5)
        ye = y1[-1] + 5 + 3 * np.arange(m)
        x2, y2 = _diag(rng, int(xe[0]) + 3, int(ye[-1]) + 3, 12)
        parts.append(mk(np.concatenate([x1, xe, x2]), np.concatenate([y1, ye, y2]), seg=g))
    parts.append(mk(np.full(70, 500), 900 + 2 * np.arange(70), seg=5))       # a run that is one equal-x group: no predecessor is ever available
    parts.append(mk([700], [800], seg=6))                                    # a run of one anchor
    parts.append(mk([700, 710], [800, 810], seg=7))                          # ... of two
    return Case("equal_x", np.concatenate(parts))


def group_boundary_case():
    """six small groups -- segment and strand bits -- in runs of three, flag bits above bit 40 of y: the windows are emptied at every change inside a run"""
    rng = np.random.default_rng(23)
    parts = []
    for g in range(6):
        n = int(rng.integers(30, 90))
        x, y = _diag(rng, 40, 200 if g % 2 else 60, n, step=(1, 9))
        parts.append(mk(x, y, seg=g // 2, strand=g % 2, flags=rng.integers(0, 1 << 23, n)))
    return Case("group_boundaries", np.concatenate(parts), merge=3)


def key_cases():
    """the key (y_i - 1, index 0): anchor 1 lies one base down the diagonal of anchor 0.  With anchor 0 the READ's first anchor it is a candidate (p = 0); as the first anchor
    of a later run of the read (beg != base) it is not (p = -1).  The launch holds other reads in front, so `base` is 0 for none but the first read."""
    tail_x, tail_y = 300 + 7 * np.arange(20), 900 + 7 * np.arange(20)
    first = mk(np.concatenate([[100, 101], tail_x]), np.concatenate([[500, 501], tail_y]))
    k1 = Case("key_read_first_run", first, probe={"p": {1: 0}})
    k2 = Case("key_read_base_not_0", first.copy(), probe={"p": {1: 0}})
    lead = mk(40 + 5 * np.arange(15), 70 + 5 * np.arange(15), seg=0)
    later = mk(np.concatenate([[100, 101], tail_x]), np.concatenate([[500, 501], tail_y]), seg=1)
    k3 = Case("key_later_run", np.concatenate([lead, later]), probe={"p": {16: -1}})
    return k1, k2, k3


def _neighbour(rng, seg):
    x, y = _diag(rng, 60, 90, 80, step=(1, 9))
    return mk(x, y, seg=seg)


def tie_cases():
    """A and B are isolated (neither sees the other: B lies below A), so f = q_span for both, and x + y is equal: equal priorities.  Z sees both.  Every read has an ordinary
    run before and behind the run in question."""
    rng = np.random.default_rng(24)
    A, B, Z = (1000, 2000), (1010, 1990), (1500, 2500)

    def read(name, pts, status, probe):
        mid = mk([q[0] for q in pts], [q[1] for q in pts], seg=1)
        return Case(name, np.concatenate([_neighbour(rng, 0), xsort(mid), _neighbour(rng, 2)]), expect={1: status} if status else {}, probe=probe)
    fill2 = [(1000 + k, 5000 - 2 * k) for k in range(1, 64)]
    fill3 = [(1000 + k, 7000 - 2 * k) for k in range(65, 128)]
    fill = [(1000 + k, 5000 - k) for k in range(1, 64)]   # 63 anchors between A and B that never enter Z's query (y above it) and chain with nothing but A
    return [read("tie_lanes", [A, B, Z], 1, {"tie_run": 1}),
            read("tie_not_at_minimum", [A, B, (1200, 1900), Z], 0, {"no_tie_run": 1}),               # C = (1200, 1900): x + y larger, sees neither A nor B, strictly better
            read("tie_partner_outside_y", [A, B, (1500, 2001)], 0, {"no_tie_run": 1}),                # y_A = y_Z - 1 is outside the query unless A is index 0 of the read
            read("tie_same_lane", [A] + fill + [(1064, 1936), Z], 1, {"tie_run": 1}),                 # indices 64 apart: one lane meets both
            # one lane meets A and B, tied, and then the strictly better C (index 128: the lane's tie mark must be dropped); or C is another lane's (index 65: the tie is in
            # a lane that does not hold the minimum).  The anchors between have x + y of their own, lie above Z's query, and those behind B see neither A nor B.
            read("tie_same_lane_then_better", [A] + fill2 + [(1064, 1936)] + fill3 + [(1128, 1900), Z], 0, {"no_tie_run": 1}),
            read("tie_same_lane_other_lane_better", [A] + fill2 + [(1064, 1936), (1065, 1937), Z], 0, {"no_tie_run": 1})]


def cand_case(n_cand, variant, seed):
    """exactly n_cand anchors in the inner window of the run's last anchor Z, which lies far to the right (dr > dq against every candidate: its range-minimum answer is never
    exact and the walk always happens).  Candidates sit on a few diagonals, so that marks land on candidates visited later; variant "eqy": a few query positions shared by many."""
    par = cand_par(0)
    rng = np.random.default_rng(seed)
    xz, yz = 9000, 6000
    pts = []
    n_chain = max(n_cand - 2, 0) if n_cand >= 2 else n_cand
    K = int(rng.integers(3, 8))
    for i in range(n_chain):
        c = i % K
        x = 5001 + i
        pts.append((x, (3300 + 13 * (i % 9)) if variant == "eqy" else (x - 1400 + 60 * c)))
    if n_cand >= 2:   # the ends of the query-position range
        pts.append((5000, yz - 1))
        pts.append((5000, yz - par.max_dist_inner))
    # not candidates: left of the inner window, at its edge, below and above the query-position range
    pts += [(int(x), int(y)) for x, y in zip(rng.integers(100, 1000, 25), rng.integers(2500, 5500, 25))]
    # (anchors behind the candidates lie so far up in y that the candidates are in no inner window but Z's)
    pts += [(xz - par.max_dist_inner - 1, 4000), (5700, yz - par.max_dist_inner - 1)]
    pts += [(int(x), int(y)) for x, y in zip(rng.integers(5800, 8000, 12), rng.integers(10100, 11000, 12))]
    pts += [(xz, 3000), (xz, yz)]   # (Z's own x: not available to Z)
    a = xsort(mk([q[0] for q in pts], [q[1] for q in pts]))
    assert int(a["x"][-1]) == xz and int(a["y"][-1] & np.uint64(0xffffffff)) == yz
    return Case("cand_%d_%s" % (n_cand, variant), a, expect={0: 2} if n_cand > RQ_CAND_MAX else {}, probe={"count": (len(a) - 1, n_cand)})


SKIP_CUTS = (40, 63, 64, 100, 128)   # where the walk of the skip sets' last anchor is cut: first block, its last lane, the first lane of the second block, later blocks


def skip_cut_case(max_skip, cut):
    """the walk of the last anchor Z = (9000, 6000) is cut at candidate `cut` exactly, and its RESULT says so.  In visiting order (descending y):
      H, alone, with a long span: the best priority, so the range-minimum answer, but beyond the band from Z: max_f stays q_span and the walk happens;
      n isolated anchors (no predecessor: they mark nothing, are marked by nothing, improve nothing);
      a chain of max_skip + 2 far off Z's diagonal, top down: the top unmarked, each further member marked by the one before and improving nothing, so the skip counter
        passes max_skip at its LAST member: the cut, at n + max_skip + 2;
      a chain of 8 on Z's exact diagonal, unmarked, better than q_span: the host never reaches it (f = q_span, p = -1).  A walk that is cut late or not at all, or that
        lost the counter on the way (cuts 64 and 128: the marked members straddle a block boundary), takes its top."""
    n = cut - max_skip - 2
    assert n >= 0
    pts = [(7000 + k, 5990 - 2 * k) for k in range(n)]
    pts += [(7200 + 2 * k, 5600 + 2 * k) for k in range(max_skip + 2)]
    pts += [(8000 + 10 * k, 5000 + 10 * k) for k in range(8)]
    a = xsort(np.concatenate([mk([q[0] for q in pts], [q[1] for q in pts]), mk([6900], [5998], span=255), mk([9000], [6000])]))
    return Case("skip_cut_at_%d" % cut, a, probe={"cut": cut, "carry": max_skip > 0 and cut in (64, 128)})


def late_winner_case(n):
    """the walk of the last anchor Z finds its winner at candidate n + 1, in the second block (n = 70) or the third (n = 130): H, alone and with a long span, has the best
    priority and is the range-minimum answer, but lies far off Z's diagonal and scores below q_span; n isolated anchors improve nothing; then the top of a chain of 20 on
    Z's diagonal -- unmarked, strictly better than everything before it"""
    pts = [(7100 + k, 5990 - 2 * k) for k in range(n)]
    pts += [(8000 + 10 * k, 4995 + 10 * k) for k in range(20)]
    a = xsort(np.concatenate([mk([q[0] for q in pts], [q[1] for q in pts]), mk([8500], [5995], span=255), mk([9000], [6000])]))
    return Case("late_winner_at_%d" % (n + 1), a, probe={"improve": n + 1})


def cand_groups():
    out = []
    for ms in CAND_SKIPS:
        cases = [cand_case(n, "diag", 300 + n) for n in CAND_COUNTS] + [cand_case(n, "eqy", 900 + n) for n in (65, 129, 512)]
        cases += [skip_cut_case(ms, c) for c in SKIP_CUTS if c - ms - 1 >= 0] + [late_winner_case(70), late_winner_case(130)]
        out.append(Group("candidates/max_skip=%d" % ms, cand_par(ms), cases))
    return out


def shape_group():
    rng = np.random.default_rng(25)
    k1, k2, k3 = key_cases()
    return Group("shapes", WIN, [k1, window_case(), equal_x_cases(), k2, group_boundary_case(), k3] + tie_cases() + [Case("plain", _neighbour(rng, 3))])


CAP_EVICT = Par(4000, 200, 2000, 25, 100, 0.8, 0.05)


def cap_evict_group():
    """a cap that bites the outer window alone and changes the result: a chain of 10, then 150 isolated anchors 10 bases apart and far above it in y, then Z on the chain's
    diagonal.  Without the cap Z joins the chain's top; with it the chain has left the window (100 anchors) and Z stays alone.  The inner window (200 bases: 20 anchors) is whole."""
    pts = [(1000 + 10 * k, 5000 + 10 * k) for k in range(10)] + [(1200 + 10 * k, 9000 - 3 * k) for k in range(150)] + [(2750, 6750)]
    c = Case("cap_evicts_the_answer", mk([q[0] for q in pts], [q[1] for q in pts]), probe={"cap_changes": len(pts) - 1})
    rng = np.random.default_rng(26)
    return Group("cap_outer_only_evicts", CAP_EVICT, [Case("plain", _neighbour(rng, 0)), c])


def all_groups():
    return [shape_group()] + cand_groups() + [cap_evict_group()] + random_groups()


def launch(group):
    """the chunk-level layout rq_dev_worker builds: the reads' arrays back to back, (beg, end, base) per run -> (a, runs, [(case, first run, abs0)])"""
    arrs, runs, where, abs0 = [], [], [], 0
    for c in group.cases:
        where.append((c, len(runs), abs0))
        runs += [(abs0 + b, abs0 + e, abs0) for b, e in c.cuts]
        arrs.append(c.a)
        abs0 += len(c.a)
    return (np.concatenate(arrs) if arrs else np.zeros(0, M128)), np.array(runs, dtype=np.int64).reshape(-1, 3), where


# ---------------------------------------------------------------- sets for the long-join rescue inside k_lchain

FIRST = dict(max_dist_x=5000, max_dist_y=5000, bw=500, max_skip=25, max_iter=5000, min_cnt=2, min_sc=20, pen_gap=0.12, pen_skip=0.01)
RESCUE = dict(max_dist=5000, max_dist_inner=1000, bw=20000, max_skip=25, cap=100000, min_cnt=2, min_sc=20, pen_gap=0.12, pen_skip=0.01, rescue_size=1000, rescue_ratio=0.1)
RESCUE_NV = (5, 63, 64, 65, 335, 336, 337, 1000, 3000)


def rescue_par(rs):
    return Par(rs["max_dist"], rs["max_dist_inner"], rs["bw"], rs["max_skip"], rs["cap"], rs["pen_gap"], rs["pen_skip"])


class RescueCase:
    """one read for mga.lchain_batch(..., rescue=, qlens=): flag = what the kernel must report; qlen may be set from the first pass's chains (fix_qlen)"""
    def __init__(self, name, a, flag, n_v=None, rescue=None, qlen=None, fix_qlen=None, probe=None):
        self.name, self.a, self.flag, self.n_v = name, np.ascontiguousarray(a, dtype=M128), flag, n_v
        self.rescue = dict(RESCUE, **(rescue or {}))
        self.qlen = int(qlen if qlen is not None else int((self.a["y"] & np.uint64(0xffffffff)).max()) + 500)
        self.fix_qlen, self.probe = fix_qlen, probe or {}


def pieces(rng, sizes, step=(20, 61), jump=(2500, 1000), x0=300, y0=200):
    """colinear pieces, each one chain of the first pass (every anchor chained), whose joins are wider than bw and narrower than bw_long"""
    xs, ys = [], []
    for n in sizes:
        d = rng.integers(step[0], step[1], n) if step[1] > step[0] else np.full(n, step[0])
        d[0] = 0
        xs.append(x0 + np.cumsum(d))
        ys.append(y0 + np.cumsum(d))
        x0, y0 = int(xs[-1][-1]) + jump[0], int(ys[-1][-1]) + jump[1]
    return mk(np.concatenate(xs), np.concatenate(ys))


def rescue_nv_case(n_v):
    rng = np.random.default_rng(4000 + n_v)
    sizes = (3, 2) if n_v == 5 else (n_v // 2, n_v - n_v // 2) if n_v < 300 else (n_v // 3, n_v // 3, n_v - 2 * (n_v // 3))
    return RescueCase("n_v=%d" % n_v, pieces(rng, sizes, step=(15, 16) if n_v == 5 else (20, 61)), 1, n_v=n_v)


def rescue_tie_case(n_long):
    """two chains of two anchors whose first anchors A and B are isolated with equal x + y; A2 sees both: the rescue hands the read back.  A long piece far behind them is the
    best chain and sets the form (n_v = n_long + 4)."""
    rng = np.random.default_rng(4100 + n_long)
    head = mk([1000, 1010, 1017, 1027], [2000, 1990, 2017, 2007])
    long_ = pieces(rng, (n_long,), x0=9000, y0=9000)
    return RescueCase("tie/n_v=%d" % (n_long + 4), np.concatenate([head, long_]), 2, n_v=n_long + 4, probe={"tie": True})


def rescue_cand_case(n_cand, n_second):
    """35 anchors 45 bases apart, then n_cand anchors 15 apart (exact predecessors: no walk), then Z one base off the diagonal, 20 behind the last: its walk meets exactly the
    n_cand anchors of the dense stretch (the one before it lies 1000 + bases back), and no other anchor has more than 64 in its window.  The second piece sets the form."""
    d = np.concatenate([[0], np.full(34, 45), [45], np.full(n_cand - 1, 15)])
    x1, y1 = 300 + np.cumsum(d), 200 + np.cumsum(d)
    xz, yz = int(x1[-1]) + 20, int(y1[-1]) + 21
    x2 = xz + 2500 + 16 * np.arange(n_second)
    y2 = yz + 1000 + 16 * np.arange(n_second)
    a = mk(np.concatenate([x1, [xz], x2]), np.concatenate([y1, [yz], y2]))
    return RescueCase("cand_%d/n_v=%d" % (n_cand, len(a)), a, 2 if n_cand > LC_CAND_MAX else 1, n_v=len(a), probe={"count": ((xz, yz), n_cand)})


def rescue_cap_case(n_v, over):
    rng = np.random.default_rng(4200 + n_v)
    return RescueCase("cap=%s/n_v=%d" % ("n_v-1" if over else "n_v", n_v), pieces(rng, (n_v // 2, n_v - n_v // 2)), 2 if over else 1, n_v=n_v, rescue=dict(cap=n_v - 1 if over else n_v))


def rescue_condition_cases():
    """the uncovered length qlen - (end - start of the best chain) exactly at rescue_size / qlen * rescue_ratio and one beyond; qlen is set from the first pass's best chain"""
    rng = np.random.default_rng(4300)
    a = pieces(rng, (200, 150), step=(30, 31))
    out = []
    for name, rs, fix, flag in (("size_at", dict(rescue_size=1000, rescue_ratio=1.0), lambda s: s + 1000, 0), ("size_over", dict(rescue_size=1000, rescue_ratio=1.0), lambda s: s + 1001, 1),
                                ("ratio_at", dict(rescue_size=1 << 30, rescue_ratio=0.5), lambda s: 2 * s, 0), ("ratio_over", dict(rescue_size=1 << 30, rescue_ratio=0.5), lambda s: 2 * s + 1, 1)):
        out.append(RescueCase("condition/" + name, a.copy(), flag, rescue=rs, fix_qlen=fix))
    out.append(RescueCase("condition/one_chain", pieces(rng, (120,)), 0, qlen=1 << 20))
    return out


def rescue_cases(ora):
    """every read of the rescue tests; ora: the oracle (its first pass fixes the query lengths of the condition cases)"""
    cs = [rescue_nv_case(n) for n in RESCUE_NV] + rescue_condition_cases()
    for n2 in (50, 400):   # the LDS form and the one over global memory
        cs += [rescue_tie_case(n2), rescue_cand_case(65, n2), rescue_cand_case(64, n2)]
    for n_v in (120, 500):
        cs += [rescue_cap_case(n_v, True), rescue_cap_case(n_v, False)]
    for c in cs:
        if c.fix_qlen:
            u, b = ora.lchain_dp(c.a, **first_kw(c))
            c.qlen = int(c.fix_qlen(int(b["y"][int(u[0] & np.uint64(0xffffffff)) - 1] & np.uint64(0xffffffff)) - int(b["y"][0] & np.uint64(0xffffffff))))
    return cs


def first_kw(c):
    return FIRST


def rescue_recipe(ora, c):
    """the host recipe of batch.c (chain_worker: do_rescue) from parts with tests of their own: the oracle's first pass, the condition, mga_ksort_128x over the chained anchors, the host tree with bw_long
    -> (u, b, due, first-pass u, first-pass b, sorted chained anchors)"""
    u1, b1 = ora.lchain_dp(c.a, **first_kw(c))
    rs = c.rescue
    due = False
    if len(u1) > 1:
        st, en = int(b1["y"][0] & np.uint64(0xffffffff)), int(b1["y"][int(u1[0] & np.uint64(0xffffffff)) - 1] & np.uint64(0xffffffff))
        unc = c.qlen - (en - st)
        due = bool(unc > rs["rescue_size"] or np.float32(unc) > np.float32(c.qlen) * np.float32(rs["rescue_ratio"]))
    if not due:
        return u1, b1, False, u1, b1, None
    s = ksort(b1)
    u2, b2 = host_chain(s, rescue_par(rs), rs["min_cnt"], rs["min_sc"])
    return u2, b2, True, u1, b1, s
