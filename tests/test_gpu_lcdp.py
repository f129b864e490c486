"""The first-pass DP of ultra-long -x lr reads on the device (k_lcrun.hip), both forms, bit for bit against the host's loop over the whole read (hchain.c:
mga_lchain_dp_fwd), and the path end to end under both settings of MGA_DEV_LCDP.  The seeded anchor helper is shared with test_lcdp_runs_host.py."""
import ctypes as C
import faulthandler
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import minigraph_amd as mga

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAR = dict(max_dist_y=500, bw=100, max_skip=25, max_iter=200, pen_gap=0.12, pen_skip=0.0)
DIST_X = 500


@pytest.fixture(autouse=True)
def time_limit():
    """every test here under its own limit: a persistent kernel that never ends would otherwise hold the whole run (the dump names the test; the process exits)"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def anchors(seed, n, hi=0, t0=1000, decoys=3, step=(3, 40), down=False):
    """n x-sorted anchors on one (segment, strand) word `hi`: a colinear chain with small indels plus `decoys` anchors per chain anchor close to it (shared predecessors:
    skip hits, equal scores); down: query positions fall instead, so that nothing chains and f is the span (13 .. 15) -- many equal best anchors in reach"""
    rng = np.random.default_rng(seed)
    m = max(1, n // (1 + decoys))
    st = rng.integers(step[0], step[1], m)
    t, q = t0 + np.cumsum(st), 100 + np.cumsum(st + rng.integers(-1, 2, m) * (rng.random(m) < 0.2))
    src = rng.integers(0, m, n - m)
    tt, qq = np.concatenate([t, t[src] + rng.integers(0, 3, n - m)]), np.concatenate([q, q[src] + rng.integers(-60, 60, n - m)])
    a = np.zeros(n, mga.m128)
    a["x"] = (np.uint64(hi) << np.uint64(32)) | tt.astype(np.uint64)
    a["y"] = np.maximum(qq, 1).astype(np.uint64) | np.uint64(15) << np.uint64(32)
    a = a[np.lexsort((a["y"], a["x"]))]
    if down:
        a["y"] = (10 ** 6 - 2 * np.arange(n)).astype(np.uint64) | rng.integers(13, 16, n).astype(np.uint64) << np.uint64(32)
    return a


def host_fwd(a, dist_x=DIST_X, rng=None, out=None, **par):
    """mga_lchain_dp_fwd over the whole array, or the work item rng = (beg, end) of it into out = (f, p, v) -> (f, p, v)"""
    P, n = dict(PAR, **par), len(a)
    f, p, v = out or (np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int32))
    arg = [dist_x, P["max_dist_y"], P["bw"], P["max_skip"], P["max_iter"], C.c_float(P["pen_gap"]), C.c_float(P["pen_skip"])]
    t = np.zeros(n, np.int32)
    ptr = [C.c_void_p(x.ctypes.data) for x in (a, f, p, v, t)]
    if rng is None:
        mga.load().mga_lchain_dp_fwd(*arg, C.c_int64(n), *ptr)
    else:
        mga.load().mga_lchain_dp_fwd_range(*arg, C.c_int64(rng[0]), C.c_int64(rng[1]), *ptr)
    return f, p, v


def cut(a, dist_x, run_min):
    cuts, n_cut = C.POINTER(C.c_int64)(), C.c_int32(0)
    mga.load().mga_lcdp_cut(C.c_int64(len(a)), C.c_void_p(a.ctypes.data), dist_x, C.c_int64(run_min), C.byref(cuts), C.byref(n_cut))
    return [cuts[k] for k in range(n_cut.value + 1)]   # (a few words, left to the process)


def case(name):
    """-> (reads [(anchors, dist_x, cuts)], parameters, wg_min of the workgroup form)"""
    NW, RING = mga.lcdp_shape()
    sizes = [1, 2, 63, 64, 65, 64 * NW - 1, 64 * NW, 64 * NW + 1]
    one = lambda a: (a, DIST_X, [0, len(a)])
    dense = lambda seed, n: anchors(seed, n, decoys=30, step=(1, 4))   # more than 64 * NW anchors in reach: several trips, cuts at every lane and wave, equal scores
    if name == "sizes":
        return [one(anchors(20 + n, n)) for n in sizes], dict(max_skip=25), 1
    if name == "sizes_skip2":
        return [one(dense(40 + n, n)) for n in sizes], dict(max_iter=100, max_skip=2), 1
    if name == "ring_wrap":       # more anchors than the ring holds, the window below it
        return [one(anchors(3, RING + 700)), one(dense(4, RING + 100))], dict(max_skip=2), 1
    if name == "ring_over":       # max_iter one above the ring: the workgroup form hands the middle item back, its neighbours (wave form) are done
        return [one(anchors(5, 300)), one(anchors(6, 400)), one(anchors(7, 300))], dict(max_iter=RING + 1), 301
    if name in ("dense_skip2", "dense_skip25"):   # windows of 600 > 64 * NW anchors: two trips, every wave of a trip, cuts before the best anchor in reach
        return [one(dense(8, 1500)), one(dense(9, 700))], dict(max_iter=600, max_skip=int(name[10:])), 1
    if name == "recompute":       # a high-scoring chain, then 1500 anchors that chain to nothing: the best anchor in reach falls out of reach again and again, over equal f
        A = anchors(80, 300)
        return [one(np.concatenate([A, anchors(81, 1500, t0=int(A["x"][-1]) + 5, decoys=0, step=(1, 4), down=True)]))], {}, 1
    reads = []                    # merged_F: items of several merged runs, two items per read (p counts from the read), another dist_x in the second read (-F)
    for seed, dist_x in ((60, DIST_X), (70, 300)):
        parts, t = [], 1000
        for k, n in enumerate([5, 400, 1, 1, 700, 30, 1100, 2, 90]):   # the pieces out of each other's reach, on alternating strands
            parts.append(anchors(seed + k, n, hi=7 | (k & 1) << 31, t0=t))
            t = (int(parts[-1]["x"][-1]) & 0xffffffff) + DIST_X + 1
        a = np.concatenate(parts)
        reads.append((a, dist_x, cut(a, dist_x, 1024)))
    assert all(len(c) >= 3 for _, _, c in reads)
    return reads, {}, 1


@pytest.mark.parametrize("name", ["sizes", "sizes_skip2", "ring_wrap", "ring_over", "dense_skip2", "dense_skip25", "recompute", "merged_F"])
@pytest.mark.parametrize("form", ["wave", "wg"])
def test_lcdp_fwd_equals_host_loop(form, name):
    reads, par, wg_min = case(name)
    wg_min = wg_min if form == "wg" else 1 << 40
    P = dict(PAR, **par)
    items, off = [], 0
    for a, dist_x, cuts in reads:
        items += [(off + b, off + e, off, dist_x) for b, e in zip(cuts[:-1], cuts[1:])]
        off += len(a)
    f, p, v, status = mga.lcdp_fwd_batch(np.concatenate([a for a, _, _ in reads]), items, wg_min=wg_min, **P)
    q = 0
    for a, dist_x, cuts in reads:
        base, (hf, hp, hv) = items[q][2], host_fwd(a, dist_x, **par)
        for b, e in zip(cuts[:-1], cuts[1:]):
            s = slice(base + b, base + e)
            if e - b >= wg_min and P["max_iter"] > mga.lcdp_shape()[1]:   # handed back, nothing of it written
                assert status[q] == 3 and not f[s].any() and not p[s].any() and not v[s].any(), (name, q)
            else:
                assert status[q] == 0, (name, q, status[q])
                assert np.array_equal(f[s], hf[b:e]) and np.array_equal(v[s], hv[b:e]), (name, q)
                assert np.array_equal(p[s], hp[b:e]), (name, q, "p")   # relative to the read's first anchor
            q += 1


CHILD = """import ctypes, json, sys
sys.path.insert(0, %r)
import minigraph_amd as mga
mga.map_files(sys.argv[1], [sys.argv[2]], sys.argv[3], preset="lr", cigar=True, n_threads=4, verbose=0)
st = (ctypes.c_int64 * 8)()
mga.load().mga_rq_dev_stats(st, 0)
print("STATS", json.dumps(list(st)))"""


def test_ultra_long_reads_same_bytes_with_the_dp_on_the_device():
    """reads beyond MGA_LONG_READ on a small bubble graph through the file path: the same GAF with the first chaining pass on the device and on a host thread (and as the
    reference, where it is built); the work items are counted where they went.  A fresh process per setting."""
    d = tempfile.mkdtemp()
    subprocess.check_call([mga.MGSIM, "-p", d + "/t", "-G", "3000000", "-H", "3", "-n", "3", "-l", "300000", "-e", "0.05", "-s", "92"], stderr=subprocess.DEVNULL)
    out, stats = {}, {}
    for knob in ("1", "0", "barriers"):   # (barriers: the A/B form of the phases, MGA_RQ_BARRIERS=1, is the host's whatever MGA_DEV_LCDP says)
        env = dict(os.environ, MGA_DEV_LCDP="1", MGA_RQ_BARRIERS="1") if knob == "barriers" else dict(os.environ, MGA_DEV_LCDP=knob)
        r = subprocess.run([sys.executable, "-c", CHILD % ROOT, d + "/t.gfa", d + "/t.reads.fa", d + "/out.gaf"], env=env, capture_output=True, timeout=110)
        assert r.returncode == 0, r.stderr[-2000:]
        stats[knob] = json.loads(r.stdout.decode().split("STATS")[1])
        out[knob] = open(d + "/out.gaf", "rb").read()
    assert len(out["0"]) > 0 and out["1"] == out["0"] and out["barriers"] == out["0"]
    assert stats["1"][5] > 0 and stats["1"][7] == 0 and stats["0"][5] == 0 and stats["barriers"][5] == 0, stats
    ref = os.path.join(ROOT, "oracle", "_ref", "minigraph")
    if os.path.exists(ref):
        assert out["1"] == subprocess.run([ref, "-c", "-x", "lr", "-t", "4", d + "/t.gfa", d + "/t.reads.fa"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout
