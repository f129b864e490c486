"""GPU: the wide workgroup form of the bridge (k_gwfa_wgx.hip) against the host's mga_gwfa_bridge(), which tests/test_host_gwfa.py holds to the reference's
gfa_ed_step: same edit distance, same vertex walk, problem by problem, and never handed back for the width of a wavefront of cells."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import minigraph_amd as mga
from test_gpu_gwfa_wg import BIG, walks
from test_host_gwfa import load_gfa, mutate, vseq

pytestmark = pytest.mark.gpu

NW, WIDE = 8, 3072   # wavefronts of the wide form, cells of its wavefront buffers (asserted against the library below)


def build_cases(segs, arcs):
    """group -> problems (query, v0, off0, v1, off1, max_lag, s_term); a wavefront is about twice the edit distance wide"""
    v = max(range(len(segs)), key=lambda s: len(segs[s])) << 1
    s = vseq(segs, v)
    rng = np.random.default_rng(5)
    full = lambda ws, s_term=BIG, max_lag=5000: [w + (max_lag, s_term) for w in ws]
    two_bubbles = lambda seed, rate, want: walks(segs, arcs, seed, rate, 18000, want, n_vert=5)   # stem, allele, stem, allele, stem: 18 kb
    return {
        "inside": [(s[100:100 + n], v, 100, v, 100 + n - 1, 5000, BIG) for n in (0, 1, 63, 64, 65)] +
                  [(mutate(rng, s[100:100 + n], 0.1), v | 1, 100, v | 1, 100 + n - 1, 5000, BIG) for n in (63, 64, 65)],
        "narrow": full(two_bubbles(11, 0.002, 2)) + full(two_bubbles(12, 0.0035, 2)),       # what the 1 024-cell form serves: peaks of 65 .. 1 024 cells
        # what the 1 024-cell form hands back (its `too_wide` group: 339 edits over two bubbles, ~600 over one or two vertices), and twice the edits over two bubbles (689)
        "wide": full(two_bubbles(18, 0.018, 1)) + full(two_bubbles(19, 0.036, 1)) + full(walks(segs, arcs, 17, 0.3, 2400, 2)),
        # more than 1 000 cells at every 16th step for hundreds of steps, with a lag bound that lets the pruning drop cells
        "pruned": full(walks(segs, arcs, 17, 0.3, 2400, 2), max_lag=3) + full(two_bubbles(19, 0.036, 1), max_lag=40),
        "reverse": full(walks(segs, arcs, 13, 0.08, 1500, 4, n_vert=2, rev=True)),
        "fails": [w[:3] + (w[3] ^ 1, w[4], 5000, 400) for w in walks(segs, arcs, 14, 0.1, 600, 2, n_vert=2)] + full(walks(segs, arcs, 15, 0.2, 800, 2), s_term=25),
        # hundreds of cells reach the end of a bubble's stem nearly as one: each becomes a head cell that pushes flagged cells into both alleles, far more than the 64
        # up to which the sort is klib's insertion sort
        "dedup_many": full(two_bubbles(20, 0.01, 2)),
    }


@pytest.fixture(scope="module")
def bridges(tmp_path_factory):
    """the problems, the host's answers and the wide form's (one launch)"""
    L = mga.load()
    d = str(tmp_path_factory.mktemp("gwfa_wgx"))
    subprocess.check_call([mga.MGSIM, "-p", os.path.join(d, "t"), "-G", "400000", "-H", "4", "-n", "1", "-s", "13"], stderr=subprocess.DEVNULL)
    gfa = os.path.join(d, "t.gfa")
    cases = build_cases(*load_gfa(gfa))
    G = mga.Graph(gfa, preset="lr", n_threads=4)
    es = C.cast(G.gi, C.POINTER(C.c_void_p))[1]                   # mg_idx_t.es (minigraph.h:93-98)
    L.mga_gwfa_bridge.restype = C.c_int32
    L.mga_gwfa_bridge.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_char_p, C.c_uint32, C.c_int32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32,
                                  C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_int32)]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    flat, host = [p for grp in cases.values() for p in grp], []
    for q, v0, off0, v1, off1, max_lag, s_term in flat:
        p, nv = C.POINTER(C.c_int32)(), C.c_int32(0)
        ed = L.mga_gwfa_bridge(G.g, es, len(q), q, v0, off0, v1, off1, max_lag, s_term, C.byref(p), C.byref(nv))
        host.append((ed, [p[i] for i in range(nv.value)] if ed >= 0 else [], mga.gwfa_bridge_cells()))   # + (largest wavefront, cells pruned) of the host routine
        if p:
            libc.free(p)
    dev = mga.gwfa_bridge_batch(G, flat, form="wide")
    mga.gwfa_wgx_stats(reset=True)
    again = mga.gwfa_bridge_batch(G, cases["dedup_many"], form="wide")   # that group alone: what its dedups sorted
    sorted_ = mga.gwfa_wgx_stats()
    G.close()
    index, k = {}, 0
    for name, grp in cases.items():
        index[name] = range(k, k + len(grp))
        k += len(grp)
    assert again == [dev[i] for i in index["dedup_many"]]
    return index, host, dev, sorted_


def test_shape():
    assert mga.gwfa_wgx_shape() == (NW, WIDE, WIDE)


@pytest.mark.parametrize("group", ["inside", "narrow", "wide", "pruned", "reverse", "fails", "dedup_many"])
def test_wide_form_matches_host(bridges, group):
    index, host, dev, sorted_ = bridges
    for i in index[group]:
        ed, path, status, peak = dev[i]
        print(group, i, "host ed", host[i][0], "device ed", ed, "vertices", len(path), mga.GWFA_STATUS[status], "peak", peak, "host (peak, pruned)", host[i][2])
        assert (ed, path) == host[i][:2], (group, i)
        assert mga.GWFA_STATUS[status] == "wide workgroup", (group, i, peak)
    top = max(dev[i][3] for i in index[group])
    if group == "narrow":
        assert 64 < top <= 1024, top
    if group == "wide":
        assert top > 1024 and [host[i][0] for i in index[group]][:2] == [339, 689], top   # the wide buffers held a wavefront the 1 024-cell form cannot
    if group == "pruned":
        # on the host: the routine's wavefront passed the 1 000 cells above which the pruning is taken, and the pruning dropped cells
        assert all(host[i][2][0] > 1000 and host[i][2][1] > 0 for i in index[group]), [host[i][2] for i in index[group]]
    if group == "fails":
        assert [host[i][0] for i in index[group]] == [-1] * 4
    if group == "reverse":
        assert any(v & 1 for i in index[group] for v in host[i][1])
    if group == "dedup_many":
        print("dedup_many", sorted_)
        assert sorted_["max_flagged"] > 64 and all(len(host[i][1]) >= 5 for i in index[group])   # the 8-wave rank sort ran on more cells than klib's insertion sort takes
