"""GPU: the bridge between two linear chains on a workgroup (k_gwfa_wg.hip) against the host's mga_gwfa_bridge(), which tests/test_host_gwfa.py holds to the
reference's gfa_ed_step: same edit distance, same vertex walk, problem by problem; and the mapping path with the form switched on, byte for byte."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import minigraph_amd as mga
from test_host_gwfa import load_gfa, mutate, sample_walk, vseq

pytestmark = pytest.mark.gpu

NW, CAP = 8, 1024   # wavefronts of the workgroup form, cells of its wavefront buffers (asserted against the library below)
BIG = 10000


def walks(segs, arcs, seed, rate, length, want, n_vert=1, rev=False):
    """`want` bridges (query, v0, off0, v1, off1) over sampled walks of at least n_vert vertices (rev: some of them reverse-strand), mutated at `rate`"""
    rng, out = np.random.default_rng(seed), []
    while len(out) < want:
        v0, off0, v1, off1, seq, path = sample_walk(rng, segs, arcs, length)
        if len(seq) >= 4 and len(path) >= n_vert and (not rev or any(v & 1 for v in path)):
            out.append((mutate(rng, seq, rate), v0, off0, v1, off1))
    return out


def build_cases(segs, arcs):
    """group -> problems (query, v0, off0, v1, off1, max_lag, s_term).  A wavefront is about twice the edit distance wide (two cells join per step until the 1 000-cell
    pruning), so the mutation rate times the length places a case below 64 cells, between 64 and 64 * NW, between 64 * NW and CAP, or beyond CAP."""
    v = max(range(len(segs)), key=lambda s: len(segs[s])) << 1
    s = vseq(segs, v)
    rng = np.random.default_rng(5)
    inside = [(s[100:100 + n], v, 100, v, 100 + n - 1, 5000, BIG) for n in (0, 1, 63, 64, 65)]
    inside += [(mutate(rng, s[100:100 + n], 0.1), v | 1, 100, v | 1, 100 + n - 1, 5000, BIG) for n in (63, 64, 65)]
    full = lambda ws, s_term=BIG: [w + (5000, s_term) for w in ws]
    return {
        "inside": inside,                                                       # (a) one vertex, query gaps of 0, 1, 63, 64, 65 bases
        # (b) walks over five vertices -- stem, allele, stem, allele, stem: two bubbles; 18 kb in this graph of long stems -- at mutation rates that put the largest
        # wavefront, as the host routine runs it, beyond one wave's share (64 cells) and beyond one trip of the workgroup (64 * NW cells)
        "wave_share": full(walks(segs, arcs, 11, 0.002, 18000, 3, n_vert=5)),
        "one_trip": full(walks(segs, arcs, 12, 0.0035, 18000, 3, n_vert=5)),
        "reverse": full(walks(segs, arcs, 13, 0.08, 1500, 4, n_vert=2, rev=True)),   # (c) reverse-strand vertices
        "fails": [w[:3] + (w[3] ^ 1, w[4], 5000, 400) for w in walks(segs, arcs, 14, 0.1, 600, 2, n_vert=2)] +  # (d) the wrong end vertex ...
                 full(walks(segs, arcs, 15, 0.2, 800, 2), s_term=25) +                                          #     ... s_term too small ...
                 [w + (3, BIG) for w in walks(segs, arcs, 16, 0.2, 2000, 1)],                                   #     ... and a max_lag that prunes hard (found or not: equal on both sides)
        "too_wide": full(walks(segs, arcs, 17, 0.3, 2400, 2)) + full(walks(segs, arcs, 18, 0.018, 18000, 1, n_vert=5)),   # (e) past the LDS capacity: handed back
    }


PEAK = {"inside": (1, 128), "wave_share": (65, 64 * NW), "one_trip": (64 * NW + 1, CAP), "reverse": (65, CAP)}   # cells the largest wavefront must hold, per served group


@pytest.fixture(scope="module")
def bridges(tmp_path_factory):
    """the problems, the host's answers, and the device's answers in both forms (one launch each)"""
    L = mga.load()
    d = str(tmp_path_factory.mktemp("gwfa_wg"))
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
        host.append((ed, [p[i] for i in range(nv.value)] if ed >= 0 else []))
        if p:
            libc.free(p)
    dev = {form: mga.gwfa_bridge_batch(G, flat, form=form) for form in ("workgroup", "wave")}
    G.close()
    index, k = {}, 0
    for name, grp in cases.items():
        index[name] = range(k, k + len(grp))
        k += len(grp)
    return index, host, dev


def test_shape():
    assert mga.gwfa_wg_shape() == (NW, CAP)


@pytest.mark.parametrize("group", ["inside", "wave_share", "one_trip", "reverse", "fails", "too_wide"])
def test_workgroup_form_matches_host(bridges, group):
    index, host, dev = bridges
    for i in index[group]:
        ed, path, status, peak = dev["workgroup"][i]
        print(group, i, "host ed", host[i][0], "device ed", ed, "vertices", len(path), mga.GWFA_STATUS[status], "peak", peak)
        assert (ed, path) == host[i], (group, i)
        assert mga.GWFA_STATUS[status] == ("handed back" if group == "too_wide" else "workgroup"), (group, i, peak)
    if group in PEAK:
        top = max(dev["workgroup"][i][3] for i in index[group])
        assert PEAK[group][0] <= top <= PEAK[group][1], (group, top)
    if group == "fails":
        assert [host[i][0] for i in index[group]][:4] == [-1] * 4
    if group in ("wave_share", "one_trip"):
        assert all(len(host[i][1]) >= 5 for i in index[group])
    if group == "reverse":
        assert any(v & 1 for i in index[group] for v in host[i][1])


def test_wave_form_matches_host(bridges):
    index, host, dev = bridges
    for i, (ed, path, status, _) in enumerate(dev["wave"]):
        assert (ed, path) == host[i] and mga.GWFA_STATUS[status] == "wave", i


CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import minigraph_amd as mga
G = mga.Graph(sys.argv[1], preset="lr", n_threads=4)
R = mga.Reads(sys.argv[2])
gaf = mga.map_reads(G, R, n_threads=4)
st = mga.gc_wg_stats()
print("RESULT", hashlib.md5(gaf).hexdigest(), len(gaf), st["served"], st["handed_back"])
"""


def test_mapping_path_is_byte_identical(tmp_path):
    """300 simulated 20 kb reads at 20 % error over a bubble graph of 8 haplotypes (long, diverged gaps between the chains: bridges of the top gap classes), a fresh process per setting: the GAF does not change, and the form runs only where it is asked for"""
    d = str(tmp_path)
    subprocess.check_call([mga.MGSIM, "-p", os.path.join(d, "t"), "-G", "400000", "-H", "8", "-n", "300", "-l", "20000", "-e", "0.2", "-s", "13"], stderr=subprocess.DEVNULL)
    got = {}
    for name, env in (("wg", {"MGA_GC_SPLIT": "1", "MGA_GC_BRIDGE_WG": "1"}), ("split", {"MGA_GC_SPLIT": "1", "MGA_GC_BRIDGE_WG": "0"}), ("default", {})):
        e = {k: v for k, v in os.environ.items() if k not in ("MGA_GC_SPLIT", "MGA_GC_BRIDGE_WG")}
        e.update(env, MGA_DEV_GCHAIN="1")   # every chunk's graph chaining on the device
        out = subprocess.run([sys.executable, "-c", CHILD % mga.ROOT, os.path.join(d, "t.gfa"), os.path.join(d, "t.reads.fa")], env=e, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        got[name] = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][0].split()[1:]
        print(name, got[name])
    assert got["wg"][:2] == got["split"][:2] == got["default"][:2] and int(got["default"][1]) > 0
    assert int(got["wg"][2]) > 0 and got["split"][2:] == ["0", "0"] and got["default"][2:] == ["0", "0"]
