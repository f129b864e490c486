"""Read coverage (--cov) without a GPU: the host instantiation of cov_core.h against mg_cov_map() of the reference library on the reference's own chains, hand-made
walks, and the tagging of a graph that already carries dc:f: / cv:f: tags.

The integer sums divided once must give the float the reference stores (gfa-base.c:475: a float): (float)cov_seg is compared bit for bit, link counts as integers.
The integer form differs from the reference's running double sum by about n * 2^-53 relative, so a mismatch would be a rounding tie of a fixture, not a tolerance.
Fixtures: tests/golden/MT.gfa with MT-orangA.fa and MT-chimp.fa; mgsim -G 200000 -H 3 -n 200 -l 5000 -s 5.  Every value of both agreed with the first seed tried."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import minigraph_amd as mga
import refbind as rb
import cov_cases as cc


def need_ref():
    """the reference library is the checker here: its absence is a failure, never a skip"""
    assert rb.have_ref(), "oracle/_ref/libmgref.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` where the reference sources exist"


def read_fasta(path):
    name, seq, out = None, [], []
    for line in open(path, "rb"):
        line = line.rstrip()
        if line.startswith(b">"):
            if name is not None:
                out.append((name, b"".join(seq).upper()))
            name, seq = line[1:].split()[0], []
        else:
            seq.append(line)
    if name is not None:
        out.append((name, b"".join(seq).upper()))
    return out


def ref_lib():
    need_ref()
    R = C.CDLL(rb.REF_SO)
    R.gfa_read.argtypes, R.gfa_read.restype = [C.c_char_p], C.c_void_p
    R.gfa_destroy.argtypes = [C.c_void_p]
    R.mg_opt_set.argtypes = [C.c_char_p, C.POINTER(mga.idxopt_t), C.POINTER(mga.mapopt_t), C.POINTER(mga.ggopt_t)]
    R.mg_index.argtypes, R.mg_index.restype = [C.c_void_p, C.POINTER(mga.idxopt_t), C.c_int, C.POINTER(mga.mapopt_t)], C.c_void_p
    R.mg_idx_destroy.argtypes = [C.c_void_p]
    R.mg_tbuf_init.restype = C.c_void_p
    R.mg_tbuf_destroy.argtypes = [C.c_void_p]
    R.mg_map.argtypes, R.mg_map.restype = [C.c_void_p, C.c_int, C.c_char_p, C.c_void_p, C.POINTER(mga.mapopt_t), C.c_char_p], C.c_void_p
    R.mg_gchain_free.argtypes = [C.c_void_p]
    R.mg_cov_map.argtypes, R.mg_cov_map.restype = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_char_p], None
    R.gfa_aux_update_cv.argtypes, R.gfa_aux_update_cv.restype = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p], None
    return R


def compare_on(graph, read_paths, min_mapq, min_blen, cigar):
    """the reference's chains of every read through both counters"""
    L, R = mga.load(), ref_lib()
    L.mga_cov_gchains.argtypes, L.mga_cov_gchains.restype = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(mga.cov_stats_t)], None
    io, mo, go = mga.idxopt_t(), mga.mapopt_t(), mga.ggopt_t()
    R.mg_opt_set(None, C.byref(io), C.byref(mo), C.byref(go))
    R.mg_opt_set(b"lr", C.byref(io), C.byref(mo), C.byref(go))
    if cigar:
        mo.flag |= mga.MG_M_CIGAR
    g = R.gfa_read(graph.encode())
    gi = R.mg_index(g, C.byref(io), 2, C.byref(mo))
    n_seg, n_arc = mga._cov_sizes(g)
    c_seg, c_link = np.zeros(n_seg, dtype=np.float64), np.zeros(n_arc, dtype=np.float64)
    sb, lc, st = np.zeros(n_seg, dtype=np.int64), np.zeros(n_arc, dtype=np.int64), mga.cov_stats_t()
    tb = R.mg_tbuf_init()
    for p in read_paths:
        for name, seq in read_fasta(p):
            gt = R.mg_map(gi, len(seq), seq, tb, C.byref(mo), name)
            R.mg_cov_map(g, gt, min_mapq, min_blen, c_seg.ctypes.data, c_link.ctypes.data, name)
            L.mga_cov_gchains(g, gt, min_mapq, min_blen, sb.ctypes.data, lc.ctypes.data, C.byref(st))
            R.mg_gchain_free(gt)
    R.mg_tbuf_destroy(tb)
    cs, cl = mga.cov_finish(g, sb, lc)
    R.mg_idx_destroy(gi)
    R.gfa_destroy(g)
    assert st.chains_counted > 0 and sb.sum() > 0
    assert np.array_equal(lc, c_link.astype(np.int64)) and np.array_equal(cl, c_link)
    assert np.array_equal(cs.astype(np.float32).view(np.uint32), c_seg.astype(np.float32).view(np.uint32)), np.nonzero(cs.astype(np.float32) != c_seg.astype(np.float32))[0][:10]
    return st


@pytest.mark.parametrize("min_mapq,min_blen,cigar", [(20, 1000, True), (0, 1000, True), (20, 50, False)])
def test_mt_vs_mg_cov_map(min_mapq, min_blen, cigar):
    graph, reads = cc.mt_fixture()
    compare_on(graph, reads, min_mapq, min_blen, cigar)


@pytest.mark.parametrize("min_mapq,min_blen,cigar", [(20, 1000, True), (0, 50, False)])
def test_bubble_vs_mg_cov_map(min_mapq, min_blen, cigar):
    d = tempfile.mkdtemp()
    graph, rd = cc.bubble_fixture(d)
    st = compare_on(graph, [rd], min_mapq, min_blen, cigar)
    assert st.links_counted > 0


@pytest.fixture(scope="module")
def chain_g():
    L = mga.load()
    path = os.path.join(tempfile.mkdtemp(), "chain.gfa")
    cc.write_chain_gfa(path)
    g = L.gfa_read(path.encode())
    assert g
    cc.tamper(g)
    yield g
    L.gfa_destroy(g)


def test_one_vertex_chain(chain_g):
    K = cc.Cases()
    K.add(cc.fwd(40, 1), ps=10, tail=20)
    sb, lc, st = mga.cov_chains_host(chain_g, *K.arrays(), 20, 1000)
    assert sb[40] == 60 - 10 - 20 and sb.sum() == 30 and lc.sum() == 0 and st == {"chains_counted": 1, "links_counted": 0, "links_skipped": 0}


def test_both_orientations_of_one_segment(chain_g):
    K = cc.Cases()
    K.add(cc.fwd(40, 3))   # s40+ s41+ s42+
    K.add(cc.rev(42, 3))   # s42- s41- s40-
    sb, lc, st = mga.cov_chains_host(chain_g, *K.arrays(), 20, 1000)
    assert list(sb[40:43]) == [57 + 55, 120, 55 + 57]
    for v, w in ((40, 41), (41, 42)):
        assert lc[cc.find_arc(chain_g, v << 1, w << 1)] == 2 and lc[cc.find_arc(chain_g, w << 1 | 1, v << 1 | 1)] == 2
    assert lc.sum() == 8 and st["links_counted"] == 4


def test_duplicate_and_missing_arcs_are_skipped(chain_g):
    K = cc.Cases()
    K.add(cc.fwd(cc.DUP_AT, 2))
    sb, lc, st = mga.cov_chains_host(chain_g, *K.arrays(), 20, 1000)
    assert lc.sum() == 0 and st["links_skipped"] == 1 and sb[0] == 57 and sb[1] == 55
    K = cc.Cases()
    K.add(cc.fwd(cc.MISS_AT, 2))
    sb, lc, st = mga.cov_chains_host(chain_g, *K.arrays(), 20, 1000)
    assert lc.sum() == 0 and st["links_skipped"] == 1 and st["chains_counted"] == 1


def test_filters(chain_g):
    K = cc.Cases()
    K.add(cc.fwd(40, 2), mapq=60)
    K.add(cc.fwd(40, 2), mapq=0)              # a secondary chain (gcmisc.c:221)
    K.add(cc.fwd(40, 2), mapq=60, blen=999)   # fails the blen bar only
    assert mga.cov_chains_host(chain_g, *K.arrays(), 20, 1000)[2]["chains_counted"] == 1
    assert mga.cov_chains_host(chain_g, *K.arrays(), 0, 1000)[2]["chains_counted"] == 2
    assert mga.cov_chains_host(chain_g, *K.arrays(), 0, 999)[2]["chains_counted"] == 3


def test_aux_update_on_a_graph_with_tags():
    """gfa_aux_update_cv (gfa-base.c:475-503) on lines that already carry dc:f: and cv:f: (and cv:i:) tags: this library's function and the reference's on two copies of
    one graph, both printed by the reference's gfa_print.  (The graph is read by the reference's reader: this library's keeps only the tags the mapping path reads.)"""
    L, R = mga.load(), ref_lib()
    d = tempfile.mkdtemp()
    path = os.path.join(d, "tags.gfa")
    with open(path, "wb") as f:
        f.write(b"S\ta\tACGTACGTAC\tSN:Z:c\tSO:i:0\tSR:i:0\tdc:f:1.5\n")
        f.write(b"S\tb\tACGTACG\tSN:Z:c\tSO:i:10\tSR:i:0\tcv:f:2.25\txx:Z:keep\n")
        f.write(b"S\tc\tACGTA\tSN:Z:c\tSO:i:17\tSR:i:0\n")
        f.write(b"S\td\tACG\tSN:Z:d\tSO:i:0\tSR:i:1\tyy:i:7\tcv:i:3\tdc:f:9\n")
        f.write(b"L\ta\t+\tb\t+\t0M\tSR:i:0\tdc:f:4\n")
        f.write(b"L\tb\t+\tc\t+\t0M\tSR:i:0\tcv:f:5\n")
        f.write(b"L\ta\t+\td\t+\t0M\tSR:i:1\n")
        f.write(b"L\td\t+\tc\t+\t0M\tSR:i:1\tzz:Z:t\n")
    L.mga_gfa_aux_update_cv.argtypes, L.mga_gfa_aux_update_cv.restype = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p], None
    g1, g2 = R.gfa_read(path.encode()), R.gfa_read(path.encode())
    n_seg, n_arc = mga._cov_sizes(g1)
    sb, lc = np.arange(3, 3 + 7 * n_seg, 7, dtype=np.int64), np.arange(1, 1 + n_arc, dtype=np.int64)
    cs, cl = mga.cov_finish(g1, sb, lc)
    R.gfa_aux_update_cv(g1, b"dc", cs.ctypes.data, cl.ctypes.data)
    L.mga_gfa_aux_update_cv(g2, b"dc", cs.ctypes.data, cl.ctypes.data)
    want, got = cc.ref_print(R, g1, os.path.join(d, "want.gfa")), cc.ref_print(R, g2, os.path.join(d, "got.gfa"))
    R.gfa_destroy(g1); R.gfa_destroy(g2)
    assert b"dc:f:" in want and b"cv:" in want
    assert got == want
