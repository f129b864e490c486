"""--call without a GPU: mga_call_asm_host (csrc/call.c + the host instantiation of call_core.h + csrc/bubble.c) on the REFERENCE's chains -- mg_map of libmgref.so under
-x asm, with and without -c, on a graph whose reference arcs the reference sorted (main.c:280) -- against the bytes of `oracle/_ref/minigraph [-c] -x asm --call` on the
same files.  Then the Python replay of call_cases.py is proved equal to the host instantiation on those real chains, and used to predict every crafted case that
test_gpu_call.py sends through the kernel."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

import minigraph_amd as mga
import refbind as rb
import call_cases as kc
from test_cov_host import read_fasta


def need_ref():
    assert rb.have_ref() and os.path.exists(rb.REF_BIN), "oracle/_ref is missing: run `python -c 'import __graft_entry__ as g; g.build()'` where the reference sources exist"


class RefChains:
    """the reference's graph, index and chains of every sequence of one query file, kept for the tests of one case"""

    def __init__(self, graph, query, cigar):
        need_ref()
        self.R = R = kc.ref_lib()
        self.io, self.mo, self.go = mga.idxopt_t(), mga.mapopt_t(), mga.ggopt_t()
        R.mg_opt_set(None, C.byref(self.io), C.byref(self.mo), C.byref(self.go))
        assert R.mg_opt_set(b"asm", C.byref(self.io), C.byref(self.mo), C.byref(self.go)) == 0
        if cigar:
            self.mo.flag |= mga.MG_M_CIGAR
        self.g = R.gfa_read(graph.encode())
        R.gfa_sort_ref_arc(self.g)
        self.gi = R.mg_index(self.g, C.byref(self.io), 4, C.byref(self.mo))
        tb = R.mg_tbuf_init()
        recs = read_fasta(query)
        self.names = [n for n, _ in recs]
        self.gcs = [R.mg_map(self.gi, len(s), s, tb, C.byref(self.mo), n) for n, s in recs]
        R.mg_tbuf_destroy(tb)


@functools.lru_cache(maxsize=None)
def mgsim_files():
    need_ref()
    d = tempfile.mkdtemp()
    graph, reads = kc.mgsim_asm(d)
    assert kc.bed_is_ground(kc.ref_call(graph, reads, os.path.join(d, "ground.bed"))), "the reference's BED of the mgsim case must carry >= 50 walks and a '.' line: pick another seed"
    return graph, reads


def case_files(case):
    if case == "mgsim":
        return mgsim_files()
    return os.path.join(kc.GOLD, "MT.gfa"), os.path.join(kc.GOLD, case)


def min_len_of(case, rc):
    """-l: the preset's 100 kb would index nothing of a 16.5 kb genome (and print nothing); the MT cases run with -l 5000 on both sides"""
    return rc.go.min_map_len if case == "mgsim" else 5000


def cli_of(case):
    return [] if case == "mgsim" else ["-l", "5000"]


@functools.lru_cache(maxsize=None)
def chains_of(case, cigar):
    return RefChains(*case_files(case), cigar)


@pytest.mark.parametrize("cigar", [True, False])
@pytest.mark.parametrize("case", ["MT-orangA.fa", "MT-chimp.fa", "mgsim"])
def test_bed_equals_reference_binary(case, cigar):
    rc = chains_of(case, cigar)
    graph, query = case_files(case)
    want = kc.ref_call(graph, query, os.path.join(tempfile.mkdtemp(), "want.bed"), cigar, cli_of(case))
    got = mga.call_asm_host(rc.g, rc.names, rc.gcs, rc.go.min_mapq, min_len_of(case, rc))
    assert want.count(b"\n") > 0
    assert got == want


def test_nothing_indexed_prints_nothing():
    """min_mapq / min_blen beyond every chain: mg_gc_index returns 0 and mg_call_asm prints nothing at all -- on both sides"""
    rc = chains_of("mgsim", True)
    graph, query = case_files("mgsim")
    d = tempfile.mkdtemp()
    assert kc.ref_call(graph, query, os.path.join(d, "a.bed"), True, ["-q", "250"]) == b""
    assert mga.call_asm_host(rc.g, rc.names, rc.gcs, 250, rc.go.min_map_len) == b""
    assert kc.ref_call(graph, query, os.path.join(d, "b.bed"), True, ["-l", "100000000"]) == b""
    assert mga.call_asm_host(rc.g, rc.names, rc.gcs, rc.go.min_mapq, 100000000) == b""


def called(bed):
    return sum(1 for l in bed.splitlines() if l.split(b"\t")[5] != b".")


def test_a_repeated_contig_triggers_the_graph_overlap_rejection():
    """the query file with its first contig twice: two query-disjoint chains over the same segments, so those segments carry two indexed intervals and the
    candidates over them are dropped -- the reference calls fewer bubbles than with one copy, and this library prints the same bytes"""
    graph, query = case_files("mgsim")
    d = tempfile.mkdtemp()
    recs = read_fasta(query)
    twice = os.path.join(d, "twice.fa")
    with open(twice, "wb") as f:
        for n, s in [recs[0], (recs[0][0] + b"_again", recs[0][1])] + recs[1:]:
            f.write(b">" + n + b"\n" + s + b"\n")
    once = kc.ref_call(graph, query, os.path.join(d, "once.bed"))
    want = kc.ref_call(graph, twice, os.path.join(d, "twice.bed"))
    assert called(want) < called(once), (called(want), called(once))
    rc = RefChains(graph, twice, True)
    assert mga.call_asm_host(rc.g, rc.names, rc.gcs, rc.go.min_mapq, rc.go.min_map_len) == want


# ---- the replay ----

def real_flat(case, cigar):
    rc = chains_of(case, cigar)
    bb, bv = mga.bubbles(rc.g)
    return rc, bb, bv, kc.flat_from_gchains(rc.gcs, kc.seg_lens(rc.g), bb, bv, rc.go.min_mapq, min_len_of(case, rc))


@pytest.mark.parametrize("case,cigar", [("MT-orangA.fa", True), ("MT-chimp.fa", False), ("mgsim", True)])
def test_replay_equals_host_instantiation_on_real_chains(case, cigar):
    """flat records made in Python from the reference's chains: the replay (a scalar loop, as the reference writes it) and mga_call_batch_host (running sums, as the
    kernel forms them) give the same winner per bubble, and that winner is the one the reference binary printed (strand, glen, qs, qe of column 6)"""
    rc, bb, bv, F = real_flat(case, cigar)
    assert F is not None
    win, warns = kc.replay(**F)
    hwin, hwarn = mga.call_chains_host(**F)
    assert kc.win_of(hwin) == win and kc.warn_of(hwarn) == warns
    graph, query = case_files(case)
    lines = kc.ref_call(graph, query, os.path.join(tempfile.mkdtemp(), "want.bed"), cigar, cli_of(case)).splitlines()
    assert len(lines) == len(bb)
    for i, l in enumerate(lines):
        col = l.split(b"\t")[5]
        if col == b".":
            assert i not in win, i
            continue
        walk, glen, strand, name, qs, qe = col.split(b":")
        w = win[i]
        assert (w[7], "+" if w[4] > 0 else "-", rc.names[w[8]], w[5], w[6]) == (int(glen), strand.decode(), name, int(qs), int(qe)), (i, w, col)
        assert (walk == b"*") == (w[2] == w[3])
    if case == "mgsim":
        assert len(win) >= 50


K, GROUPS = kc.crafted()


@pytest.mark.parametrize("name", sorted(GROUPS) + ["all", "all_reversed"])
def test_crafted_cases_host_instantiation_equals_replay(name):
    F = K.arrays(GROUPS.get(name))
    if name == "all_reversed":
        F["chains"] = F["chains"][::-1].copy()
    win, warns = kc.replay(**F)
    hwin, hwarn = mga.call_chains_host(**F)
    assert kc.win_of(hwin) == win and kc.warn_of(hwarn) == warns


def test_crafted_cases_are_what_they_claim():
    """what each crafted case must produce, stated once from the reference's rules, so that the GPU tests cannot agree with the replay on empty ground"""
    def one(name):
        return kc.replay(**K.arrays(GROUPS[name]))
    assert one("one_vertex") == ({}, []) and one("nonstem_at_0_later_chain") == ({}, [])
    w, _ = one("nonstem_at_0_first_chain")
    assert list(w) == [2] and w[2][2:4] == (3, 4)
    w, _ = one("two_stems")
    assert list(w) == [1] and w[1][2] == w[1][3]
    for n in (63, 64, 65, 128, 129):
        w, _ = one("walk_%d" % n)
        off = int(K.arrays(GROUPS["walk_%d" % n])["chains"][0]["lc_off"])
        assert list(w) == [1] and (w[1][2] - off, w[1][3] - off) == (1, n - 1)
    w, _ = one("open_at_lane_63")
    off = int(K.arrays(GROUPS["open_at_lane_63"])["chains"][0]["lc_off"])
    assert sorted(w) == [1, 2] and (w[2][2] - off, w[2][3] - off) == (63, 68)
    w, _ = one("open_at_lane_0")
    off = int(K.arrays(GROUPS["open_at_lane_0"])["chains"][0]["lc_off"])
    assert (w[2][2] - off, w[2][3] - off) == (64, 67)
    w, _ = one("three_blocks")
    off = int(K.arrays(GROUPS["three_blocks"])["chains"][0]["lc_off"])
    assert (w[1][2] - off, w[1][3] - off) == (22, 172)
    w, _ = one("stale_st")
    assert sorted(w) == [1, 2, 3] and w[2][2] == w[2][3]
    w, _ = one("qs_gt_qe")
    assert w[2][5] > w[2][6]
    assert list(one("q_touch_one")[0]) == [2] and one("q_two") == ({}, [])
    assert list(one("q_many_one")[0]) == [2] and one("q_many_two") == ({}, [])
    assert one("over_inside") == ({}, []) and list(one("over_outside")[0]) == [2]
    assert one("strand_minus")[0][3][4] == -1
    assert one("equal_bid_src_sum_1")[0][8][4] == -1   # the later chain (reverse walk) overwrites the forward one
    assert [x[1] for x in one("equal_bid_src_sum_2_and_0")[1]] == [1, 1] and one("equal_bid_src_sum_2_and_0")[0] == {}
    assert [x[1] for x in one("foreign_bid")[1]] == [2, 2] and one("foreign_bid")[0] == {}
    assert one("int32_wrap")[0][5][7] == kc.i32(2 * 2147483000)
    assert list(one("not_primary")[0]) == [6]
    w, _ = one("three_compete")
    assert w[7][0] >> 32 == GROUPS["three_compete"][2]
