"""Shared inputs of the coverage tests (test_cov_host.py, test_gpu_cov.py): a synthetic chain graph whose arcs are tampered in memory, flat chain
records over it, and the small fixtures of the whole-job tests."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import minigraph_amd as mga

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MG_M_CAL_COV, MG_M_FRAG_MODE, MG_M_SKIP_GCHECK = 0x4000, 0x40, 0x2000000
N_SEG, BIG, BIG_LEN, SEG_LEN = 1200, 5, 100000, 60   # s0 .. s1199 in a line, 60 bases each, s5 of 100 000; an extra link s0+ -> s2+
DUP_AT, MISS_AT = 0, 10   # after tampering: two arcs s0+ -> s1+ (several: skipped); no arc s11- -> s10- (the walk s10+ s11+ is skipped)


class arc_t(C.Structure):  # gfa_arc_t
    _fields_ = [("v_lv", C.c_uint64), ("w", C.c_uint32), ("rank", C.c_int32), ("ov", C.c_int32), ("ow", C.c_int32), ("bits", C.c_uint64)]


def write_chain_gfa(path, seed=7):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        off = 0
        for i in range(N_SEG):
            n = BIG_LEN if i == BIG else SEG_LEN
            f.write(b"S\ts%d\t%s\tSN:Z:chr\tSO:i:%d\tSR:i:0\n" % (i, rng.choice(acgt, size=n).tobytes(), off))
            off += n
        for i in range(N_SEG - 1):
            f.write(b"L\ts%d\t+\ts%d\t+\t0M\tSR:i:0\n" % (i, i + 1))
        f.write(b"L\ts0\t+\ts2\t+\t0M\tSR:i:1\n")


def graph_arrays(g):
    """(arc array view, idx array view, n_seg, n_arc) of a gfa_t*"""
    n_seg, n_arc = mga._cov_sizes(g)
    u64 = C.cast(g, C.POINTER(C.c_uint64))
    arc = C.cast(C.c_void_p(int(u64[9])), C.POINTER(arc_t))
    idx = C.cast(C.c_void_p(int(u64[11])), C.POINTER(C.c_uint64))
    return arc, idx, n_seg, n_arc


def tamper(g):
    """a duplicate arc and a missing reverse arc, made in memory (a finalized graph read from a file is always symmetric)"""
    arc, idx, _, _ = graph_arrays(g)

    def arcs_of(v):
        x = int(idx[v])
        return [(x >> 32) + i for i in range(x & 0xffffffff)]
    a0 = arcs_of(DUP_AT << 1)
    assert sorted(arc[k].w for k in a0) == [1 << 1, 2 << 1]
    for k in a0:
        arc[k].w = 1 << 1
    rv = arcs_of((MISS_AT + 1) << 1 | 1)
    assert [arc[k].w for k in rv] == [MISS_AT << 1 | 1]
    arc[rv[0]].w = (MISS_AT - 1) << 1 | 1


def find_arc(g, v, w):
    arc, idx, _, _ = graph_arrays(g)
    x = int(idx[v])
    hit = [(x >> 32) + i for i in range(x & 0xffffffff) if arc[(x >> 32) + i].w == w]
    return hit[0] if len(hit) == 1 else -1 if not hit else -2


def seg_lens():
    return np.array([BIG_LEN if i == BIG else SEG_LEN for i in range(N_SEG)], dtype=np.int64)


class Cases:
    """flat chain records + walks"""

    def __init__(self):
        self.rec, self.vert = [], []

    def add(self, walk, ps=3, tail=5, mapq=60, blen=5000):
        """walk: oriented vertices; the chain starts at base ps of the first segment and ends `tail` bases before the end of the last"""
        lens = seg_lens()
        plen = int(sum(lens[v >> 1] for v in walk))
        self.rec.append((len(self.vert), len(walk), ps, plen - tail, plen, mapq, blen))
        self.vert.extend(walk)

    def arrays(self):
        return np.array(self.rec, dtype=mga.cov_chain_dtype), np.array(self.vert, dtype=np.uint32)


def fwd(first, n):
    return [(first + j) << 1 for j in range(n)]


def rev(first, n):
    return [(first - j) << 1 | 1 for j in range(n)]


def bubble_fixture(d):
    """an mgsim bubble graph with 200 reads of 5 kb: (graph, reads)"""
    subprocess.check_call([mga.MGSIM, "-p", os.path.join(d, "t"), "-G", "200000", "-H", "3", "-n", "200", "-l", "5000", "-s", "5"], stderr=subprocess.DEVNULL)
    return os.path.join(d, "t.gfa"), os.path.join(d, "t.reads.fa")


def mt_fixture():
    return os.path.join(GOLD, "MT.gfa"), [os.path.join(GOLD, "MT-orangA.fa"), os.path.join(GOLD, "MT-chimp.fa")]


def options(preset="lr", cigar=True, flags=0, **map_opt):
    L = mga.load()
    io, mo, go = mga.idxopt_t(), mga.mapopt_t(), mga.ggopt_t()
    L.mg_opt_set(None, C.byref(io), C.byref(mo), C.byref(go))
    assert L.mg_opt_set(preset.encode(), C.byref(io), C.byref(mo), C.byref(go)) == 0
    if cigar:
        mo.flag |= mga.MG_M_CIGAR
    mo.flag |= flags
    for k, v in map_opt.items():
        setattr(mo, k, v)
    return io, mo, go


def ref_print(ref_lib, g, path):
    """gfa_print of the reference library on a gfa_t* into a file"""
    libc = C.CDLL(None)
    libc.fopen.restype, libc.fopen.argtypes, libc.fclose.argtypes = C.c_void_p, [C.c_char_p, C.c_char_p], [C.c_void_p]
    ref_lib.gfa_print.argtypes, ref_lib.gfa_print.restype = [C.c_void_p, C.c_void_p, C.c_int], None
    fp = libc.fopen(path.encode(), b"wb")
    assert fp
    ref_lib.gfa_print(g, C.c_void_p(fp), 0)
    libc.fclose(C.c_void_p(fp))
    return open(path, "rb").read()
