"""Shared inputs of the --call tests (test_bubble_host.py, test_call_host.py, test_gpu_call.py, test_gpu_call_e2e.py): bindings of the reference's bubble finder, small
hand-written graphs, the flat records of call_core.h made in Python from mg_gchains_t objects, a Python replay of mg_call_asm's scan (asm-call.c:47-115) over those
records, and crafted walks over a crafted segment table whose outcomes the replay predicts."""
import ctypes as C
import os
import subprocess

import numpy as np

import minigraph_amd as mga
import refbind as rb

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the reference library ----

class ref_bubble_t(C.Structure):  # gfa_bubble_t, gfa-priv.h:32-38
    _fields_ = [("snid", C.c_int32), ("ss", C.c_int32), ("se", C.c_int32), ("vs", C.c_uint32), ("ve", C.c_uint32), ("is_bidir", C.c_int32), ("n_seg", C.c_int32),
                ("len_max", C.c_int32), ("len_min", C.c_int32), ("v", C.POINTER(C.c_uint32)), ("n_paths", C.c_uint32), ("seq_max", C.c_char_p), ("seq_min", C.c_char_p)]


class arc_t(C.Structure):  # gfa_arc_t
    _fields_ = [("v_lv", C.c_uint64), ("w", C.c_uint32), ("rank", C.c_int32), ("ov", C.c_int32), ("ow", C.c_int32), ("bits", C.c_uint64)]


class llchain_t(C.Structure):  # mg_llchain_t
    _fields_ = [("off", C.c_int32), ("cnt", C.c_int32), ("v", C.c_uint32), ("score", C.c_int32), ("ed", C.c_int32)]


class cigar_t(C.Structure):  # mg_cigar_t (header)
    _fields_ = [("n_cigar", C.c_int32), ("mlen", C.c_int32), ("blen", C.c_int32), ("aplen", C.c_int32), ("ss", C.c_int32), ("ee", C.c_int32)]


class gchain_t(C.Structure):  # mg_gchain_t
    _fields_ = [(n, C.c_int32) for n in ("id", "parent", "off", "cnt", "n_anchor", "score", "qs", "qe", "plen", "ps", "pe", "blen", "mlen")] + \
               [("div", C.c_float), ("hash", C.c_uint32), ("subsc", C.c_int32), ("n_sub", C.c_int32), ("mapq", C.c_uint32, 8), ("flt", C.c_uint32, 1), ("dummy", C.c_uint32, 23),
                ("p", C.POINTER(cigar_t)), ("ds_len", C.c_int32), ("ds_n_off", C.c_int32), ("ds_off", C.c_void_p), ("ds_ds", C.c_void_p)]


class gchains_t(C.Structure):  # mg_gchains_t
    _fields_ = [("km", C.c_void_p), ("n_gc", C.c_int32), ("n_lc", C.c_int32), ("n_a", C.c_int32), ("rep_len", C.c_int32), ("gc", C.POINTER(gchain_t)),
                ("lc", C.POINTER(llchain_t)), ("a", C.c_void_p)]


assert C.sizeof(gchain_t) == 104 and C.sizeof(gchains_t) == 48 and C.sizeof(llchain_t) == 20 and C.sizeof(ref_bubble_t) == 72


def ref_lib():
    R = C.CDLL(rb.REF_SO)
    R.gfa_read.argtypes, R.gfa_read.restype = [C.c_char_p], C.c_void_p
    R.gfa_destroy.argtypes = [C.c_void_p]
    R.gfa_sort_ref_arc.argtypes, R.gfa_sort_ref_arc.restype = [C.c_void_p], None
    R.gfa_bubble.argtypes, R.gfa_bubble.restype = [C.c_void_p, C.POINTER(C.c_int32)], C.POINTER(ref_bubble_t)
    R.mg_opt_set.argtypes = [C.c_char_p, C.POINTER(mga.idxopt_t), C.POINTER(mga.mapopt_t), C.POINTER(mga.ggopt_t)]
    R.mg_opt_update.argtypes = [C.c_void_p, C.POINTER(mga.mapopt_t), C.POINTER(mga.ggopt_t)]
    R.mg_index.argtypes, R.mg_index.restype = [C.c_void_p, C.POINTER(mga.idxopt_t), C.c_int, C.POINTER(mga.mapopt_t)], C.c_void_p
    R.mg_idx_destroy.argtypes = [C.c_void_p]
    R.mg_tbuf_init.restype = C.c_void_p
    R.mg_tbuf_destroy.argtypes = [C.c_void_p]
    R.mg_map.argtypes, R.mg_map.restype = [C.c_void_p, C.c_int, C.c_char_p, C.c_void_p, C.POINTER(mga.mapopt_t), C.c_char_p], C.c_void_p
    R.mg_gchain_free.argtypes = [C.c_void_p]
    return R


def gfa_fields(g):
    """(n_seg, seg*, n_arc, arc*, idx*) of a gfa_t*"""
    u32, u64 = C.cast(g, C.POINTER(C.c_uint32)), C.cast(g, C.POINTER(C.c_uint64))
    return int(u32[1]), int(u64[2]), int(u64[8]), int(u64[9]), int(u64[11])


def arcs_of(g):
    _, _, n_arc, arc, _ = gfa_fields(g)
    a = C.cast(C.c_void_p(arc), C.POINTER(arc_t))
    return [(a[k].v_lv, a[k].w, a[k].rank, a[k].ov, a[k].ow, a[k].bits) for k in range(n_arc)]


def seg_lens(g):
    n_seg, seg, _, _, _ = gfa_fields(g)
    raw = np.frombuffer(C.string_at(seg, n_seg * 64), dtype=np.int32).reshape(n_seg, 16)   # gfa_seg_t is 64 bytes, len first
    return raw[:, 0].copy()


def ref_bubbles(R, rg):
    n = C.c_int32(0)
    bb = R.gfa_bubble(rg, C.byref(n))
    out = [(bb[i].snid, bb[i].ss, bb[i].se, bb[i].n_seg, [int(bb[i].v[k]) for k in range(bb[i].n_seg)]) for i in range(n.value)]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    for i in range(n.value):
        libc.free(C.cast(bb[i].v, C.c_void_p))
    libc.free(C.cast(bb, C.c_void_p))
    return out


# ---- hand-written graphs: reference path s1 s2 ... of 40-base segments on chr1, alternative segments of rank 1 on stable sequences of their own ----

def _gfa(n_ref, alts, links):
    """alts: names of rank-1 segments; links: (from, strand, to, strand, rank)"""
    out = []
    for i in range(1, n_ref + 1):
        out.append("S\ts%d\t%s\tSN:Z:chr1\tSO:i:%d\tSR:i:0" % (i, "ACGT" * 10, (i - 1) * 40))
    for k, a in enumerate(alts):
        out.append("S\t%s\t%s\tSN:Z:alt_%s\tSO:i:0\tSR:i:1" % (a, "TTGCA" * (3 + k), a))
    for i in range(1, n_ref):
        out.append("L\ts%d\t+\ts%d\t+\t0M\tSR:i:0\tL1:i:40\tL2:i:40" % (i, i + 1))
    for a, sa, b, sb, r in links:
        out.append("L\t%s\t%s\t%s\t%s\t0M\tSR:i:%d\tL1:i:40\tL2:i:40" % (a, sa, b, sb, r))
    return "\n".join(out) + "\n"


# name -> (text, bubbles expected, a segment is listed by two bubbles)
HAND_GRAPHS = {
    "no_bubble": (_gfa(3, [], []), 2, True),   # (no variation: the reference lists every adjacent pair of a linear stretch as a bubble of two stems and nothing between)
    "one_bubble": (_gfa(3, ["a"], [("s1", "+", "a", "+", 1), ("a", "+", "s3", "+", 1)]), 1, False),
    "nested": (_gfa(5, ["a", "b"], [("s2", "+", "a", "+", 1), ("a", "+", "s4", "+", 1), ("s1", "+", "b", "+", 2), ("b", "+", "s5", "+", 2)]), 1, False),
    "deletion": (_gfa(3, [], [("s1", "+", "s3", "+", 1)]), 1, False),
    "inversion": (_gfa(3, [], [("s1", "+", "s2", "-", 1), ("s2", "-", "s3", "+", 1)]), 1, False),
    "cycle": (_gfa(4, ["a"], [("s2", "+", "a", "+", 1), ("a", "+", "s2", "+", 1), ("s1", "+", "s3", "+", 1)]), 2, True),   # (the walk back through a keeps s2 inside; what follows s3 closes as a bubble of its own, in the reference too)
    "no_rank0_sseq": (_gfa(3, ["a", "z"], [("s1", "+", "a", "+", 1), ("a", "+", "s3", "+", 1), ("a", "+", "z", "+", 2), ("z", "+", "s3", "+", 2)]), 1, False),
    "shared_stem": (_gfa(5, ["a", "b"], [("s1", "+", "a", "+", 1), ("a", "+", "s3", "+", 1), ("s3", "+", "b", "+", 1), ("b", "+", "s5", "+", 1)]), 2, True),
}


def write_hand_graph(name, path):
    text, n_bb, multi = HAND_GRAPHS[name]
    with open(path, "w") as f:
        f.write(text)
    return n_bb, multi


# ---- flat records from mg_gchains_t objects (what csrc/call.c makes in C) ----

def i32(x):
    return int(np.int64(x).astype(np.int32)) if isinstance(x, np.integer) else ((int(x) + (1 << 31)) % (1 << 32)) - (1 << 31)


def flat_from_gchains(gcs, lens, bb, bv, min_mapq, min_blen):
    """gcs: mg_gchains_t* per sequence (0 allowed) -> dict of the arrays mga_call_batch takes, or None when nothing is indexed (mg_gc_index returns 0)"""
    n_seg = len(lens)
    n_on, qintv, q_off, chains, pos, max_acnt = np.zeros(n_seg, dtype=np.int64), [], [0], [], [], 0
    for t, ptr in enumerate(gcs):
        if not ptr:
            q_off.append(len(qintv))
            continue
        gt = C.cast(C.c_void_p(ptr), C.POINTER(gchains_t)).contents
        a = np.frombuffer(C.string_at(gt.a, gt.n_a * 16), dtype=mga.m128) if gt.n_a else np.zeros(0, dtype=mga.m128)
        for i in range(gt.n_gc):
            gc = gt.gc[i]
            walk = [gt.lc[gc.off + j] for j in range(gc.cnt)]
            if gc.id == gc.parent and gc.blen >= min_blen and gc.mapq >= min_mapq:
                max_acnt = max(max_acnt, gc.n_anchor)
                qintv.append((gc.qs, gc.qe))
                for j, lc in enumerate(walk):
                    ln = int(lens[lc.v >> 1])
                    rs, re = 0, ln
                    if lc.cnt > 0:
                        q0, q1 = a[lc.off], a[lc.off + lc.cnt - 1]
                        if j == 0:
                            rs = gc.p.contents.ss if gc.p else i32(int(q0["x"]) & 0xffffffff) + 1 - (int(q0["y"]) >> 32 & 0xff)
                        if j == gc.cnt - 1:
                            re = gc.p.contents.ee if gc.p else i32(int(q1["x"]) & 0xffffffff)
                        if lc.v & 1:
                            rs, re = ln - re, ln - rs
                    if rs < ln and 0 < re:
                        n_on[lc.v >> 1] += 1
            chains.append((len(pos), gc.cnt, gc.off, t, len(chains)))
            for lc in walk:
                last, first = max(lc.off + lc.cnt - 1, 0), lc.off
                pos.append((lc.v, i32(int(a[last]["y"]) & 0xffffffff) + 1, i32(int(a[first]["y"]) & 0xffffffff) + 1, int(a[first]["y"]) >> 32 & 0xff))
        q_off.append(len(qintv))
    if max_acnt == 0:
        return None
    seg = np.zeros(n_seg, dtype=mga.call_seg_dtype)
    seg["over"] = n_on > 1
    for i, b in enumerate(bb):
        v = bv[b["v_off"]:b["v_off"] + b["n_seg"]]
        seg["bid"][v >> 1] = i
        seg["is_stem"][v[0] >> 1] = seg["is_stem"][v[-1] >> 1] = 1
        seg["is_src"][v[0] >> 1] = 1
    return dict(chains=np.array(chains, dtype=mga.call_chain_dtype), pos=np.array(pos, dtype=mga.call_pos_dtype), seg=seg, seg_len=np.asarray(lens, dtype=np.int32),
                q_off=np.array(q_off, dtype=np.int64), qintv=np.array(qintv, dtype=mga.call_intv_dtype).reshape(-1), n_bb=len(bb))


# ---- the replay: asm-call.c:47-115 over the flat records, written as the reference writes it (a scalar loop with a running st; no sums, no scans) ----

def replay(chains, pos, seg, seg_len, q_off, qintv, n_bb):
    """-> (win: {bid: (key, bid, st, en, strand, qs, qe, glen, t)}, warnings [(key, type, t, qs, qe, v)] in key order)"""
    win, warns = {}, []
    for c in sorted(chains, key=lambda c: int(c["ord"])):
        p = pos[int(c["pos_beg"]):int(c["pos_beg"]) + int(c["cnt"])]
        ca = seg[p["v"] >> 1]
        t, off, st = int(c["t"]), int(c["lc_off"]), -1
        qa = qintv[int(q_off[t]):int(q_off[t + 1])]
        for j in range(1, len(p)):
            cur, prev = bool(ca[j]["is_stem"]), bool(ca[j - 1]["is_stem"])
            if not cur and prev:
                st = off + j
                continue
            if not ((cur and not prev and st > 0) or (cur and prev)):
                continue
            en = off + j
            if cur and prev:
                st = off + j
            s, e = st - off, en - off
            qs, qe = int(p[s - 1]["yl1"]), i32(int(p[e]["yf1"]) - int(p[s]["span"]))
            if sum(1 for a in qa if a["st"] < qe and qs < a["en"]) > 1:
                continue
            glen, bad = 0, False
            for k in range(s, e):
                glen = i32(glen + int(seg_len[p[k]["v"] >> 1]))
                if ca[k]["over"]:
                    bad = True
                    break
            if bad:
                continue
            A, B = ca[s - 1], ca[e]
            key = int(c["ord"]) << 32 | j
            if A["bid"] < B["bid"]:
                strand = 1
            elif A["bid"] > B["bid"]:
                strand = -1
            else:
                if int(A["is_src"]) + int(B["is_src"]) != 1:
                    warns.append((key, 1, t, qs, qe, int(p[s]["v"])))
                    continue
                strand = 1 if A["is_src"] else -1
            bid = int(A["bid"] if strand > 0 else B["bid"])
            if any(int(ca[k]["bid"]) != bid for k in range(s, e)):
                warns.append((key, 2, t, qs, qe, int(p[s]["v"])))
                continue
            win[bid] = (key, bid, st, en, strand, qs, qe, glen, t)   # (t, i, j) order: the last one stays
    return win, warns


def win_of(rec):
    """the winners an entry point returned, in the replay's form"""
    return {int(r["bid"]): tuple(int(r[f]) for f in ("key", "bid", "st", "en", "strand", "qs", "qe", "glen", "t")) for r in rec if int(r["key"]) != 0}


def warn_of(rec):
    return [tuple(int(r[f]) for f in ("key", "type", "t", "qs", "qe", "v")) for r in rec]


# ---- crafted walks over a crafted segment table ----
# stems T0 .. T9 = segments 0 .. 9 of a chain of bubbles 0 .. 8 (bubble i: T_i -> T_{i+1}; a stem between two bubbles carries the later one's id, T9 the id 8);
# inner segments of bubble i: 10 + 2 i and 11 + 2 i; 28: in no bubble; 29: inner of bubble 3 carrying two indexed intervals; 30, 31: stems of bubble 10, BOTH sources;
# 32, 33: stems of bubble 11, NEITHER a source; 34 / 35: inner of 10 / 11; 36: inner of bubble 5, 2 147 483 000 bases (two of them wrap an int32)
N_BB, N_CSEG = 12, 37


def crafted_table():
    seg = np.zeros(N_CSEG, dtype=mga.call_seg_dtype)
    for i in range(10):
        seg[i] = (min(i, 8), 1, 1 if i < 9 else 0, 0, 0)
    for i in range(9):
        seg[10 + 2 * i] = seg[11 + 2 * i] = (i, 0, 0, 0, 0)
    seg[29] = (3, 0, 0, 1, 0)
    seg[30] = seg[31] = (10, 1, 1, 0, 0)
    seg[32] = seg[33] = (11, 1, 0, 0, 0)
    seg[34], seg[35], seg[36] = (10, 0, 0, 0, 0), (11, 0, 0, 0, 0), (5, 0, 0, 0, 0)
    lens = np.array([100 + 7 * i for i in range(N_CSEG)], dtype=np.int32)
    lens[36] = 2147483000
    return seg, lens


def T(i):
    return i << 1


def run(b, n):
    return [(10 + 2 * b + (k & 1)) << 1 for k in range(n)]


def rev(walk):
    return [v ^ 1 for v in reversed(walk)]


# query intervals per sequence: 0: one interval over everything; 1: two that meet at 5000; 2: none; 3: 130 intervals, one (index 100) in reach; 4: 130, two (3 and 127) in reach
Q_INTV = [[(0, 10 ** 9)], [(0, 5000), (5000, 10 ** 9)], [], [(-10 - k, -5 - k) for k in range(100)] + [(0, 10 ** 9)] + [(-900 - k, -800) for k in range(29)],
          [(-10 - k, -5 - k) for k in range(3)] + [(0, 10 ** 9)] + [(-900 - k, -800) for k in range(123)] + [(10, 10 ** 9)] + [(-7, -6), (-9, -8)]]


class Crafted:
    """chains in (t, i) order; add() returns the chain's ordinal"""

    def __init__(self):
        self.chains, self.pos, self.lc_next = [], [], {}

    def add(self, t, walk, y0=10000, over=None):
        """position k of the walk: first anchor at y0 + 1000 k + 50, last at y0 + 1000 k + 900, span 19; over: {k: (yl1, yf1, span)} replaces a position's"""
        off = self.lc_next.get(t, 0)
        self.lc_next[t] = off + len(walk)
        self.chains.append((len(self.pos), len(walk), off, t, len(self.chains)))
        for k, v in enumerate(walk):
            self.pos.append((v,) + tuple((over or {}).get(k, (y0 + 1000 * k + 901, y0 + 1000 * k + 51, 19))))
        return len(self.chains) - 1

    def arrays(self, only=None, order=None):
        """only: ordinals to keep (their records keep ord, pos_beg, lc_off); order: a permutation of the kept records = the launch order"""
        seg, lens = crafted_table()
        ch = np.array(self.chains, dtype=mga.call_chain_dtype)
        if only is not None:
            ch = ch[sorted(only)]
        if order is not None:
            ch = ch[order]
        q_off = np.cumsum([0] + [len(q) for q in Q_INTV]).astype(np.int64)
        qi = np.array([x for q in Q_INTV for x in q], dtype=mga.call_intv_dtype)
        return dict(chains=ch, pos=np.array(self.pos, dtype=mga.call_pos_dtype), seg=seg, seg_len=lens, q_off=q_off, qintv=qi, n_bb=N_BB)


def crafted():
    """-> (Crafted, groups {name: ordinals}); every group is a case of the issue's list"""
    K, G = Crafted(), {}
    G["nonstem_at_0_first_chain"] = [K.add(0, run(1, 2) + [T(2)] + run(2, 1) + [T(3)])]       # the run at position 0 closes nothing; [3, 4) of bubble 2 does
    G["one_vertex"] = [K.add(0, [T(1)])]
    G["two_stems"] = [K.add(0, [T(1), T(2)])]                                                  # a deletion at j = 1, st == en
    G["nonstem_at_0_later_chain"] = [K.add(0, run(4, 3) + [T(5)])]                             # lc_off > 0, still no candidate
    for n in (63, 64, 65, 128, 129):                                                           # one run from j = 1 to the last vertex: closes at lane 62, 63, 0, 63, 0
        G["walk_%d" % n] = [K.add(0, [T(1)] + run(1, n - 2) + [T(2)])]
    G["open_at_lane_63"] = [K.add(0, [T(1)] + run(1, 61) + [T(2)] + run(2, 5) + [T(3)])]       # stem at 62, the run opens at j = 63 and closes in the next block
    G["open_at_lane_0"] = [K.add(0, [T(1)] + run(1, 62) + [T(2)] + run(2, 3) + [T(3)])]        # stem at 63, the run opens at j = 64
    G["three_blocks"] = [K.add(0, [T(0)] + run(0, 20) + [T(1)] + run(1, 150) + [T(2)])]        # opens at j = 22, closes at j = 172
    G["stale_st"] = [K.add(0, [T(1)] + run(1, 1) + [T(2), T(3)] + run(3, 2) + [T(4)])]
    G["qs_gt_qe"] = [K.add(0, [T(2)] + run(2, 1) + [T(3)], over={0: (90000, 51, 19)})]
    G["q_touch_one"] = [K.add(1, [T(2)] + run(2, 1) + [T(3)], over={0: (5000, 51, 19)})]       # [5000, ..): the first interval only touches -> 1 overlap, kept
    G["q_two"] = [K.add(1, [T(3)] + run(3, 1) + [T(4)], over={0: (4999, 51, 19)})]             # both overlap -> dropped
    G["q_many_one"] = [K.add(3, [T(2)] + run(2, 1) + [T(3)])]
    G["q_many_two"] = [K.add(4, [T(2)] + run(2, 1) + [T(3)])]
    G["over_inside"] = [K.add(0, [T(3), 29 << 1, T(4)])]
    G["over_outside"] = [K.add(0, [29 << 1, T(2)] + run(2, 1) + [T(3)])]
    G["strand_minus"] = [K.add(0, rev([T(3)] + run(3, 2) + [T(4)]))]
    G["equal_bid_src_sum_1"] = [K.add(0, [T(8)] + run(8, 1) + [T(9)]), K.add(0, rev([T(8)] + run(8, 2) + [T(9)]))]
    G["equal_bid_src_sum_2_and_0"] = [K.add(0, [30 << 1, 34 << 1, 31 << 1]), K.add(0, [32 << 1, 35 << 1, 33 << 1 | 1])]
    G["foreign_bid"] = [K.add(0, [T(4)] + run(4, 1) + [28 << 1] + run(4, 1) + [T(5)]), K.add(0, [T(4), 28 << 1, T(5)])]
    G["int32_wrap"] = [K.add(0, [T(5), 36 << 1, 36 << 1, T(6)])]
    G["not_primary"] = [K.add(2, [T(6)] + run(6, 2) + [T(7)])]                                 # sequence 2 has no interval at all
    a = K.add(0, [T(7)] + run(7, 1) + [T(8)])
    for _ in range(6):
        K.add(2, [T(1)])
    b = K.add(0, [T(7)] + run(7, 3) + [T(8)])
    for _ in range(5):
        K.add(2, [T(1)])
    c = K.add(0, [T(7)] + run(7, 2) + [T(8)])
    assert len({a >> 2, b >> 2, c >> 2}) == 3                                                  # three workgroups
    G["three_compete"] = [a, b, c]
    return K, G


# ---- files ----

def mgsim_asm(d, seed=5):
    """the workload of test_dropin_call_and_graph_generation_consume_our_chains -- eight 300 kb contigs at 0.4 % divergence on a 3-haplotype bubble graph -- on a graph of
    4 Mbp and seed 5: the reference's BED then has 78 lines with a walk and 109 '.' (at 1.5 Mbp the contigs overlap each other and the seeds tried stay below 50 walks)"""
    subprocess.check_call([mga.MGSIM, "-p", os.path.join(d, "t"), "-G", "4000000", "-H", "3", "-n", "8", "-l", "300000", "-e", "0.004", "-s", str(seed)], stderr=subprocess.DEVNULL)
    return os.path.join(d, "t.gfa"), os.path.join(d, "t.reads.fa")


def ref_call(graph, query, out, cigar=True, extra=()):
    """the reference binary's BED"""
    with open(out, "wb") as fo:
        subprocess.check_call([rb.REF_BIN] + (["-c"] if cigar else []) + ["-x", "asm", "--call", "-t", "4"] + list(extra) + [graph, query], stdout=fo, stderr=subprocess.DEVNULL, timeout=600)
    return open(out, "rb").read()


def bed_is_ground(bed):
    """the issue's two conditions on the reference's BED: at least 50 lines carry a walk, at least one is '.'"""
    col6 = [l.split(b"\t")[5] for l in bed.splitlines()]
    return sum(1 for c in col6 if c not in (b".", b"")) >= 50 and sum(1 for c in col6 if c == b".") >= 1
