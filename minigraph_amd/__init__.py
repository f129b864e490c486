"""minigraph_amd -- thin ctypes loader for libminigraph_amd.so (the C-ABI product library).

Python is plumbing here (tests, bench harness); the product is the shared library built from
``minigraph_amd/csrc`` (host C + hand-written HIP kernels for gfx950).  There is NO CPU fallback:
if the library is missing, ``load()`` raises, and every entry point fails when no GPU is visible.
"""
import ctypes as C
import os
import subprocess

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
LIB_PATH = os.environ.get("MGA_LIB") or os.path.join(PKG, "lib", "libminigraph_amd.so")  # MGA_LIB: a test build of the same library (tests/test_wave_model.py)
MGSIM = os.path.join(PKG, "lib", "mgsim")

m128 = np.dtype([("x", "<u8"), ("y", "<u8")])

_lib = None


def build(verbose=False):
    """Compile the library (hipcc --offload-arch=gfx950 + gcc) and the workload generator in-tree."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j8"], stdout=out)
    os.makedirs(os.path.join(PKG, "lib"), exist_ok=True)
    subprocess.check_call(["gcc", "-O2", "-o", MGSIM, os.path.join(PKG, "tools", "mgsim.c")], stdout=out)


class lchain_par_t(C.Structure):
    _fields_ = [("max_dist_x", C.c_int32), ("max_dist_y", C.c_int32), ("bw", C.c_int32), ("max_skip", C.c_int32),
                ("max_iter", C.c_int32), ("min_cnt", C.c_int32), ("min_sc", C.c_int32),
                ("chn_pen_gap", C.c_float), ("chn_pen_skip", C.c_float)]


class idxopt_t(C.Structure):
    _fields_ = [("w", C.c_int), ("k", C.c_int), ("bucket_bits", C.c_int)]


class mapopt_t(C.Structure):  # minigraph.h:51-77
    _fields_ = [("flag", C.c_uint64), ("mini_batch_size", C.c_int64), ("seed", C.c_int), ("max_qlen", C.c_int),
                ("pe_ori", C.c_int), ("occ_max1", C.c_int), ("occ_max1_cap", C.c_int), ("occ_max1_frac", C.c_float),
                ("bw", C.c_int), ("bw_long", C.c_int), ("rmq_size_cap", C.c_int), ("rmq_rescue_size", C.c_int),
                ("rmq_rescue_ratio", C.c_float), ("max_gap_pre", C.c_int), ("max_gap", C.c_int),
                ("max_gap_ref", C.c_int), ("max_frag_len", C.c_int), ("div", C.c_float), ("chn_pen_gap", C.c_float),
                ("chn_pen_skip", C.c_float), ("max_lc_skip", C.c_int), ("max_lc_iter", C.c_int),
                ("max_gc_skip", C.c_int), ("min_lc_cnt", C.c_int), ("min_lc_score", C.c_int), ("min_gc_cnt", C.c_int),
                ("min_gc_score", C.c_int), ("gdp_max_ed", C.c_int), ("lc_max_trim", C.c_int), ("lc_max_occ", C.c_int),
                ("mask_level", C.c_float), ("sub_diff", C.c_int), ("best_n", C.c_int), ("pri_ratio", C.c_float),
                ("ref_bonus", C.c_int), ("cap_kalloc", C.c_int64), ("min_cov_mapq", C.c_int), ("min_cov_blen", C.c_int)]


class ggopt_t(C.Structure):
    _fields_ = [("flag", C.c_uint64), ("algo", C.c_int), ("min_mapq", C.c_int), ("min_map_len", C.c_int),
                ("min_depth_len", C.c_int), ("min_var_len", C.c_int), ("match_pen", C.c_int),
                ("ggs_shrink_pen", C.c_int), ("ggs_min_end_cnt", C.c_int), ("ggs_min_end_frac", C.c_float),
                ("ggs_max_iden", C.c_float), ("ggs_min_inv_iden", C.c_float)]


MG_M_CIGAR = 0x4000000

KERNELS = ["k_sketch", "k_seed_count", "k_seed_fill", "k_lchain", "k_wfa_r[64]", "k_wfa_r[128]", "k_wfa_r[192]", "k_wfa_r[256]", "k_wfa_r[512]",
           "k_wfa_r[1024]", "k_wfa_r[2048]", "k_wfa[hbm4096]", "k_wfa[hbm32768]", "k_scan", "k_text", "k_gchain", "k_plan",
           "k_wfa_w[16x4]", "k_wfa_w[32x2]", "k_wfa_w[64]", "k_wfa_w[128]", "k_wfa_w[192]", "k_wfa_w[256]", "k_wfa_tb", "k_gchain_p2", "k_gchain_p3", "k_gaf", "k_cov"]


class stats_t(C.Structure):  # mga_stats_t
    _fields_ = [(n, C.c_int64) for n in ("n_reads", "n_bases", "n_mz", "n_probe", "n_hit", "n_anchor_chained", "n_wfa",
                                         "wfa_t_bases", "wfa_q_bases", "wfa_cells", "gaf_bytes")] + \
               [(n, C.c_double) for n in ("t_sketch", "t_seed", "t_lchain", "t_host_chain", "t_wfa", "t_host_post", "t_gaf")] + \
               [(n, C.c_int64) for n in ("n_rescue_dev", "n_rescue_host", "n_gwfa", "n_shortk", "n_gc_retry", "gc_arena_peak", "n_wfa_dev_plan", "n_gc_host")]


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the HIP path)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    pp = C.POINTER(C.c_void_p)
    L.mga_free.argtypes = [C.c_void_p]
    L.mga_device_count.restype = C.c_int
    L.mga_last_error.restype = C.c_char_p
    L.mga_sketch_batch.argtypes = [C.c_int, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, pp, pp]
    L.mga_wfa_batch.argtypes = [C.c_int, C.c_char_p, C.c_void_p, C.c_char_p, C.c_void_p, pp, pp, pp]
    L.mga_wfa_seg_batch.argtypes = [C.c_int, C.c_char_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_int32, pp, pp, pp]
    L.mga_wfa_seg_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.mga_wfa_seg_bytes.restype = C.c_int64
    L.mga_wfa_seg_step.argtypes = [C.c_int32, C.c_int32]
    L.mga_wfa_seg_step.restype = C.c_int32
    L.mga_wfa_seg_stats.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]
    L.mga_wfa_seg_stats.restype = None
    L.gfa_read.argtypes = [C.c_char_p]
    L.gfa_read.restype = C.c_void_p
    L.gfa_destroy.argtypes = [C.c_void_p]
    L.mg_opt_set.argtypes = [C.c_char_p, C.POINTER(idxopt_t), C.POINTER(mapopt_t), C.POINTER(ggopt_t)]
    L.mg_index.argtypes = [C.c_void_p, C.POINTER(idxopt_t), C.c_int, C.POINTER(mapopt_t)]
    L.mg_index.restype = C.c_void_p
    L.mg_idx_destroy.argtypes = [C.c_void_p]
    L.mga_graph_image_save.argtypes = [C.c_void_p, C.c_char_p]
    L.mga_index_load_image.argtypes = [C.c_char_p, C.POINTER(idxopt_t), C.c_int, C.POINTER(mapopt_t)]
    L.mga_index_load_image.restype = C.c_void_p
    L.mga_seed_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, pp, pp, pp, pp, pp]
    L.mga_lchain_batch.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(lchain_par_t), pp, pp, pp, pp]
    L.mga_lchain_rescue_batch.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(lchain_par_t), C.POINTER(rescue_par_t), C.c_void_p, pp, pp, pp, pp, C.c_void_p]
    L.mga_lchain_rescue_batch.restype = C.c_int
    L.mga_rmq_fwd_batch.argtypes = [C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_float, C.c_float] + [C.c_void_p] * 4
    L.mga_rmq_fwd_batch.restype = C.c_int
    L.mga_map_files_to_path.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(idxopt_t),
                                        C.POINTER(mapopt_t), C.c_int, C.c_char_p]
    L.mga_map_files_shard.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(mapopt_t), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      pp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), pp, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.mga_reads_shard_dump.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_char_p, pp, C.POINTER(C.c_int)]
    L.mga_reads_load.argtypes = [C.c_char_p, C.c_int64]
    L.mga_reads_load.restype = C.c_void_p
    L.mga_reads_free.argtypes = [C.c_void_p]
    L.mga_reads_count.argtypes = [C.c_void_p]
    L.mga_reads_bases.argtypes = [C.c_void_p]
    L.mga_reads_bases.restype = C.c_int64
    L.mga_map_reads.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(mapopt_t), C.c_int, pp, C.POINTER(C.c_int64)]
    L.mga_get_stats.argtypes = [C.c_void_p, C.POINTER(stats_t), C.c_int]
    L.mga_prof_enable.argtypes = [C.c_int]
    L.mga_idx_stream_close.argtypes = [C.c_void_p]
    L.mga_prof_get.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    _lib = L
    return L


def _take(ptr, n, dtype):
    """copy n items out of a malloc'ed C buffer and release it"""
    L = load()
    out = np.empty(n, dtype=dtype)
    if n and ptr.value:
        C.memmove(out.ctypes.data, ptr.value, out.nbytes)
    if ptr.value:
        L.mga_free(ptr)
    return out


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (what, load().mga_last_error().decode()))


def concat(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    if len(seqs):
        off[1:] = np.cumsum([len(s) for s in seqs])
    return b"".join(seqs), off


def sketch_batch(seqs, w, k, rid=None):
    """mg_sketch for a list of byte strings -> list of m128 arrays (HIP kernel k_sketch)."""
    L = load()
    buf, off = concat(seqs)
    mz, mzo = C.c_void_p(), C.c_void_p()
    r = None if rid is None else np.ascontiguousarray(rid, dtype=np.uint32)
    _check(L.mga_sketch_batch(len(seqs), buf, off.ctypes.data, None if r is None else r.ctypes.data, w, k,
                              C.byref(mz), C.byref(mzo)), "mga_sketch_batch")
    o = _take(mzo, len(seqs) + 1, np.int64)
    a = _take(mz, int(o[-1]), m128)
    return [a[o[i]:o[i + 1]] for i in range(len(seqs))]


def wfa_batch(targets, queries):
    """exact miniwfa alignment of n (target, query) pairs -> (scores, list of uint32 cigar arrays)."""
    return _wfa_batch(targets, queries, None)


def wfa_seg_batch(targets, queries, step=0):
    """the same alignments through the low-memory rung alone (k_wfa_seg.hip: a snapshot every `step` scores, then a second pass whose
    band restarts at the checkpoints); step 0: the host's choice.  Score and CIGAR equal wfa_batch's for every step."""
    return _wfa_batch(targets, queries, int(step))


def wfa_seg_stats(reset=False):
    """problems the low-memory rung solved and snapshots it took since the last reset"""
    p, s = C.c_int64(0), C.c_int64(0)
    load().mga_wfa_seg_stats(C.byref(p), C.byref(s), 1 if reset else 0)
    return {"problems": p.value, "snapshots": s.value}


def wfa_seg_bytes(tl, ql, step=0):
    """workspace in bytes the low-memory rung reserves for one tl x ql problem (formula: include/minigraph_amd.h); no GPU involved"""
    return int(load().mga_wfa_seg_bytes(tl, ql, step))


def wfa_seg_step(tl, ql):
    """the snapshot distance the host chooses for a tl x ql problem (MGA_WFA_SEG_STEP, else the one of least memory)"""
    return int(load().mga_wfa_seg_step(tl, ql))


def _wfa_batch(targets, queries, seg_step):
    L = load()
    tb, to = concat(targets)
    qb, qo = concat(queries)
    sc, cg, co = C.c_void_p(), C.c_void_p(), C.c_void_p()
    if seg_step is None:
        _check(L.mga_wfa_batch(len(targets), tb, to.ctypes.data, qb, qo.ctypes.data, C.byref(sc), C.byref(cg), C.byref(co)),
               "mga_wfa_batch")
    else:
        _check(L.mga_wfa_seg_batch(len(targets), tb, to.ctypes.data, qb, qo.ctypes.data, seg_step, C.byref(sc), C.byref(cg), C.byref(co)),
               "mga_wfa_seg_batch")
    n = len(targets)
    o = _take(co, n + 1, np.int64)
    s = _take(sc, n, np.int32)
    c = _take(cg, int(o[-1]), np.uint32)
    return s, [c[o[i]:o[i + 1]] for i in range(n)]


class Graph:
    """gfa_read() + mg_index(): the graph and its minimizer index (host + HBM replica)."""

    def __init__(self, path, preset="lr", cigar=True, n_threads=4, image=False):
        """image=True: `path` is a graph image written by save_image() (mga_graph_image_save): mapped, not parsed; the index owns the graph"""
        L = load()
        self.io, self.mo, self.go = idxopt_t(), mapopt_t(), ggopt_t()
        L.mg_opt_set(None, C.byref(self.io), C.byref(self.mo), C.byref(self.go))
        if L.mg_opt_set(preset.encode(), C.byref(self.io), C.byref(self.mo), C.byref(self.go)) != 0:
            raise ValueError("unknown preset %r" % preset)
        if cigar:
            self.mo.flag |= MG_M_CIGAR
        if image:
            self.g = None
            self.gi = L.mga_index_load_image(path.encode(), C.byref(self.io), n_threads, C.byref(self.mo))
            if not self.gi:
                raise RuntimeError("mga_index_load_image(%s) failed: %s" % (path, L.mga_last_error().decode()))
            return
        self.g = L.gfa_read(path.encode())
        if not self.g:
            raise RuntimeError("gfa_read(%s) failed" % path)
        self.gi = L.mg_index(self.g, C.byref(self.io), n_threads, C.byref(self.mo))
        if not self.gi:
            raise RuntimeError("mg_index failed: %s" % L.mga_last_error().decode())

    def save_image(self, path):
        """the graph as one binary image (mga_graph_image_save): Graph(path, image=True) maps it instead of parsing GFA text"""
        if not self.g:
            raise RuntimeError("this graph was loaded from an image")
        _check(load().mga_graph_image_save(self.g, path.encode()), "mga_graph_image_save")

    def close(self):
        L = load()
        if self.gi:
            L.mg_idx_destroy(self.gi)
        if self.g:
            L.gfa_destroy(self.g)
        self.gi = self.g = None

    def seed_batch(self, mz_list, max_occ=None):
        """collect_seed_hits for each read's minimizers -> list of (anchors, rep_len, mini_pos)"""
        L = load()
        n = len(mz_list)
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(m) for m in mz_list])
        flat = np.ascontiguousarray(np.concatenate(mz_list)) if n else np.zeros(0, dtype=m128)
        a, ao, rl, mp, mo = (C.c_void_p() for _ in range(5))
        _check(L.mga_seed_batch(self.gi, n, flat.ctypes.data, off.ctypes.data,
                                self.mo.occ_max1 if max_occ is None else max_occ,
                                C.byref(a), C.byref(ao), C.byref(rl), C.byref(mp), C.byref(mo)), "mga_seed_batch")
        aoff = _take(ao, n + 1, np.int64)
        moff = _take(mo, n + 1, np.int64)
        aa = _take(a, int(aoff[-1]), m128)
        rep = _take(rl, n, np.int32)
        mini = _take(mp, int(moff[-1]), np.int32)
        return [(aa[aoff[i]:aoff[i + 1]], int(rep[i]), mini[moff[i]:moff[i + 1]]) for i in range(n)]


class rescue_par_t(C.Structure):  # mga_rescue_par_t
    _fields_ = [("enabled", C.c_int32), ("max_dist", C.c_int32), ("max_dist_inner", C.c_int32), ("bw", C.c_int32), ("max_skip", C.c_int32),
                ("cap", C.c_int32), ("min_cnt", C.c_int32), ("min_sc", C.c_int32), ("chn_pen_gap", C.c_float), ("chn_pen_skip", C.c_float),
                ("rescue_size", C.c_int32), ("rescue_ratio", C.c_float), ("frag_len", C.c_int32), ("frag_min_gap", C.c_int32)]


def lchain_batch(anchor_list, rescue=None, qlens=None, **kw):
    """mg_lchain_dp for each read's x-sorted anchors -> list of (u, compacted anchors).
    rescue=dict(max_dist, max_dist_inner, bw, max_skip, cap, min_cnt, min_sc, pen_gap, pen_skip, rescue_size, rescue_ratio) with qlens (one query length per read):
    the long-join rescue of the kernel is on (map-algo.c:407-417) -> list of (u, compacted anchors, flag), flag 0 first-pass chains / 1 rescued / 2 rescue due, handed back"""
    L = load()
    n = len(anchor_list)
    par = lchain_par_t(kw.get("max_dist_x", 5000), kw.get("max_dist_y", 5000), kw.get("bw", 500),
                       kw.get("max_skip", 25), kw.get("max_iter", 5000), kw.get("min_cnt", 5), kw.get("min_sc", 40),
                       kw.get("pen_gap", 1.0), kw.get("pen_skip", 0.05))
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(a) for a in anchor_list])
    flat = np.ascontiguousarray(np.concatenate(anchor_list)) if n else np.zeros(0, dtype=m128)
    u, uo, b, bo = (C.c_void_p() for _ in range(4))
    flag = None
    if rescue is None:
        _check(L.mga_lchain_batch(n, flat.ctypes.data, off.ctypes.data, C.byref(par), C.byref(u), C.byref(uo),
                                  C.byref(b), C.byref(bo)), "mga_lchain_batch")
    else:
        if qlens is None or len(qlens) != n:
            raise ValueError("lchain_batch: rescue needs one query length per read")
        rs = rescue_par_t(1, rescue.get("max_dist", 5000), rescue.get("max_dist_inner", 1000), rescue.get("bw", 20000), rescue.get("max_skip", par.max_skip),
                          rescue.get("cap", 100000), rescue.get("min_cnt", par.min_cnt), rescue.get("min_sc", par.min_sc),
                          rescue.get("pen_gap", par.chn_pen_gap), rescue.get("pen_skip", par.chn_pen_skip),
                          rescue.get("rescue_size", 1000), rescue.get("rescue_ratio", 0.1), 0, 0)
        ql = np.ascontiguousarray(qlens, dtype=np.int32)
        flag = np.full(n, -1, dtype=np.int32)
        _check(L.mga_lchain_rescue_batch(n, flat.ctypes.data, off.ctypes.data, C.byref(par), C.byref(rs), ql.ctypes.data, C.byref(u), C.byref(uo),
                                         C.byref(b), C.byref(bo), flag.ctypes.data), "mga_lchain_rescue_batch")
    uoff = _take(uo, n + 1, np.int64)
    boff = _take(bo, n + 1, np.int64)
    uu = _take(u, int(uoff[-1]), np.uint64)
    bb = _take(b, int(boff[-1]), m128)
    if flag is not None:
        return [(uu[uoff[i]:uoff[i + 1]], bb[boff[i]:boff[i + 1]], int(flag[i])) for i in range(n)]
    return [(uu[uoff[i]:uoff[i + 1]], bb[boff[i]:boff[i + 1]]) for i in range(n)]


def rmq_fwd_batch(a, runs, order=None, max_dist=10000, max_dist_inner=1000, bw=2000, max_skip=25, cap=100000, pen_gap=0.8, pen_skip=0.05):
    """forward pass of the RMQ chainer (k_rmq.hip) over the runs (beg, end, base) of one chunk-level x-sorted anchor array, one wavefront per run, in one launch;
    order: run indices in launch order (None: the table's) -> (f, p, v, status): p counts from the run's base (-1: none), status 0 / 1 (tie) / 2 (inner window
    beyond the kernel's sort) per run, 4 for a run the kernel never took"""
    L = load()
    a = np.ascontiguousarray(a, dtype=m128)
    runs = np.ascontiguousarray(np.asarray(runs, dtype=np.int64).reshape(-1, 3))
    n, n_runs = len(a), len(runs)
    f, p, v = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    status = np.zeros(n_runs, dtype=np.int32)
    od = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    _check(L.mga_rmq_fwd_batch(n, a.ctypes.data, n_runs, runs.ctypes.data, n_runs if od is None else len(od), None if od is None else od.ctypes.data,
                               max_dist, max_dist_inner, bw, max_skip, cap, pen_gap, pen_skip, f.ctypes.data, p.ctypes.data, v.ctypes.data, status.ctypes.data),
           "mga_rmq_fwd_batch")
    return f, p, v, status


def gaf_div_batch(div):
    """dv:f: text of each float as the device's GAF writer prints it -> list of bytes"""
    L = load()
    div = np.ascontiguousarray(div, dtype=np.float32)
    out = np.zeros(len(div) * 8, dtype=np.uint8)
    L.mga_gaf_div_batch.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    _check(L.mga_gaf_div_batch(len(div), div.ctypes.data, out.ctypes.data), "mga_gaf_div_batch")
    return [bytes(out[8 * i:8 * i + 8]).rstrip(b"\0") for i in range(len(div))]


def sort128x_batch(arrays):
    """radix_sort_128x on the device, one wavefront per array (the chaining kernels' sort: LDS form up to 1024 elements) -> list of sorted copies"""
    L = load()
    n = len(arrays)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(a) for a in arrays])
    flat = np.ascontiguousarray(np.concatenate(arrays)) if n else np.zeros(0, dtype=m128)
    L.mga_sort128x_batch.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    _check(L.mga_sort128x_batch(n, flat.ctypes.data, off.ctypes.data), "mga_sort128x_batch")
    return [flat[off[i]:off[i + 1]] for i in range(n)]


def map_files(graph_path, read_paths, out_path, preset="lr", cigar=True, n_threads=8, verbose=1, idx_opt=None, map_opt=None, flags=0):
    """gfa_read + mg_map_files: the whole `minigraph -cx lr graph reads > out` job through the C ABI.
    idx_opt / map_opt: {field: value} written into mg_idxopt_t / mg_mapopt_t after the preset, the way main.c:131-191 applies
    command-line options; flags: MG_M_* bits OR-ed into mg_mapopt_t.flag."""
    L = load()
    io, mo, go = idxopt_t(), mapopt_t(), ggopt_t()
    L.mg_opt_set(None, C.byref(io), C.byref(mo), C.byref(go))
    if L.mg_opt_set(preset.encode(), C.byref(io), C.byref(mo), C.byref(go)) != 0:
        raise ValueError("unknown preset %r" % preset)
    if cigar:
        mo.flag |= MG_M_CIGAR
    mo.flag |= flags
    for k, v in (idx_opt or {}).items():
        setattr(io, k, v)
    for k, v in (map_opt or {}).items():
        setattr(mo, k, v)
    if L.mg_opt_check(C.byref(io), C.byref(mo), C.byref(go)) != 0:
        raise ValueError("mg_opt_check rejected the options")
    C.c_int.in_dll(L, "mg_verbose").value = verbose
    g = L.gfa_read(graph_path.encode())
    if not g:
        raise RuntimeError("gfa_read(%s) failed" % graph_path)
    fns = (C.c_char_p * len(read_paths))(*[p.encode() for p in read_paths])
    rc = L.mga_map_files_to_path(g, len(read_paths), fns, C.byref(io), C.byref(mo), n_threads, out_path.encode())
    L.gfa_destroy(g)
    if rc != 0:
        raise RuntimeError("mapping failed: %s" % L.mga_last_error().decode())


class MappedGaf:
    """GAF text of one mga_map_files_shard() call: a malloc'ed buffer owned by this object (zero-copy numpy view, bytes on request)"""

    def __init__(self, ptr, n, seg_len, t_map, cap=0):
        self.ptr, self.n, self.seg_len, self.t_map, self.cap = ptr, n, seg_len, t_map, cap

    def __len__(self):
        return self.n

    def view(self):
        return np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_uint8)), shape=(self.n,)) if self.n else np.zeros(0, dtype=np.uint8)

    def bytes(self):
        return C.string_at(self.ptr, self.n) if self.n else b""

    def free(self):
        if self.ptr is not None and self.ptr.value:
            load().mga_free(self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def map_files_idx(graph, read_paths, n_threads=8, rank=0, world=1, reuse=None, out_path=None):
    """the mapping phase of mg_map_files() against an existing index: FASTA/FASTQ files -> GAF text in memory (MappedGaf).
    world > 1: this process maps shard `rank` (see mga_map_files_shard in include/minigraph_amd.h); .seg_len lists its bytes per
    output segment, .t_map is the wall time of the phase (reader + pipeline + sink) measured inside the library.
    reuse: a MappedGaf of an earlier call whose buffer may be overwritten (it is consumed).
    out_path: the GAF goes to this FILE through the library's writer thread (the reference's step 2, gmap.c:119-139) instead of a buffer; returns the seconds of the phase."""
    L = load()
    fns = (C.c_char_p * len(read_paths))(*[p.encode() for p in read_paths])
    mem, n, cap, seg, nseg, t = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_void_p(), C.c_int(0), C.c_double(0.0)
    if out_path is not None:
        libc = C.CDLL(None)
        libc.fopen.restype, libc.fopen.argtypes, libc.fclose.argtypes = C.c_void_p, [C.c_char_p, C.c_char_p], [C.c_void_p]
        fp = libc.fopen(out_path.encode(), b"wb")
        if not fp:
            raise OSError("cannot open %s" % out_path)
        try:
            _check(L.mga_map_files_shard(graph.gi, len(read_paths), fns, C.byref(graph.mo), n_threads, rank, world, C.c_void_p(fp),
                                         None, None, None, C.byref(seg), C.byref(nseg), C.byref(t)), "mga_map_files_shard")
        finally:
            libc.fclose(fp)
        L.mga_free(seg)
        return t.value
    if reuse is not None and reuse.ptr is not None and reuse.ptr.value and reuse.cap > 0:
        mem, cap = reuse.ptr, C.c_int64(reuse.cap)
        reuse.ptr, reuse.n = None, 0
    _check(L.mga_map_files_shard(graph.gi, len(read_paths), fns, C.byref(graph.mo), n_threads, rank, world, None,
                                 C.byref(mem), C.byref(n), C.byref(cap), C.byref(seg), C.byref(nseg), C.byref(t)), "mga_map_files_shard")
    seg_len = _take(seg, nseg.value, np.int64)
    return MappedGaf(mem, n.value, seg_len, t.value, cap.value)


def reads_shard_dump(path, out_path, rank, world, batch_bases=500000000, n_threads=4):
    """the reads of shard rank/world as the sharded reader cuts them -> one-line FASTA in out_path; returns records per segment"""
    L = load()
    seg, nseg = C.c_void_p(), C.c_int(0)
    _check(L.mga_reads_shard_dump(path.encode(), batch_bases, n_threads, rank, world, out_path.encode(), C.byref(seg), C.byref(nseg)),
           "mga_reads_shard_dump")
    return _take(seg, nseg.value, np.int64)


class kstring_t(C.Structure):
    _fields_ = [("l", C.c_uint), ("m", C.c_uint), ("s", C.c_void_p)]


def map_batch_api(graph, names, seqs, n_threads=4, per_read=False):
    """The reference-shaped C API, as a caller of minigraph.h would use it: mg_map_batch() (or mg_map() read by read when
    per_read=True) -> mg_gchains_t objects -> mg_write_gaf() per read -> mg_gchain_free().  Returns the GAF bytes."""
    L = load()
    n = len(seqs)
    L.mg_map.restype = C.c_void_p
    L.mg_tbuf_init.restype = C.c_void_p
    L.mg_map.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_void_p, C.POINTER(mapopt_t), C.c_char_p]
    L.mg_map_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_void_p),
                               C.POINTER(mapopt_t), C.c_int]
    L.mg_write_gaf.argtypes = [C.POINTER(kstring_t), C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_char_p, C.c_uint64, C.c_void_p]
    L.mg_write_gaf.restype = None
    L.mg_gchain_free.argtypes = [C.c_void_p]
    L.mg_gchain_free.restype = None
    L.mg_tbuf_destroy.argtypes = [C.c_void_p]
    gcs = (C.c_void_p * n)()
    if per_read:
        tb = L.mg_tbuf_init()
        for i in range(n):
            gcs[i] = L.mg_map(graph.gi, len(seqs[i]), seqs[i], tb, C.byref(graph.mo), names[i])
        L.mg_tbuf_destroy(tb)
    else:
        qlens = (C.c_int * n)(*[len(s) for s in seqs])
        sp, npp = (C.c_char_p * n)(*seqs), (C.c_char_p * n)(*names)
        _check(L.mg_map_batch(graph.gi, n, qlens, sp, npp, gcs, C.byref(graph.mo), n_threads), "mg_map_batch")
    out, ks = [], kstring_t(0, 0, None)
    for i in range(n):
        ql = C.c_int32(len(seqs[i]))
        L.mg_write_gaf(C.byref(ks), graph.g, gcs[i], 1, C.byref(ql), names[i], graph.mo.flag, None)
        if ks.l:
            out.append(C.string_at(ks.s, ks.l))
        L.mg_gchain_free(gcs[i])
    L.mga_free(ks.s)
    return b"".join(out)


class Reads:
    """mga_reads_load(): a read set resident in host memory and HBM"""

    def __init__(self, path, max_reads=0):
        L = load()
        self.h = L.mga_reads_load(path.encode(), max_reads)
        if not self.h:
            raise RuntimeError("mga_reads_load failed: %s" % L.mga_last_error().decode())
        self.n, self.bases = L.mga_reads_count(self.h), L.mga_reads_bases(self.h)

    def close(self):
        if self.h:
            load().mga_reads_free(self.h)
        self.h = None


class GafBuffer:
    """the GAF text of one pass, owned by the index inside the C library: valid until the next map_reads() on the same
    Graph (no copy until bytes() is asked for)"""

    def __init__(self, ptr, n):
        self.ptr, self.n = ptr, n

    def __len__(self):
        return self.n

    def view(self):
        return np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_uint8)), shape=(self.n,)) if self.n else np.zeros(0, dtype=np.uint8)

    def bytes(self):
        return C.string_at(self.ptr, self.n)

    def free(self):
        self.ptr = None


def map_reads(graph, reads, n_threads=8, copy=True):
    """one pass of the hot path over a resident read set -> GAF bytes (or a GafBuffer when copy=False)"""
    L = load()
    buf, n = C.c_void_p(), C.c_int64(0)
    _check(L.mga_map_reads(graph.gi, reads.h, C.byref(graph.mo), n_threads, C.byref(buf), C.byref(n)), "mga_map_reads")
    gb = GafBuffer(buf, n.value)
    if not copy:
        return gb
    out = gb.bytes()
    gb.free()
    return out


class cov_chain_t(C.Structure):  # mga_cov_chain_t
    _fields_ = [("vert_beg", C.c_int64), ("vert_cnt", C.c_int32), ("ps", C.c_int32), ("pe", C.c_int32), ("plen", C.c_int32),
                ("mapq", C.c_int32), ("blen", C.c_int32)]


class cov_stats_t(C.Structure):  # mga_cov_stats_t
    _fields_ = [(n, C.c_int64) for n in ("chains_counted", "links_counted", "links_skipped")]


cov_chain_dtype = np.dtype([("vert_beg", "<i8"), ("vert_cnt", "<i4"), ("ps", "<i4"), ("pe", "<i4"), ("plen", "<i4"), ("mapq", "<i4"), ("blen", "<i4")])


def _cov_sizes(g):
    """(n_seg, n_arc) of a gfa_t* (gfa_t: m_seg, n_seg, max_rank, seg, h_names, m_sseq, n_sseq, sseq, h_snames, m_arc, n_arc, ...)"""
    u32 = C.cast(g, C.POINTER(C.c_uint32))
    u64 = C.cast(g, C.POINTER(C.c_uint64))
    return int(u32[1]), int(u64[8])


def _cov_stats(st):
    return {k: getattr(st, k) for k, _ in st._fields_}


def cov_finish(g, seg_bases, link_cnt):
    """mga_cov_finish: the doubles the reference hands to gfa_aux_update_cv, from the integer sums"""
    L = load()
    cs, cl = np.zeros(len(seg_bases), dtype=np.float64), np.zeros(len(link_cnt), dtype=np.float64)
    L.mga_cov_finish.argtypes = [C.c_void_p] * 5
    L.mga_cov_finish.restype = None
    L.mga_cov_finish(g, seg_bases.ctypes.data, link_cnt.ctypes.data, cs.ctypes.data, cl.ctypes.data)
    return cs, cl


def map_cov_ints(graph, read_paths, n_threads=8, rank=0, world=1, min_cov_mapq=None, min_cov_blen=None):
    """mga_map_files_cov: this rank's shard of the files -> (seg_bases, link_cnt, stats, t_map); the two int64 arrays of several ranks / calls simply add"""
    L = load()
    n_seg, n_arc = _cov_sizes(graph.g)
    mo = mapopt_t.from_buffer_copy(graph.mo)
    if min_cov_mapq is not None:
        mo.min_cov_mapq = min_cov_mapq
    if min_cov_blen is not None:
        mo.min_cov_blen = min_cov_blen
    fns = (C.c_char_p * len(read_paths))(*[p.encode() for p in read_paths])
    sb, lc = np.zeros(n_seg, dtype=np.int64), np.zeros(n_arc, dtype=np.int64)
    st, t = cov_stats_t(), C.c_double(0.0)
    L.mga_map_files_cov.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(mapopt_t), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.POINTER(cov_stats_t), C.POINTER(C.c_double)]
    _check(L.mga_map_files_cov(graph.gi, len(read_paths), fns, C.byref(mo), n_threads, rank, world, sb.ctypes.data, lc.ctypes.data, C.byref(st), C.byref(t)),
           "mga_map_files_cov")
    return sb, lc, _cov_stats(st), t.value


def map_cov(graph, read_paths, n_threads=8, min_cov_mapq=None, min_cov_blen=None):
    """read coverage of the files on the graph (`minigraph --cov`): (seg_bases, link_cnt, cov_seg, cov_link) -- covered bases per segment and traversals per
    arc as int64, and the doubles the reference tags the graph with (dc:f: stores them as float)"""
    sb, lc, _, _ = map_cov_ints(graph, read_paths, n_threads, 0, 1, min_cov_mapq, min_cov_blen)
    cs, cl = cov_finish(graph.g, sb, lc)
    return sb, lc, cs, cl


def _cov_flat(chains, vert):
    ch = np.ascontiguousarray(chains, dtype=cov_chain_dtype)
    v = np.ascontiguousarray(vert, dtype=np.uint32)
    return ch, v


def cov_chains_host(g, chains, vert, min_mapq, min_blen):
    """the host instantiation of cov_core.h over flat chain records (no GPU): (seg_bases, link_cnt, stats)"""
    L = load()
    ch, v = _cov_flat(chains, vert)
    n_seg, n_arc = _cov_sizes(g)
    sb, lc, st = np.zeros(n_seg, dtype=np.int64), np.zeros(n_arc, dtype=np.int64), cov_stats_t()
    L.mga_cov_chains_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(cov_stats_t)]
    L.mga_cov_chains_host.restype = None
    L.mga_cov_chains_host(g, len(ch), ch.ctypes.data, v.ctypes.data, min_mapq, min_blen, sb.ctypes.data, lc.ctypes.data, C.byref(st))
    return sb, lc, _cov_stats(st)


def cov_batch(graph, chains, vert, min_mapq, min_blen):
    """the same records through k_cov.hip against the graph's replica in HBM: (seg_bases, link_cnt, stats)"""
    L = load()
    ch, v = _cov_flat(chains, vert)
    n_seg, n_arc = _cov_sizes(graph.g)
    sb, lc, st = np.zeros(n_seg, dtype=np.int64), np.zeros(n_arc, dtype=np.int64), cov_stats_t()
    L.mga_cov_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(cov_stats_t)]
    _check(L.mga_cov_batch(graph.gi, len(ch), ch.ctypes.data, len(v), v.ctypes.data, min_mapq, min_blen, sb.ctypes.data, lc.ctypes.data, C.byref(st)), "mga_cov_batch")
    return sb, lc, _cov_stats(st)


bubble_dtype = np.dtype([("snid", "<i4"), ("ss", "<i4"), ("se", "<i4"), ("n_seg", "<i4"), ("v_off", "<i8")])   # mga_bubble_t
call_seg_dtype = np.dtype([("bid", "<i4"), ("is_stem", "u1"), ("is_src", "u1"), ("over", "u1"), ("pad", "u1")])   # mga_call_seg_t
call_pos_dtype = np.dtype([("v", "<u4"), ("yl1", "<i4"), ("yf1", "<i4"), ("span", "<i4")])   # mga_call_pos_t
call_chain_dtype = np.dtype([("pos_beg", "<i8"), ("cnt", "<i4"), ("lc_off", "<i4"), ("t", "<i4"), ("ord", "<i4")])   # mga_call_chain_t
call_intv_dtype = np.dtype([("st", "<i4"), ("en", "<i4")])   # mga_call_intv_t
call_cand_dtype = np.dtype([("key", "<u8"), ("bid", "<i4"), ("st", "<i4"), ("en", "<i4"), ("strand", "<i4"), ("qs", "<i4"), ("qe", "<i4"), ("glen", "<i4"), ("t", "<i4")])   # mga_call_cand_t
call_warn_dtype = np.dtype([("key", "<u8"), ("type", "<i4"), ("t", "<i4"), ("qs", "<i4"), ("qe", "<i4"), ("v", "<u4"), ("pad", "<i4")])   # mga_call_warn_t


def sort_ref_arc(g):
    """mga_sort_ref_arc on a gfa_t* (before the index is built)"""
    L = load()
    L.mga_sort_ref_arc.argtypes, L.mga_sort_ref_arc.restype = [C.c_void_p], None
    L.mga_sort_ref_arc(g)


def bubbles(g):
    """mga_bubbles on a gfa_t* (or a Graph) -> (records of bubble_dtype, uint32 vertex pool); bubble i lists pool[v_off : v_off + n_seg]"""
    L = load()
    g = getattr(g, "g", g)
    L.mga_bubbles.argtypes, L.mga_bubbles.restype = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_void_p)], C.c_void_p
    L.mga_bubbles_free.argtypes, L.mga_bubbles_free.restype = [C.c_void_p, C.c_void_p], None
    n, pool = C.c_int32(0), C.c_void_p()
    bb = L.mga_bubbles(g, C.byref(n), C.byref(pool))
    rec = np.empty(n.value, dtype=bubble_dtype)
    if n.value:
        C.memmove(rec.ctypes.data, bb, rec.nbytes)
    n_v = int((rec["v_off"] + rec["n_seg"]).max()) if n.value else 0
    v = np.empty(n_v, dtype=np.uint32)
    if n_v:
        C.memmove(v.ctypes.data, pool.value, v.nbytes)
    L.mga_bubbles_free(bb, pool)
    return rec, v


def _call_batch(fn, chains, pos, seg, seg_len, q_off, qintv, n_bb):
    L = load()
    ch, ps = np.ascontiguousarray(chains, dtype=call_chain_dtype), np.ascontiguousarray(pos, dtype=call_pos_dtype)
    sg, sl = np.ascontiguousarray(seg, dtype=call_seg_dtype), np.ascontiguousarray(seg_len, dtype=np.int32)
    qo, qi = np.ascontiguousarray(q_off, dtype=np.int64), np.ascontiguousarray(qintv, dtype=call_intv_dtype)
    assert len(sg) == len(sl) and len(qo) >= 1 and int(qo[-1]) <= len(qi)
    win = np.zeros(max(n_bb, 1), dtype=call_cand_dtype)
    warn, n_warn = C.c_void_p(), C.c_int64(0)
    f = getattr(L, fn)
    f.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                  C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    _check(f(len(ch), ch.ctypes.data, len(ps), ps.ctypes.data, len(sg), sg.ctypes.data, sl.ctypes.data, len(qo) - 1, qo.ctypes.data, qi.ctypes.data, n_bb, win.ctypes.data,
             C.byref(warn), C.byref(n_warn)), fn)
    return win[:n_bb], _take(warn, n_warn.value, call_warn_dtype)


def call_batch(chains, pos, seg, seg_len, q_off, qintv, n_bb):
    """the candidates of --call for flat records through k_call.hip -> (winner per bubble, key 0 = none; warnings in key order)"""
    return _call_batch("mga_call_batch", chains, pos, seg, seg_len, q_off, qintv, n_bb)


def call_chains_host(chains, pos, seg, seg_len, q_off, qintv, n_bb):
    """the same records through the host instantiation of call_core.h (no GPU)"""
    return _call_batch("mga_call_batch_host", chains, pos, seg, seg_len, q_off, qintv, n_bb)


def _call_asm(fn, handle, names, gcs, min_mapq, min_blen):
    L = load()
    n = len(names)
    f = getattr(L, fn)
    f.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.POINTER(kstring_t)]
    ks = kstring_t(0, 0, None)
    rc = f(handle, n, (C.c_char_p * n)(*names), (C.c_void_p * n)(*gcs), min_mapq, min_blen, C.byref(ks))
    out = C.string_at(ks.s, ks.l) if ks.l else b""
    L.mga_free(ks.s)
    _check(rc, fn)
    return out


def call_asm(graph, names, gcs, min_mapq=5, min_blen=100000):
    """mga_call_asm: the BED of `--call` from the mg_gchains_t* of every sequence of one file (input order), candidates on the device; graph: a Graph"""
    return _call_asm("mga_call_asm", graph.gi, names, gcs, min_mapq, min_blen)


def call_asm_host(g, names, gcs, min_mapq=5, min_blen=100000):
    """mga_call_asm_host: the same on the calling thread, no GPU; g: a gfa_t*"""
    return _call_asm("mga_call_asm_host", g, names, gcs, min_mapq, min_blen)


def call_times():
    """wall seconds of the phases of the last call_files() / call_asm*(): sort + index, read + map, bubbles, intervals + flatten, candidates, text"""
    t = (C.c_double * 6)()
    load().mga_call_times(t)
    return dict(zip(("index", "map", "bubbles", "flatten", "candidates", "text"), t))


def call_files(graph_path, query_path, preset="asm", cigar=True, n_threads=8, verbose=1, min_mapq=None, min_map_len=None):
    """gfa_read + mga_call_files: the whole `minigraph -cx asm --call graph query` job through the C ABI -> BED bytes"""
    import tempfile
    L = load()
    io, mo, go = idxopt_t(), mapopt_t(), ggopt_t()
    L.mg_opt_set(None, C.byref(io), C.byref(mo), C.byref(go))
    if L.mg_opt_set(preset.encode(), C.byref(io), C.byref(mo), C.byref(go)) != 0:
        raise ValueError("unknown preset %r" % preset)
    if cigar:
        mo.flag |= MG_M_CIGAR
    if min_mapq is not None:
        go.min_mapq = min_mapq
    if min_map_len is not None:
        go.min_map_len = min_map_len
    C.c_int.in_dll(L, "mg_verbose").value = verbose
    g = L.gfa_read(graph_path.encode())
    if not g:
        raise RuntimeError("gfa_read(%s) failed" % graph_path)
    libc = C.CDLL(None)
    libc.fopen.restype, libc.fopen.argtypes, libc.fclose.argtypes = C.c_void_p, [C.c_char_p, C.c_char_p], [C.c_void_p]
    L.mga_call_files.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(idxopt_t), C.POINTER(mapopt_t), C.POINTER(ggopt_t), C.c_int, C.c_void_p]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "call.bed")
        fp = libc.fopen(path.encode(), b"wb")
        if not fp:
            L.gfa_destroy(g)
            raise OSError("cannot open %s" % path)
        rc = L.mga_call_files(g, query_path.encode(), C.byref(io), C.byref(mo), C.byref(go), n_threads, C.c_void_p(fp))
        libc.fclose(C.c_void_p(fp))
        L.gfa_destroy(g)
        _check(rc, "mga_call_files")
        return open(path, "rb").read()


def get_stats(graph, reset=False):
    st = stats_t()
    load().mga_get_stats(graph.gi, C.byref(st), 1 if reset else 0)
    return {k: getattr(st, k) for k, _ in st._fields_}


def prof_enable(on=True):
    load().mga_prof_enable(1 if on else 0)


def prof_get(reset=False):
    ms = np.zeros(len(KERNELS), dtype=np.float64)
    cnt = np.zeros(len(KERNELS), dtype=np.int64)
    load().mga_prof_get(ms.ctypes.data, cnt.ctypes.data, 1 if reset else 0)
    return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(KERNELS)}
