#!/usr/bin/env python3
"""One measured case for the low-memory WFA rung (k_wfa_seg.hip): a gap whose plain traceback would pass the 32 GiB of the last HBM tier.

The pair: a random target of --len bases and a query that is the target at ~35 % divergence with indels, in which no 13 bases in a row stay unchanged --
so the two share no 13-mer along the alignment and mg_chain() finds no chain to cut the pair with.  To stay above the k-mer similarity of 0.02 under
which mwf_wfa_chain() writes D+I instead of aligning (miniwfa.c:795), every 400-base block of the query carries an exact 25-mer of the target, taken from
the MIRRORED block: 13 shared 13-mers per block, but any two of the copies are in opposite order on the two sequences, so the longest chain is a single
copy, whose co-diagonal run of 25 bases is below the anchor filter's 30 (miniwfa.c:755-774).  The plan of the chained fallback is then ONE stretch: the
whole pair.  That is checked on the CPU (mga_wfa_chain_plan) before anything runs on the GPU.

Default: mga.wfa_batch() once (exact pass -> 1e8-cell cap -> chained fallback -> ladder -> the 32 GiB tier gives up -> low-memory rung), compared with the
reference's mwf_wfa_auto().  --rung-only: the same pair through the rung alone (mga.wfa_seg_batch), without the single wavefront of the 32 GiB tier walking
the same cells first.  Prints the wall time of the rung, the chosen step, the snapshot count and wfa_seg_bytes.  Needs oracle/_ref/libmgref.so, or
--ref-cache with an earlier result of it for the same pair.

    python minigraph_amd/tools/wfa_seg_check.py [--len 150000] [--plan-only] [--rung-only] [--ref-cache FILE.npz]
"""
import argparse
import ctypes as C
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import minigraph_amd as mga  # noqa: E402


class wc_el_t(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sub", "op", "len", "x0", "y0", "tl", "ql")]


class wc_plan_t(C.Structure):
    _fields_ = [("n", C.c_int32), ("m", C.c_int32), ("n_sub", C.c_int32), ("score", C.c_int32), ("el", C.POINTER(wc_el_t))]


def build_pair(n, seed):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    t = rng.choice(acgt, size=n)
    q = bytearray()
    BLOCK, KEEP = 400, 25
    nb = n // BLOCK
    for j in range(nb + 1):
        blk = t[j * BLOCK:(j + 1) * BLOCK]
        u = rng.random(len(blk))
        run = 0
        for c, r in zip(blk.tolist(), u.tolist()):
            if run >= 12 and r >= 0.32:  # no 13 unchanged bases in a row
                r = 0.0
            if r < 0.24:  # substitution
                q.append(int(rng.choice(acgt[acgt != c])))
                run = 0
            elif r < 0.28:  # deletion
                run = 0
            elif r < 0.32:  # insertion
                q.append(c)
                q.append(int(rng.choice(acgt)))
                run = 0
            else:
                q.append(c)
                run += 1
        if j < nb and abs(2 * j - (nb - 1)) > 4:  # an exact 25-mer of the mirrored block (an insertion as far as the alignment goes); not where a block mirrors onto its neighbourhood
            m = (nb - 1 - j) * BLOCK + 100
            q += bytes(t[m:m + KEEP].tolist())
    return bytes(t.tolist()), bytes(q)


def plan_of(ts, qs):
    L = mga.load()
    par = (C.c_int32 * 8)()
    L.mga_wc_par_default(par)
    L.mga_wfa_chain_plan.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, C.c_void_p]
    L.mga_wfa_chain_plan_free.argtypes = [C.c_void_p]
    p = wc_plan_t()
    if L.mga_wfa_chain_plan(par, len(ts), ts, len(qs), qs, C.byref(p)) < 0:
        raise RuntimeError("mga_wfa_chain_plan failed")
    subs = [(p.el[i].tl, p.el[i].ql) for i in range(p.n) if p.el[i].sub]
    L.mga_wfa_chain_plan_free(C.byref(p))
    return subs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--len", type=int, default=150000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--plan-only", action="store_true", help="build the pair and check the plan on the CPU, run nothing on the GPU")
    ap.add_argument("--rung-only", action="store_true", help="run the pair through the low-memory rung alone (mga.wfa_seg_batch) instead of the whole ladder")
    ap.add_argument("--ref-only", action="store_true", help="compute the reference's result into --ref-cache on the CPU, run nothing on the GPU")
    ap.add_argument("--ref-cache", default=None, help="npz file with the reference's result for this pair: read when it matches the pair, written otherwise")
    a = ap.parse_args()
    ts, qs = build_pair(a.len, a.seed)
    subs = plan_of(ts, qs)
    step, nbytes = mga.wfa_seg_step(len(ts), len(qs)), mga.wfa_seg_bytes(len(ts), len(qs), 0)
    print("pair: %d x %d bases; plan: %d stretch(es), the longest %s; host step %d, wfa_seg_bytes %d (%.2f GiB)"
          % (len(ts), len(qs), len(subs), max(subs, key=min) if subs else None, step, nbytes, nbytes / 2.0**30))
    if subs != [(len(ts), len(qs))]:
        sys.exit("the plan does not leave the pair as one stretch: the D+I shortcut or kept anchors cut it")
    if a.plan_only:
        return
    key = hashlib.sha1(ts + b"|" + qs).hexdigest()
    want = None
    if a.ref_cache and os.path.exists(a.ref_cache):
        z = np.load(a.ref_cache)
        if str(z["key"]) == key:
            want = (int(z["score"]), z["cigar"], float(z["seconds"]))
    if want is None:
        import refbind as rb
        t0 = time.time()
        s, c = rb.Ref().wfa(ts, qs)
        want = (s, c, time.time() - t0)
        if a.ref_cache:
            np.savez(a.ref_cache, key=key, score=s, cigar=c, seconds=want[2])
    print("reference mwf_wfa_auto: score %d, %d operators, %.1f s on one host thread" % (want[0], len(want[1]), want[2]))
    if a.ref_only:
        return
    for k in ("MGA_WFA_LAST_TBCAP", "MGA_WFA_LAST_WMAX"):
        os.environ.pop(k, None)
    L = mga.load()
    L.mga_wfa_seg_seconds.restype = C.c_double
    L.mga_wfa_seg_last_step.restype = C.c_int32
    L.mga_wfa_seg_cells.restype = C.c_int64
    mga.wfa_seg_stats(reset=True)
    t0 = time.time()
    sc, cg = mga.wfa_seg_batch([ts], [qs]) if a.rung_only else mga.wfa_batch([ts], [qs])
    wall = time.time() - t0
    st = mga.wfa_seg_stats()
    print("device %s: score %d, %d operators, %.1f s in all; low-memory rung: %d problem(s), %.1f s, step %d, %d snapshots"
          % ("wfa_seg_batch" if a.rung_only else "wfa_batch", sc[0], len(cg[0]), wall, st["problems"], L.mga_wfa_seg_seconds(), L.mga_wfa_seg_last_step(), st["snapshots"]))
    cells = L.mga_wfa_seg_cells()
    print("traceback the rung's second pass wrote (one byte per cell of its narrowed band): %d = %.2f GiB" % (cells, cells / 2.0**30))
    if st["problems"] != 1:
        sys.exit("the stretch fitted the 32 GiB tier: the low-memory rung was not entered")
    if sc[0] != want[0] or not np.array_equal(cg[0], want[1]):
        sys.exit("MISMATCH with the reference")
    print("equal to the reference: score and CIGAR")


if __name__ == "__main__":
    main()
