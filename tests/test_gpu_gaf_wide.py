"""The wide form of the GAF line kernel (k_gaf_wide.hip: a workgroup per line, the path column built by scans) through mga_gaf_lines_batch, byte for byte against a Python
restatement of the reference's mg_write_gaf (format.c:121-250); the wave form (k_gaf.hip) through the same entry is a second witness.  End to end: -cx asm with
MGA_DEV_GAF_WIDE=1 writes the bytes of the wave form and of the host writer."""
import faulthandler
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import minigraph_amd as mga
import call_cases as kc

VC, NC = 0x800, 0x200000   # MG_M_VERTEX_COOR, MG_M_NO_COMP_PATH
COUNTS = lambda T: (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1)
LENS, OFFS = (0, 1, 3, 15, 16, 17, 64, 65, 4099), (0, 1, 7, 15)
LONG = b"L" * 100


@pytest.fixture(autouse=True)
def time_limit():
    """every test here under its own limit (the dump names the test; the process exits)"""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def rgfa(tmp_path_factory):
    """a hand-made rGFA: chrA and chrB (rank 0, from 0; the same segment boundaries), chrG (rank 0, one base missing between neighbours), alt (rank 1, from 1000),
    ten segments without a stable sequence, one of them with a 100-byte name -> (Graph, segments (name, snid, soff, len), stable sequences (name, min, max, rank), first id of each group)"""
    T, rng = mga.gaf_wide_tile(), random.Random(7)
    n = 2 * T + 8
    seg, first, lines = [], {}, []
    for grp, sn, rank, cnt, step in ((b"a", b"chrA", 0, n, 0), (b"b", b"chrB", 0, n, 0), (b"g", b"chrG", 0, n, 1), (b"r", b"alt", 1, 8, 0), (b"n", None, 0, 10, 0)):
        first[grp], soff = len(seg), 1000 if grp == b"r" else 0
        for k in range(cnt):
            ln = 20 + k % 7
            seg.append((LONG if grp == b"n" and k == 9 else grp + b"%d" % k, (b"chrA", b"chrB", b"chrG", b"alt").index(sn) if sn else -1, soff if sn else -1, ln))
            lines.append(b"S\t%s\t%s" % (seg[-1][0], bytes(rng.choice(b"ACGT") for _ in range(ln))) + (b"\tSN:Z:%s\tSO:i:%d\tSR:i:%d" % (sn, soff, rank) if sn else b""))
            soff += ln + step
    lines += [b"L\ta%d\t+\ta%d\t+\t0M\tSR:i:0" % (k, k + 1) for k in range(n - 1)]
    sseq = [(nm, min(s[2] for s in seg if s[1] == i), max(s[2] + s[3] for s in seg if s[1] == i), 1 if nm == b"alt" else 0) for i, nm in enumerate((b"chrA", b"chrB", b"chrG", b"alt"))]
    path = str(tmp_path_factory.mktemp("gaf_wide") / "t.gfa")
    open(path, "wb").write(b"\n".join(lines) + b"\n")
    return mga.Graph(path, preset="lr", n_threads=4), seg, sseq, first


def ref_line(seg, sseq, qname, d, walk, mlen, blen, cg, ds, flag):
    """format.c:121-250 for one line"""
    if walk is None:
        return b"%s\t%d\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0\n" % (qname, d["qlen"])
    piece = lambda o: b"%s%s:%d-%d" % (b"<" if o[1] else b">", sseq[o[0]][0], o[2], o[3])
    path, last, compact = [], None, not flag & (VC | NC)
    for v in walk:
        name, snid, soff, ln = seg[v >> 1]
        if flag & VC or snid < 0:
            path += ([piece(last)] if last else []) + [(b"<" if v & 1 else b">") + name]
            last, compact = None, False
        elif last and last[0] == snid and last[1] == (v & 1) and (soff + ln == last[2] if v & 1 else soff == last[3]):
            last[2 + (1 - (v & 1))] = soff if v & 1 else soff + ln
        else:
            if last:
                path, compact = path + [piece(last)], False
            last = [snid, v & 1, soff, soff + ln]
    compact = bool(compact and last and sseq[last[0]][3] == 0 and sseq[last[0]][1] == 0)
    if last and not compact:
        path.append(piece(last))
    rev = walk[0] & 1
    if compact:
        t = seg[walk[-1 if rev else 0] >> 1]
        be = (d["plen"] - d["pe"], d["plen"] - d["ps"]) if rev else (d["ps"], d["pe"])
        col = b"%s\t%d\t%d\t%d" % (sseq[t[1]][0], sseq[t[1]][2], t[2] + be[0], t[2] + be[1])
    else:
        col = b"".join(path) + b"\t%d\t%d\t%d" % (d["plen"], d["ps"], d["pe"])
    div = float(np.float32(d["div"]))
    return (b"%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\ttp:A:%s\tNM:i:%d\tcm:i:%d\ts1:i:%d\ts2:i:%d" % (qname, d["qlen"], d["qs"], d["qe"], b"-" if compact and rev else b"+", col, mlen, blen,
            d["mapq"], b"P" if d["primary"] else b"S", blen - mlen, d["n_anchor"], d["score"], d["subsc"]) +
            (b"\tdv:f:" + (b"0" if div == 0 else b"%.4f" % div) if 0 <= div <= 1 else b"") + b"\tcg:Z:" + cg + b"\tds:Z:" + ds + b"\n")


def line_rec(i, chain):
    return dict(read=i, chain=chain, qlen=50000 + i, qs=3 + i, qe=49000 + i, plen=60000, ps=17, pe=59001 + i, mapq=60 - i % 7, n_anchor=99 + i, score=4000 - 11 * i, subsc=i % 3 * 77,
                primary=i % 4 != 3, div=(0.0, 0.00125, 0.04565, 2.0)[i % 4])


def make_walk(kind, n, T, F):
    """n oriented vertices; runs are stretches of chrA inside chrG vertices (which never merge: a base is missing between them)"""
    a, b, g, nn = F[b"a"], F[b"b"], F[b"g"], F[b"n"]
    run = lambda p, q: [(a + k if max(0, p) <= k <= q else g + k) << 1 for k in range(n)]
    return {"forward": lambda: [(a + k) << 1 for k in range(n)],
            "reverse": lambda: [(a + n - 1 - k) << 1 | 1 for k in range(n)],
            "tail_opens_tile": lambda: run(T - 3, T),
            "head_closes_tile": lambda: run(T - 1, T + 2),
            "three_tiles": lambda: run(T - 2, 2 * T),
            "alternating": lambda: [(a + k) << 1 | k & 1 for k in range(n)],
            "gap": lambda: [(g + k) << 1 for k in range(n)],
            "other_snid": lambda: [((b if k & 1 else a) + k) << 1 for k in range(n)],
            "no_snid": lambda: [(nn + k % 9 if k % 3 == 1 else a + k) << 1 | (k % 5 == 0) for k in range(n)],
            "rank1_first": lambda: [(F[b"r"] + k if k < 8 else a + k) << 1 for k in range(n)],
            "long_name": lambda: [(nn + 9 if k == n // 2 else a + k) << 1 for k in range(n)]}[kind]()


def run_and_check(rgfa, qnames, recs, walks, mb, strs, pool, flag):
    G, seg, sseq, _ = rgfa
    want = []
    for d in recs:
        c = d["chain"]
        o, nc, ns = strs[c] if c >= 0 else (0, 0, 0)
        want.append(ref_line(seg, sseq, qnames[d["read"]], d, walks[c] if c >= 0 else None, *(mb[c] if c >= 0 else (0, 0)), pool[o:o + nc], pool[o + nc:o + nc + ns], flag))
    got, off = mga.gaf_lines_batch(G, qnames, recs, walks, mb, strs, pool, flag=flag, form="wide")
    assert list(off) == [sum(len(w) for w in want[:i]) for i in range(len(want) + 1)]
    for i, w in enumerate(want):
        assert got[off[i]:off[i + 1]] == w, (i, len(walks[recs[i]["chain"]]) if recs[i]["chain"] >= 0 else None)
    wave, woff = mga.gaf_lines_batch(G, qnames, recs, walks, mb, strs, pool, flag=flag, form="wave")
    assert wave == got and list(woff) == list(off)


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [0, VC, NC])
@pytest.mark.parametrize("kind", ["forward", "reverse", "tail_opens_tile", "head_closes_tile", "three_tiles", "alternating", "gap", "other_snid", "no_snid", "rank1_first", "long_name"])
def test_path_column(rgfa, kind, flag):
    """a line per vertex count, one launch"""
    T = mga.gaf_wide_tile()
    walks = [make_walk(kind, n, T, rgfa[3]) for n in COUNTS(T)]
    pool = b"12M3I40M:12+acg:40"
    run_and_check(rgfa, [b"read%d" % i for i in range(len(walks))], [line_rec(i, i) for i in range(len(walks))], walks, [(52, 55)] * len(walks), [(0, 9, 9)] * len(walks), pool, flag)


@pytest.mark.gpu
def test_strings_and_placement(rgfa):
    """every string length with every source alignment, names that move the destination, an unmapped read's line in the middle: one launch"""
    T, F, rng = mga.gaf_wide_tile(), rgfa[3], random.Random(3)
    pool = bytes(rng.choice(b"0123456789MIDacgt:*+-") for _ in range(400000))
    strs, at = [], 0
    for i in range(36):   # 9 lengths x 4 alignments; the ds length runs against the cg length
        at += (OFFS[i % 4] - at) % 16
        strs.append((at, LENS[i % 9], LENS[(i // 4 + i) % 9]))
        at += strs[-1][1] + strs[-1][2] + 16
    walks = [make_walk(("forward", "no_snid", "gap")[i % 3], (1, 5, T + 1, 70)[i % 4], T, F) for i in range(36)]
    recs = [line_rec(i, i) for i in range(18)] + [dict(read=18, chain=-1, qlen=777)] + [line_rec(i + 1, i) for i in range(18, 36)]
    run_and_check(rgfa, [b"q" * (1 + i % 17) for i in range(37)], recs, walks, [(1000 + i, 1100 + 2 * i) for i in range(36)], strs, pool, 0)


CHILD = ("import sys; sys.path.insert(0, %r)\nimport minigraph_amd as mga\n"
         "mga.map_files(sys.argv[1], [sys.argv[2]], sys.argv[3], preset='asm', cigar=True, n_threads=8, verbose=0)\n"
         "print('STATS', *mga.gaf_wide_stats().values())\n") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_asm_gaf_same_bytes_with_the_wide_form(tmp_path):
    """-cx asm, 300 kb contigs.  Their chunks stay below the rule of 32768 plan items + operators per chain, so MGA_GAF_WIDE_MIN=0 sends them the way of chromosome-scale ones"""
    graph, reads = kc.mgsim_asm(str(tmp_path))
    res = {}
    for mode, env in (("wide", {"MGA_DEV_GAF_WIDE": "1", "MGA_GAF_WIDE_MIN": "0"}), ("wave", {}), ("host", {"MGA_DEV_GAF": "0"})):
        e = {k: v for k, v in os.environ.items() if k not in ("MGA_DEV_GAF_WIDE", "MGA_GAF_WIDE_MIN", "MGA_DEV_GAF")}
        p = subprocess.run([sys.executable, "-c", CHILD, graph, reads, str(tmp_path / mode)], env=dict(e, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        res[mode] = [int(x) for x in p.stdout.decode().split("STATS")[1].split()], open(str(tmp_path / mode), "rb").read()
    print("lines the wide form wrote / chunks handed back:", res["wide"][0])
    assert res["wide"][0][0] > 0 and res["wide"][0][1] == 0 and res["wave"][0] == [0, 0] and res["host"][0] == [0, 0]
    assert res["wide"][1] == res["wave"][1] == res["host"][1] and len(res["host"][1]) > 1000


@pytest.mark.parametrize("total,want", [(0, 0), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31, -1), (2 ** 31 + 5, -1), (2 ** 32, -1), (2 ** 32 + 7, -1), (2 ** 40, -1)])
def test_length_that_does_not_fit_is_a_status(total, want):
    """host side only: a 64-bit line length is stored whole or as -1, never clamped or wrapped; the launcher's status for such a line sends the chunk to the host writer"""
    assert mga.gaf_len32(total) == want
    assert [mga.gaf_wide_route(rc) for rc in (0, 1, -1)] == [0, 1, -1]
