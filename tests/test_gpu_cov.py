"""Read coverage (--cov) on the device: k_cov.hip against the host instantiation of cov_core.h on synthetic walks (exact equality of both integer arrays and the
three counters), and whole `--cov -cx lr` jobs through mg_map_files_fp + gfa_print, byte-identical to the reference binary."""
import ctypes as C
import os
import socket
import subprocess
import tempfile

import numpy as np
import pytest

import minigraph_amd as mga
import refbind as rb
import cov_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def chain_graph():
    """the tampered chain graph, indexed (its replica in HBM carries the tampered arcs)"""
    L = mga.load()
    d = tempfile.mkdtemp()
    path = os.path.join(d, "chain.gfa")
    cc.write_chain_gfa(path)
    G = mga.Graph.__new__(mga.Graph)
    G.io, G.mo, G.go = cc.options()
    G.g = L.gfa_read(path.encode())
    assert G.g
    cc.tamper(G.g)
    G.gi = L.mg_index(G.g, C.byref(G.io), 4, C.byref(G.mo))
    assert G.gi, L.mga_last_error()
    yield G
    G.close()


def both(G, cases, min_mapq=20, min_blen=1000):
    rec, vert = cases.arrays()
    want = mga.cov_chains_host(G.g, rec, vert, min_mapq, min_blen)
    got = mga.cov_batch(G, rec, vert, min_mapq, min_blen)
    assert np.array_equal(got[0], want[0]), np.nonzero(got[0] != want[0])[0][:10]
    assert np.array_equal(got[1], want[1]), np.nonzero(got[1] != want[1])[0][:10]
    assert got[2] == want[2], (got[2], want[2])
    return got


def test_stage_walk_lengths(chain_graph):
    """walks of 1, 2, 63, 64, 65 and 1 000 vertices (wavefront seams), forward and reverse"""
    K = cc.Cases()
    for n in (1, 2, 63, 64, 65, 1000):
        K.add(cc.fwd(20, n))
        K.add(cc.rev(20 + n - 1, n), ps=7, tail=11)
    sb, lc, st = both(chain_graph, K)
    assert st["chains_counted"] == 12 and st["links_skipped"] == 0 and st["links_counted"] == 2 * sum(n - 1 for n in (1, 2, 63, 64, 65, 1000))
    # one value by hand: segment 20 is the first segment of the six forward walks (60 - 3 bases; alone: 60 - 3 - 5) and the last of the six reverse ones (60 - 11; alone: 60 - 7 - 11)
    assert sb[20] == 5 * 57 + 52 + 5 * 49 + 42
    assert lc[cc.find_arc(chain_graph.g, 20 << 1, 21 << 1)] == 10 and lc[cc.find_arc(chain_graph.g, 21 << 1 | 1, 20 << 1 | 1)] == 10


def test_stage_contention_past_2_32(chain_graph):
    """70 000 chains all crossing one 100 000-base segment: one address under contention, a sum past 2^32"""
    K = cc.Cases()
    walk = cc.fwd(cc.BIG - 1, 3)
    for _ in range(70000):
        K.add(walk)
    sb, lc, st = both(chain_graph, K)
    assert sb[cc.BIG] == 70000 * cc.BIG_LEN and sb[cc.BIG] > 1 << 32
    assert st == {"chains_counted": 70000, "links_counted": 140000, "links_skipped": 0}


def test_stage_duplicate_and_missing_arcs(chain_graph):
    K = cc.Cases()
    K.add(cc.fwd(cc.DUP_AT, 2))        # two arcs s0+ -> s1+: skipped, the segments still count
    K.add(cc.fwd(cc.MISS_AT, 3))       # s10+ s11+: no reverse arc, skipped; s11+ s12+ counts
    K.add(cc.rev(cc.MISS_AT + 1, 2))   # s11- s10-: the forward arc is the missing one
    sb, lc, st = both(chain_graph, K)
    assert st == {"chains_counted": 3, "links_counted": 1, "links_skipped": 3}
    assert lc.sum() == 2 and sb[0] == 57 and sb[1] == 55


def test_stage_filters_and_empty(chain_graph):
    K = cc.Cases()
    K.add(cc.fwd(30, 4), mapq=19)              # fails the MAPQ bar only
    K.add(cc.fwd(30, 4), blen=999)             # fails the blen bar only
    K.add(cc.fwd(30, 4), mapq=20, blen=1000)   # passes both, exactly
    sb, lc, st = both(chain_graph, K)
    assert st["chains_counted"] == 1
    K2 = cc.Cases()
    K2.add(cc.fwd(30, 4), mapq=0)              # a secondary chain: counted when min_cov_mapq is 0
    assert both(chain_graph, K2, min_mapq=0)[2]["chains_counted"] == 1
    assert both(chain_graph, K2)[2]["chains_counted"] == 0
    sb, lc, st = both(chain_graph, cc.Cases())  # an empty chunk
    assert sb.sum() == 0 and lc.sum() == 0 and st["chains_counted"] == 0


def run_ref_cov(args, out):
    assert os.path.exists(rb.REF_BIN), "oracle/_ref/minigraph is missing: build() where the reference sources exist; oracle/_ref/ travels with the tree"
    with open(out, "wb") as fo:
        subprocess.check_call([rb.REF_BIN, "--cov"] + args, stdout=fo, stderr=subprocess.DEVNULL)
    return open(out, "rb").read()


def our_cov(graph, reads, d, cigar=True, **map_opt):
    """mg_map_files_fp with MG_M_CAL_COV, then the reference library's gfa_print of the tagged graph; also what the GAF stream received"""
    L = mga.load()
    ref = C.CDLL(rb.REF_SO)
    io, mo, go = cc.options(cigar=cigar, flags=cc.MG_M_CAL_COV | cc.MG_M_SKIP_GCHECK, **map_opt)
    g = L.gfa_read(graph.encode())
    assert g
    fns = (C.c_char_p * len(reads))(*[p.encode() for p in reads])
    gaf = os.path.join(d, "our.gaf")
    rc = L.mga_map_files_to_path(g, len(reads), fns, C.byref(io), C.byref(mo), 4, gaf.encode())
    assert rc == 0, L.mga_last_error()
    txt = cc.ref_print(ref, g, os.path.join(d, "our.gfa"))
    L.gfa_destroy(g)
    return txt, os.path.getsize(gaf)


JOBS = [("dev_gchain", {"MGA_DEV_GCHAIN": "1"}, True, [], {}),
        ("host_gchain", {"MGA_HOST_GCHAIN": "1"}, True, [], {}),
        ("no_cigar", {}, False, [], {}),
        ("min_cov_mapq_0", {}, True, ["--min-cov-mapq", "0"], {"min_cov_mapq": 0}),
        ("min_cov_blen_50", {}, True, ["--min-cov-blen", "50"], {"min_cov_blen": 50}),
        ("two_files", {}, True, [], {})]


@pytest.mark.parametrize("fixture", ["MT", "bubble"])
@pytest.mark.parametrize("name,env,cigar,ref_args,map_opt", JOBS, ids=[j[0] for j in JOBS])
def test_whole_job_vs_reference(fixture, name, env, cigar, ref_args, map_opt, monkeypatch):
    d = tempfile.mkdtemp()
    if fixture == "MT":
        graph, reads = cc.mt_fixture()
    else:
        graph, rd = cc.bubble_fixture(d)
        reads = [rd]
    if name == "two_files":
        reads = reads + reads
    want = run_ref_cov(ref_args + (["-c"] if cigar else []) + ["-x", "lr", "-t", "4", graph] + reads, os.path.join(d, "ref.gfa"))
    assert b"dc:f:" in want
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mga.prof_enable(True); mga.prof_get(reset=True)
    got, gaf_bytes = our_cov(graph, reads, d, cigar=cigar, **map_opt)
    pr = mga.prof_get(reset=True); mga.prof_enable(False)
    assert got == want, [(a, b) for a, b in zip(want.split(b"\n"), got.split(b"\n")) if a != b][:3]
    assert pr["k_cov"][1] > 0 and pr["k_gaf"][1] == 0 and pr["k_text"][1] == 0, (pr["k_cov"], pr["k_gaf"], pr["k_text"])
    assert gaf_bytes == 0


def test_stats_no_gaf_bytes():
    graph, reads = cc.mt_fixture()
    G = mga.Graph(graph, preset="lr", cigar=True, n_threads=4)
    mga.get_stats(G, reset=True)
    sb, lc, cs, cl = mga.map_cov(G, reads, n_threads=4)
    st = mga.get_stats(G, reset=True)
    G.close()
    assert st["n_reads"] == 2 and st["gaf_bytes"] == 0 and st["n_wfa"] == 0
    assert sb.sum() > 0 and np.array_equal(cl, lc.astype(np.float64))


def test_frag_mode_still_refused():
    L = mga.load()
    graph, reads = cc.mt_fixture()
    io, mo, go = cc.options(flags=cc.MG_M_CAL_COV | cc.MG_M_FRAG_MODE)
    g = L.gfa_read(graph.encode())
    fns = (C.c_char_p * len(reads))(*[p.encode() for p in reads])
    C.c_int.in_dll(L, "mg_verbose").value = 0
    rc = L.mga_map_files_to_path(g, len(reads), fns, C.byref(io), C.byref(mo), 4, os.path.join(tempfile.mkdtemp(), "x.gaf").encode())
    C.c_int.in_dll(L, "mg_verbose").value = 1
    L.gfa_destroy(g)
    assert rc == -1 and b"frag" in L.mga_last_error()


def _shard_worker(rank, world, port, graph, reads, q):
    import torch.distributed as dist
    from minigraph_amd.dist import cov_sharded
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    G = mga.Graph(graph, preset="lr", cigar=True, n_threads=2)
    sb, lc, cs, cl = cov_sharded(G, reads, n_threads=2)
    G.close()
    q.put((rank, sb, lc))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_gloo_world2():
    """two processes on one GPU, gloo: every rank ends with exactly the single-process integer arrays"""
    import torch.multiprocessing as mp
    d = tempfile.mkdtemp()
    graph, rd = cc.bubble_fixture(d)
    G = mga.Graph(graph, preset="lr", cigar=True, n_threads=4)
    sb1, lc1, _, _ = mga.map_cov(G, [rd], n_threads=4)
    G.close()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, graph, [rd], q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(60)
    assert sb1.sum() > 0
    for rank, sb, lc in res:
        assert np.array_equal(sb, sb1) and np.array_equal(lc, lc1), rank
