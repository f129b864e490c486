"""--call end to end on the GPU: mga.call_files (sort the reference arcs, index, map under -x asm through mg_map_batch, bubbles, k_call, BED) against the bytes of the
reference binary's `-cx asm --call` and of the drop-in binary; the same contigs as two shards through pack -> assemble -> mga_call_asm; and, on the CPU, the loud failure of
mga_call_asm without a device."""
import ctypes as C
import faulthandler
import functools
import os
import subprocess
import sys
import tempfile

import pytest

import minigraph_amd as mga
import refbind as rb
import call_cases as kc
from test_cov_host import read_fasta

DROPIN = os.path.join(os.path.dirname(rb.REF_BIN), "minigraph_dropin")


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def need_ref():
    assert rb.have_ref() and os.path.exists(rb.REF_BIN), "oracle/_ref is missing: run `python -c 'import __graft_entry__ as g; g.build()'` where the reference sources exist"


@functools.lru_cache(maxsize=None)
def mgsim_case():
    """(graph, contigs, the reference binary's BED), made once; the BED carries >= 50 walks and a '.' line"""
    need_ref()
    d = tempfile.mkdtemp()
    graph, reads = kc.mgsim_asm(d)
    want = kc.ref_call(graph, reads, os.path.join(d, "want.bed"))
    assert kc.bed_is_ground(want)
    return graph, reads, want


@pytest.mark.gpu
@pytest.mark.parametrize("query", ["MT-orangA.fa", "MT-chimp.fa"])
def test_call_files_mt_equals_reference_binary(query):
    need_ref()
    graph, q = os.path.join(kc.GOLD, "MT.gfa"), os.path.join(kc.GOLD, query)
    want = kc.ref_call(graph, q, os.path.join(tempfile.mkdtemp(), "want.bed"), True, ["-l", "5000"])   # (the preset's -l 100k indexes nothing of 16.5 kb)
    assert want.count(b"\n") > 0
    assert mga.call_files(graph, q, n_threads=4, min_map_len=5000) == want


@pytest.mark.gpu
def test_call_files_mgsim_equals_reference_and_dropin():
    graph, reads, want = mgsim_case()
    got = mga.call_files(graph, reads, n_threads=8)
    assert got == want
    t = mga.call_times()
    assert t["candidates"] > 0 and t["map"] > 0
    if os.path.exists(DROPIN):
        out = os.path.join(tempfile.mkdtemp(), "dropin.bed")
        with open(out, "wb") as fo:
            subprocess.check_call([DROPIN, "-cx", "asm", "--call", "-t", "8", graph, reads], stdout=fo, stderr=subprocess.DEVNULL, timeout=280)
        assert open(out, "rb").read() == got


@pytest.mark.gpu
def test_two_shards_packed_assembled_and_called():
    """the native end of the sharded route: each of two "ranks" maps its shard (mga_ggen_map_shard), rank 0 assembles the packed parts (mga_ggen_assemble) and calls"""
    from minigraph_amd.dist import call_from_parts
    graph, reads, want = mgsim_case()
    L = mga.load()
    g = L.gfa_read(graph.encode())
    mga.sort_ref_arc(g)                       # before the index, as main.c:280
    G = mga.Graph.__new__(mga.Graph)
    G.io, G.mo, G.go = mga.idxopt_t(), mga.mapopt_t(), mga.ggopt_t()
    L.mg_opt_set(None, C.byref(G.io), C.byref(G.mo), C.byref(G.go))
    L.mg_opt_set(b"asm", C.byref(G.io), C.byref(G.mo), C.byref(G.go))
    G.mo.flag |= mga.MG_M_CIGAR
    G.g, G.gi = g, L.mg_index(g, C.byref(G.io), 8, C.byref(G.mo))
    assert G.gi
    recs = read_fasta(reads)
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    n = len(names)
    L.mga_ggen_map_shard.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    qlens, sp, npp = (C.c_int * n)(*[len(x) for x in seqs]), (C.c_char_p * n)(*seqs), (C.c_char_p * n)(*names)
    parts = []
    for rank in range(2):
        buf, nb = C.c_void_p(), C.c_int64(0)
        assert L.mga_ggen_map_shard(G.gi, n, qlens, sp, npp, C.byref(G.mo), 8, rank, 2, C.byref(buf), C.byref(nb)) == 0, L.mga_last_error()
        parts.append(C.string_at(buf, nb.value))
        L.mga_free(buf)
    assert all(len(p) > 0 for p in parts)
    got = call_from_parts(G, parts, names)
    G.close()
    assert got == want


def test_call_asm_without_a_gpu_fails_with_the_librarys_error():
    """mga_call_asm is a compute entry: with no device visible it fails loudly, it does not run the host routine instead (a child process: the device list is read once)"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import minigraph_amd as mga\n"
            "L = mga.load()\n"
            "assert L.mga_device_count() == 0\n"
            "import ctypes as C\n"
            "g = L.gfa_read(sys.argv[1].encode())\n"
            "idx = (C.c_void_p * 6)(g)\n"   # an mg_idx_t whose first field is the graph: all the entry may read before it asks for a device
            "class G: gi = C.cast(idx, C.c_void_p)\n"
            "try:\n"
            "    mga.call_asm(G, [], [])\n"
            "except RuntimeError as e:\n"
            "    print('REFUSED', e)\n") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, os.path.join(kc.GOLD, "MT.gfa")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert "REFUSED" in p.stdout.decode() and "mga_call_asm failed" in p.stdout.decode(), p.stdout.decode()
