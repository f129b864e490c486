"""The per-vertex lines of -S / --write-mz on the device (k_gaf_vert.hip): hand-made chains through mga_gaf_vert_batch against the host writer (gaf.c), byte for byte, and whole
jobs against the reference binary in both placements of graph chaining.

The hand-back case: a CPU search over every (n_mz < 4096, cnt < 4096, span < 256) found no div whose fourth decimal lies within 1e-12 of a rounding boundary; the closest
triple is 2.3e-10 away, inside the kernel's guard of 1e-9, and is the one used here."""
import math
import os
import subprocess
import sys
import tempfile

import pytest

import minigraph_amd as mga
import test_gpu_e2e as e2e

LCHAIN, MZ, VC, SECOND, UNMAP = 0x800000, 0x1000000, 0x800, 0x2000, 0x100000
LONG = b"N" * 100   # a name longer than a wavefront


@pytest.fixture(scope="module")
def graph(tmp_path_factory):
    """70 segments in a row on one stable sequence (their names, not its name, must be printed) and one with a 100-byte name"""
    lines = [b"S\ts%d\t%s\tSN:Z:chrA\tSO:i:%d\tSR:i:0" % (k, b"ACGTTGCA" * 3, 24 * k) for k in range(70)] + [b"S\t%s\t%s" % (LONG, b"ACGT" * 5)]
    path = str(tmp_path_factory.mktemp("gaf_vert") / "t.gfa")
    open(path, "wb").write(b"\n".join(lines) + b"\n")
    return mga.Graph(path, preset="lr", n_threads=4)


class Chains:
    """records and anchors of hand-made walks; every (n_mz, cnt, span) is checked to lie far from a rounding boundary of "%.4f" """

    def __init__(self):
        self.lc, self.a = [], []

    def vertex(self, v, cnt, n_mz=None, span=15, dx=(), dy=(), near=False):
        n_mz = cnt if n_mz is None else n_mz
        if cnt > 0 and n_mz != cnt:
            s = math.log(max(n_mz, cnt) / min(n_mz, cnt)) / span * 10000.0
            gap = abs(abs(s - round(s)) - 0.5)
            assert gap < 5e-10 if near else gap > 1e-6, (n_mz, cnt, span, gap)
        x, y = 5000, 700
        self.lc.append((len(self.a), cnt, v))
        for k in range(cnt):
            if k:
                x, y = x + (dx[(k - 1) % len(dx)] if dx else 7 + k % 5), y + (dy[(k - 1) % len(dy)] if dy else 6 + k % 3)
            mz = 40 + (n_mz - 1 if k == cnt - 1 else min(k, max(n_mz - 2, 0)))
            self.a.append((mz << 32 | x, span << 32 | y))

    def walk(self, vertices):
        beg = len(self.lc)
        for args in vertices:
            self.vertex(*args[:2], **(args[2] if len(args) > 2 else {}))
        return beg, len(self.lc) - beg


def chain(i, parent, walk):
    return dict(id=i, parent=parent, lc_off=walk[0], cnt=walk[1], n_anchor=50 + i, score=900 - i, subsc=i * 31, qs=5, qe=9000 + i, plen=12000, ps=3, pe=11000 + i, mapq=60 - i,
                mlen=8000, blen=8100 + i, div=(0.0, 0.0123)[i % 2], txt_off=0, cg_len=9, ds_len=9)


@pytest.fixture(scope="module")
def case():
    C = Chains()
    widths = dict(dx=(0, 10, 9999, 10000, -40, 1), dy=(0, 3, 12))   # a distance of 0, a width change, a negative target distance
    edges = C.walk([(0, 0), (3, 1, dict(n_mz=4)), (4, 2, dict(n_mz=9)), (7, 64, dict(n_mz=64, **widths)), (8, 65, dict(n_mz=300, **widths)), (140, 129, dict(n_mz=97)),
                    (11, 2050, dict(n_mz=3000, span=19, **widths))])   # cnt at the lane and trip boundaries, a reverse-strand vertex, more anchors than the LDS stage of y holds
    reads = [[chain(0, 0, edges)],
             [chain(0, 0, C.walk([(2, 3, dict(n_mz=2))]))],                                   # one vertex; n_mz < cnt
             [chain(0, 0, C.walk([(2 * k + (k % 7 == 0), 2, dict(n_mz=2 + k)) for k in range(64)]))],
             [],                                                                              # an unmapped read between mapped ones
             [chain(0, 0, C.walk([(2 * k, k % 4, dict(n_mz=k % 4 + k % 3)) for k in range(65)])),   # 65 vertices: a second trip of one lane
              chain(1, 0, C.walk([(12, 5, dict(n_mz=11)), (15, 0)]))]]                        # a secondary chain
    return C, reads


@pytest.mark.gpu
@pytest.mark.parametrize("second", [0, SECOND])
@pytest.mark.parametrize("flag", [LCHAIN, LCHAIN | MZ, LCHAIN | VC, LCHAIN | MZ | VC])
def test_stage_equals_host_writer(graph, case, flag, second):
    C, reads = case
    flag |= second | UNMAP
    args = (graph, [b"read%d" % i for i in range(len(reads))], [10000 + i for i in range(len(reads))], reads, C.lc, C.a, b"12M3I40M:12+acg:40", flag)
    want = mga.gaf_vert_batch(*args, route="host")
    mga.gaf_vert_stats(reset=True)
    got = mga.gaf_vert_batch(*args, route="device")
    stars = [l for l in want.split(b"\n") if l.startswith(b"*\t")]
    assert len(stars) == sum(c["cnt"] for r in reads for c in r if second or c["id"] == c["parent"]) and want.count(b"\ttp:A:S") == (1 if second else 0)
    assert b"read3\t10003\t0\t0\t*\t*" in want and any(l.endswith(b"\t\t") for l in stars) == (b",-40," in want) == bool(flag & MZ)   # the inputs are what they claim to be
    for i, (w, g) in enumerate(zip(want.split(b"\n"), got.split(b"\n"))):
        assert w == g, (i, w[:200], g[:200])
    assert got == want
    assert mga.gaf_vert_stats() == (len(stars), 0, 0)


@pytest.mark.gpu
def test_div_next_to_a_rounding_boundary_goes_to_the_host_writer(graph):
    """n_mz = 3497, cnt = 342, span = 33: div * 10^4 = 704.50000000023, the triple closest to a boundary below cnt = 4096 and inside the kernel's guard of 1e-9"""
    C = Chains()
    reads = [[chain(0, 0, C.walk([(4, 2, dict(n_mz=7)), (6, 342, dict(n_mz=3497, span=33, near=True))]))]]
    args = (graph, [b"r"], [9999], reads, C.lc, C.a, b"12M3I40M:12+acg:40", LCHAIN | MZ)
    mga.gaf_vert_stats(reset=True)
    got = mga.gaf_vert_batch(*args, route="device")
    assert mga.gaf_vert_stats() == (0, 1, 0)
    assert got == mga.gaf_vert_batch(*args, route="host") and b"\t342\t0.0705\t" in got


CHILD = ("import sys; sys.path.insert(0, %r)\nimport minigraph_amd as mga\n"
         "mga.map_files(sys.argv[1], [sys.argv[2]], sys.argv[3], preset='lr', cigar=sys.argv[4] == 'c', n_threads=16, verbose=0, flags=int(sys.argv[5]))\n"
         "print('STATS', *mga.gaf_vert_stats())\n") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bubbles():
    d = tempfile.mkdtemp()
    subprocess.check_call([mga.MGSIM, "-p", os.path.join(d, "t"), "-G", "1500000", "-H", "3", "-n", "150", "-s", "7"], stderr=subprocess.DEVNULL)
    return d, os.path.join(d, "t.gfa"), os.path.join(d, "t.reads.fa")


@pytest.mark.gpu
@pytest.mark.parametrize("pct", ["100", "0"])
@pytest.mark.parametrize("tag,cli,cigar,flags", [("cS", ["-c", "-S"], "c", LCHAIN), ("cSmz", ["-c", "--write-mz", "-S"], "c", LCHAIN | MZ), ("S", ["-S"], "n", LCHAIN)])
def test_jobs_equal_the_reference_in_both_placements(bubbles, tag, cli, cigar, flags, pct):
    """the bubble graph of test_gpu_e2e's option sets: the same bytes as the reference binary, and every '*' line written on the device, with the llchains and anchors read in
    place (graph chaining on the device, MGA_DEV_GCHAIN_PCT=100) and uploaded (=0).  Without -c the host formats each chain's line and copies the device's vertex lines behind it."""
    d, graph, reads = bubbles
    ref, got = os.path.join(d, "ref.%s" % tag), os.path.join(d, "got.%s.%s" % (tag, pct))
    if not os.path.exists(ref):
        e2e.run_ref(["-x", "lr", "-t", "4"] + cli + [graph, reads], ref)
    env = {k: v for k, v in os.environ.items() if k not in ("MGA_DEV_GCHAIN", "MGA_DEV_GCHAIN_PCT", "MGA_DEV_GAF_VERT", "MGA_HOST_GCHAIN")}
    p = subprocess.run([sys.executable, "-c", CHILD, graph, reads, got, cigar, str(flags)], env=dict(env, MGA_DEV_GCHAIN_PCT=pct), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    if open(ref, "rb").read() != open(got, "rb").read():
        raise AssertionError(e2e.first_diff(ref, got))
    stats = [int(x) for x in p.stdout.decode().split("STATS")[1].split()]
    n_star = sum(l.startswith(b"*\t") for l in open(got, "rb").read().split(b"\n"))
    print("vertex lines in the output / written on the device, hand-backs:", n_star, stats)
    assert n_star > 100 and stats == [n_star, 0, 0]
