"""-x asm with the contigs' bridges taken out of the graph chaining (MGA_ASM_DEV_BRIDGE), on the CPU: gc_read_p1 per contig, the gathered mga_gwfa_prob_t records answered by
the host routine mga_gwfa_bridge (=2), gc_read_p3 per contig -- the bytes of the unsplit host routine and of the reference binary."""
import os
import subprocess
import sys
import tempfile

import pytest

import minigraph_amd as mga
import refbind as rb

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.skipif(not (rb.have_oracle() and os.path.exists(mga.LIB_PATH) and os.path.exists(rb.REF_BIN)), reason="libraries not built")

CHILD = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport hostpipe as hp, minigraph_amd as mga\n"
         "g, r = sys.argv[1], sys.argv[2]\nwant, occ, lco = hp.run_reference(g, r, cigar=False, preset='asm')\n"
         "got, _ = hp.map_with_oracle_stages(g, r, occ, lco, cigar=False, preset='asm', n_threads=int(sys.argv[3]))\n"
         "sys.stdout.buffer.write(b'%%d %%d\\n' %% (int(got == want), sum(mga.asm_bridge_stats().values())) + got)\n") % (os.path.dirname(HERE), HERE)


def run(graph, reads, mode, threads):   # a child process: the switch is read once
    env = {k: v for k, v in os.environ.items() if k != "MGA_ASM_DEV_BRIDGE"}
    if mode:
        env["MGA_ASM_DEV_BRIDGE"] = mode
    p = subprocess.run([sys.executable, "-c", CHILD, graph, reads, str(threads)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    head, gaf = p.stdout.split(b"\n", 1)
    return [int(x) for x in head.split()], gaf


@pytest.mark.parametrize("div, threads", [("0.004", 3), ("0.03", 1)])
def test_split_route_equals_unsplit_routine_and_reference(div, threads):
    d = tempfile.mkdtemp()
    subprocess.check_call([mga.MGSIM, "-p", os.path.join(d, "t"), "-G", "1500000", "-H", "3", "-n", "4", "-l", "300000", "-e", div, "-s", "9"], stderr=subprocess.DEVNULL)
    graph, reads = os.path.join(d, "t.gfa"), os.path.join(d, "t.reads.fa")
    (same0, n0), whole = run(graph, reads, None, threads)
    (same2, n2), split = run(graph, reads, "2", threads)
    assert same0 == 1 and n0 == 0          # unset: the unsplit routine, the reference's bytes, no bridge counted
    assert n2 > 0                          # the contigs did list bridges, and every one went through a record
    assert split == whole and same2 == 1 and len(split) > 500
