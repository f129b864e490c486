"""-cx asm end to end with the contigs' bridges on the device (MGA_ASM_DEV_BRIDGE=1: gc_read_p1 per contig, one wide-form mga_gwfa_bridge_batch call, gc_read_p3): the GAF
bytes of the default route and of the reference binary, and the counter shows bridges the wide form served."""
import os
import subprocess
import sys
import tempfile

import pytest

import minigraph_amd as mga
import refbind as rb
import call_cases as kc

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = ("import sys; sys.path.insert(0, %r)\nimport minigraph_amd as mga\n"
         "mga.map_files(sys.argv[1], [sys.argv[2]], sys.argv[3], preset='asm', cigar=True, n_threads=8, verbose=0)\n"
         "print('STATS', *mga.asm_bridge_stats().values())\n") % os.path.dirname(HERE)


def run(graph, reads, out, mode):   # a child process: the switch is read once
    env = {k: v for k, v in os.environ.items() if k != "MGA_ASM_DEV_BRIDGE"}
    if mode:
        env["MGA_ASM_DEV_BRIDGE"] = mode
    p = subprocess.run([sys.executable, "-c", CHILD, graph, reads, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    st = [l for l in p.stdout.decode().splitlines() if l.startswith("STATS")][0].split()[1:]
    return [int(x) for x in st], open(out, "rb").read()


@pytest.mark.gpu
def test_asm_gaf_same_bytes_with_bridges_on_the_device():
    assert rb.have_ref() and os.path.exists(rb.REF_BIN), "oracle/_ref is missing"
    d = tempfile.mkdtemp()
    graph, reads = kc.mgsim_asm(d)
    want = subprocess.run([rb.REF_BIN, "-cx", "asm", "-t", "8", graph, reads], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True, timeout=280).stdout
    st0, gaf0 = run(graph, reads, os.path.join(d, "a.gaf"), None)
    st1, gaf1 = run(graph, reads, os.path.join(d, "b.gaf"), "1")
    print("bridges wide / handed back / host:", st1)
    assert st0 == [0, 0, 0] and gaf0 == want
    assert st1[0] >= 1
    assert gaf1 == want and len(want) > 1000
