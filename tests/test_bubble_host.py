"""The bubble finder of --call without a GPU: mga_sort_ref_arc + mga_bubbles (csrc/bubble.c) against gfa_sort_ref_arc + gfa_bubble of the reference library, each on the
graph its own gfa_read loaded from the same file -- the arc order after the sort arc by arc, then every bubble field by field (snid, ss, se, n_seg, every v[]).
Inputs: tests/golden/MT.gfa, mgsim bubble graphs with 3 and 5 haplotypes over several chromosomes (several stable sequences sharing one state buffer), and small
hand-written graphs, one per shape the traversal has to get right."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import minigraph_amd as mga
import refbind as rb
import call_cases as kc


def compare(path, min_bb=0):
    assert rb.have_ref(), "oracle/_ref/libmgref.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` where the reference sources exist"
    L, R = mga.load(), kc.ref_lib()
    g, rg = L.gfa_read(path.encode()), R.gfa_read(path.encode())
    assert g and rg
    mga.sort_ref_arc(g)
    R.gfa_sort_ref_arc(rg)
    ours, want = kc.arcs_of(g), kc.arcs_of(rg)
    assert ours == want, [k for k in range(min(len(ours), len(want))) if ours[k] != want[k]][:5]
    bb, v = mga.bubbles(g)
    ref = kc.ref_bubbles(R, rg)
    got = [(int(b["snid"]), int(b["ss"]), int(b["se"]), int(b["n_seg"]), [int(x) for x in v[b["v_off"]:b["v_off"] + b["n_seg"]]]) for b in bb]
    L.gfa_destroy(g)
    R.gfa_destroy(rg)
    assert len(got) == len(ref), (len(got), len(ref))
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a == b, (i, a, b)
    assert len(got) >= min_bb, len(got)
    return got


def test_mt_graph():
    compare(os.path.join(kc.GOLD, "MT.gfa"), 1)


@pytest.mark.parametrize("hap,chrom,seed", [(3, 3, 7), (5, 4, 13)])
def test_mgsim_graphs_several_chromosomes(hap, chrom, seed):
    d = tempfile.mkdtemp()
    subprocess.check_call([mga.MGSIM, "-p", os.path.join(d, "t"), "-G", "600000", "-c", str(chrom), "-H", str(hap), "-n", "1", "-l", "1000", "-s", str(seed)], stderr=subprocess.DEVNULL)
    got = compare(os.path.join(d, "t.gfa"), 20)
    assert len({b[0] for b in got}) == chrom   # bubbles on every stable sequence, found with one shared state buffer


@pytest.mark.parametrize("name", sorted(kc.HAND_GRAPHS))
def test_hand_written_graph(name):
    path = os.path.join(tempfile.mkdtemp(), name + ".gfa")
    want_bb, want_multi = kc.write_hand_graph(name, path)
    got = compare(path)
    assert len(got) == want_bb, (name, got)
    if name == "inversion":
        assert any(len({x >> 1 for x in b[4]}) < len(b[4]) for b in got)   # a bubble that lists both orientations of a segment
    listed = {}
    for i, b in enumerate(got):
        for x in b[4]:
            listed.setdefault(x >> 1, set()).add(i)
    assert any(len(s) > 1 for s in listed.values()) == want_multi, listed
