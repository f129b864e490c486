"""The low-memory WFA rung on the device (k_wfa_seg.hip): mwf_wfa_exact's checkpointed mode for the stretches of the chained fallback that outgrow the last HBM tier.
Stage parity against the oracle's exact WFA for every step, the route through the scheduler (the last tier's capacity lowered by MGA_WFA_LAST_TBCAP so that small
inputs take it), and one end-to-end mapping against the reference binary's bytes."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import minigraph_amd as mga
import refbind as rb
import wfa_seg_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ora():
    return rb.Oracle()


@pytest.fixture(scope="module")
def base(ora):
    """the shared pairs and their expected values, computed once"""
    T, Q = wc.base_pairs()
    return T, Q, [ora.wfa(t, q, max_iter=-1) for t, q in zip(T, Q)]


@pytest.mark.parametrize("step", wc.STEPS)
def test_wfa_seg_stage_parity(ora, base, step):
    T, Q, want = base
    T, Q, want = list(T), list(Q), list(want)
    for t, q, target in wc.checkpoint_pairs(step):  # termination at a checkpoint and one score before it
        es, ec = ora.wfa(t, q, max_iter=-1)
        assert es == target and (es + 1) % step in (0, 1 % step), (step, es)
        T.append(t)
        Q.append(q)
        want.append((es, ec))
    assert max(w[0] for w in want) > 512 and min(w[0] for w in want) == 0
    mga.wfa_seg_stats(reset=True)
    sc, cg = mga.wfa_seg_batch(T, Q, step)
    for i in range(len(T)):
        assert want[i][0] == sc[i], (step, i, len(T[i]), len(Q[i]))
        assert np.array_equal(want[i][1], cg[i]), (step, i, len(T[i]), len(Q[i]))
    st = mga.wfa_seg_stats()
    assert st["problems"] == len(T)
    assert st["snapshots"] == sum(w[0] // step for w in want)  # one before every slice whose score is a multiple of the step


def test_wfa_seg_host_chosen_step(ora, base):
    T, Q, want = base
    sc, cg = mga.wfa_seg_batch(T, Q)
    for i in range(len(T)):
        assert want[i][0] == sc[i] and np.array_equal(want[i][1], cg[i]), i


def test_wfa_ladder_routes_past_the_last_tier(monkeypatch):
    """the three large cases of the chained-fallback stage test (9-12 kb at 30-75 % divergence between exact flanks): with the last HBM tier cut to 16 MiB of traceback their
    long stretches fall off the ladder and are closed by the low-memory rung -- same score and CIGAR as mwf_wfa_auto(); with the tier as it is, the rung is never entered"""
    ref = rb.Ref()
    rng = np.random.default_rng(7)
    T, Q = [], []
    for n, sub, indel in [(9000, 0.3, 0.1), (12000, 0.3, 0.1), (9500, 0.75, 0.0)]:
        a, m, b = wc.rand_seq(rng, 500), wc.rand_seq(rng, n), wc.rand_seq(rng, 500)
        T.append(a + m + b)
        Q.append(a + wc.mutate_scalar(rng, m, sub, indel) + b)
    T.append(T[0][:300])  # and a gap that never leaves the first rungs
    Q.append(Q[0][5:290])
    want = [ref.wfa(t, q) for t, q in zip(T, Q)]
    monkeypatch.setenv("MGA_WFA_LAST_TBCAP", str(1 << 24))
    mga.wfa_seg_stats(reset=True)
    sc, cg = mga.wfa_batch(T, Q)
    for i in range(len(T)):
        assert want[i][0] == sc[i], i
        assert np.array_equal(want[i][1], cg[i]), i
    assert mga.wfa_seg_stats(reset=True)["problems"] > 0
    monkeypatch.delenv("MGA_WFA_LAST_TBCAP")
    sc2, cg2 = mga.wfa_batch(T, Q)
    assert mga.wfa_seg_stats()["problems"] == 0
    for i in range(len(T)):
        assert sc2[i] == sc[i] and np.array_equal(cg2[i], cg[i]), i


def test_reads_with_a_gap_beyond_the_last_tier_vs_reference_binary(monkeypatch):
    """the read set of the fallback end-to-end test (middle 9-12 kb at 30-40 % divergence), mapped with the last HBM tier cut down: the stretches of the chained
    fallback go through the low-memory rung, and the GAF still equals the reference binary's bytes.  The existing test has no golden file to fall back on
    (it requires the reference binary, and so do all end-to-end tests here: a suite that skips its parity checks is not green), so this one requires it too"""
    assert os.path.exists(rb.REF_BIN), "oracle/_ref/minigraph is missing: build it where the reference tree exists; oracle/_ref/ travels with the tree"
    rng = np.random.default_rng(11)

    def rnd(n):
        return bytes(rng.choice(list(b"ACGT"), n).tolist())

    d = tempfile.mkdtemp()
    ref = rnd(60000)
    graph, reads = os.path.join(d, "g.fa"), os.path.join(d, "r.fa")
    open(graph, "wb").write(b">chr\n" + ref + b"\n")
    with open(reads, "wb") as f:
        for i, (n, sub, ind) in enumerate([(9000, 0.3, 0.1), (12000, 0.3, 0.1), (9000, 0.25, 0.05)]):
            st = 3000 + 1000 * i
            r = ref[st:st + 6000] + wc.mutate_scalar(rng, ref[st + 6000:st + 6000 + n], sub, ind) + ref[st + 6000 + n:st + 12000 + n]
            f.write(b">r%d\n%s\n" % (i, r))
        f.write(b">plain\n%s\n" % ref[40000:50000])
    ref_out, got = os.path.join(d, "ref.gaf"), os.path.join(d, "got.gaf")
    with open(ref_out, "wb") as fo:
        subprocess.check_call([rb.REF_BIN, "-c", "-x", "lr", "-t", "2", graph, reads], stdout=fo, stderr=subprocess.DEVNULL)
    monkeypatch.setenv("MGA_WFA_LAST_TBCAP", str(1 << 24))
    mga.wfa_seg_stats(reset=True)
    mga.map_files(graph, [reads], got, cigar=True)
    assert mga.wfa_seg_stats()["problems"] > 0
    a, b = open(ref_out, "rb").read(), open(got, "rb").read()
    lines = b.split(b"\n")
    assert len(lines) == 5 and int(lines[1].split(b"\t")[10]) > 30000  # r1: block length = both sides of the unrelated stretch
    assert len(a) > 0 and a == b, "GAF differs from the reference binary's at byte %d" % next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
