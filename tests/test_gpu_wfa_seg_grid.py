"""The grid-wide form of the low-memory WFA rung's first pass (MGA_WFA_SEG_GRID=1, wfa_seg_grid.h): tiles of diagonals, a workgroup each, a block of scores per launch.
Parity with the oracle's exact full-memory WFA, with the tile and the block cut down so that small inputs cross every boundary (tiles, launches, trims, snapshots,
termination on a launch boundary), and the route from the ladder into the rung with the knob set."""
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


def grid_env(monkeypatch, tile, block):
    monkeypatch.setenv("MGA_WFA_SEG_GRID", "1")
    monkeypatch.setenv("MGA_WFA_SEG_GRID_MIN", "0")
    monkeypatch.setenv("MGA_WFA_SEG_GRID_TILE", str(tile))
    monkeypatch.setenv("MGA_WFA_SEG_GRID_BLOCK", str(block))


@pytest.mark.parametrize("step", [3, 17, 256, 5000])
@pytest.mark.parametrize("tile,block", [(64, 8), (64, 64), (256, 17), (4096, 64)])
def test_wfa_seg_grid_parity(ora, base, monkeypatch, tile, block, step):
    T, Q, want = (list(x) for x in base)
    # termination at a checkpoint and one score before it; at a multiple of the block length (a launch boundary) and one score before it
    for t, q, target in wc.checkpoint_pairs(step) + wc.checkpoint_pairs(block):
        es, ec = ora.wfa(t, q, max_iter=-1)
        assert es == target, (step, block, es)
        T.append(t)
        Q.append(q)
        want.append((es, ec))
    assert max(w[0] for w in want) > 512 and min(w[0] for w in want) == 0
    grid_env(monkeypatch, tile, block)
    mga.wfa_seg_stats(reset=True)
    mga.wfa_seg_grid_stats(reset=True)
    sc, cg = mga.wfa_seg_batch(T, Q, step)
    for i in range(len(T)):
        assert want[i][0] == sc[i], (i, len(T[i]), len(Q[i]))
        assert np.array_equal(want[i][1], cg[i]), (i, len(T[i]), len(Q[i]))
    st, gs = mga.wfa_seg_stats(), mga.wfa_seg_grid_stats()
    assert st["problems"] == len(T) and gs["problems"] == len(T)
    assert st["snapshots"] == sum(w[0] // step for w in want)  # one before every slice whose score is a multiple of the step
    if (tile, block) == (64, 8):
        assert gs["max_tiles"] > 1 and gs["launches"] > 1, gs


def test_wfa_ladder_routes_into_the_grid_form(monkeypatch):
    """the cases of test_wfa_ladder_routes_past_the_last_tier (the last HBM tier cut to 16 MiB of traceback, so that their long stretches reach the rung):
    the same scores and CIGARs with the knob set, and the rung's problems take the grid-wide form"""
    rng = np.random.default_rng(7)
    T, Q = [], []
    for n, sub, indel in [(9000, 0.3, 0.1), (12000, 0.3, 0.1), (9500, 0.75, 0.0)]:
        a, m, b = wc.rand_seq(rng, 500), wc.rand_seq(rng, n), wc.rand_seq(rng, 500)
        T.append(a + m + b)
        Q.append(a + wc.mutate_scalar(rng, m, sub, indel) + b)
    monkeypatch.setenv("MGA_WFA_LAST_TBCAP", str(1 << 24))
    monkeypatch.setenv("MGA_WFA_SEG_GRID", "0")  # the workgroup form first
    mga.wfa_seg_grid_stats(reset=True)
    sc, cg = mga.wfa_batch(T, Q)
    assert mga.wfa_seg_grid_stats()["problems"] == 0
    grid_env(monkeypatch, 1024, 64)
    mga.wfa_seg_stats(reset=True)
    sc2, cg2 = mga.wfa_batch(T, Q)
    assert mga.wfa_seg_grid_stats()["problems"] == mga.wfa_seg_stats()["problems"] > 0
    for i in range(len(T)):
        assert sc2[i] == sc[i] and np.array_equal(cg2[i], cg[i]), i
