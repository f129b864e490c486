"""The grid-wide form of the low-memory WFA rung's second pass (MGA_WFA_SEG_GRID_P2=1, wfa_seg_grid.h): the traceback pass over tiles of diagonals, re-tiled from one
tile after every checkpoint.  Parity with the oracle's exact full-memory WFA with the tile and the block cut down so that small inputs cross tile edges, launch
boundaries, trims, checkpoints (taken, and for step 3 passed over) and the regrowth after a collapse; the knob off; and the route from the ladder."""
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


def grid_env(monkeypatch, tile, block, p2):
    for k, v in (("", 1), ("_MIN", 0), ("_TILE", tile), ("_BLOCK", block), ("_P2", p2)):
        monkeypatch.setenv("MGA_WFA_SEG_GRID" + k, str(v))


@pytest.mark.parametrize("step", [3, 17, 256, 5000])
@pytest.mark.parametrize("tile,block", [(64, 8), (64, 64), (256, 17), (4096, 64)])
@pytest.mark.parametrize("p2", [1, 0])
def test_wfa_seg_grid_p2_parity(ora, base, monkeypatch, p2, tile, block, step):
    T, Q, want = (list(x) for x in base)
    # termination at a checkpoint and one score before it; at a multiple of the block length (a launch boundary) and one score before it
    for t, q, target in wc.checkpoint_pairs(step) + wc.checkpoint_pairs(block):
        es, ec = ora.wfa(t, q, max_iter=-1)
        assert es == target, (step, block, es)
        T.append(t)
        Q.append(q)
        want.append((es, ec))
    grid_env(monkeypatch, tile, block, p2)
    mga.wfa_seg_grid_p2_stats(reset=True)
    sc, cg = mga.wfa_seg_batch(T, Q, step)
    for i in range(len(T)):
        assert want[i][0] == sc[i], (i, len(T[i]), len(Q[i]))
        assert np.array_equal(want[i][1], cg[i]), (i, len(T[i]), len(Q[i]))
    gs = mga.wfa_seg_grid_p2_stats()
    assert gs["problems"] == (len(T) if p2 else 0)  # knob off: the parent's path
    if (tile, block, p2) == (64, 8, 1):
        assert gs["launches"] > 1, gs
        # between two checkpoints the band of pass 2 holds at most 2 (step + 17) + 1 diagonals: 69 at step 17, which is below two tiles of 64 -- there it must stay one tile
        assert gs["max_tiles"] == 1 if step == 17 else gs["max_tiles"] > 1, gs


def test_wfa_ladder_routes_into_the_grid_p2_form(monkeypatch):
    """the three stretches of test_wfa_ladder_routes_into_the_grid_form: the same scores and CIGARs with the second pass grid-wide, for every problem of the rung"""
    rng = np.random.default_rng(7)
    T, Q = [], []
    for n, sub, indel in [(9000, 0.3, 0.1), (12000, 0.3, 0.1), (9500, 0.75, 0.0)]:
        a, m, b = wc.rand_seq(rng, 500), wc.rand_seq(rng, n), wc.rand_seq(rng, 500)
        T.append(a + m + b)
        Q.append(a + wc.mutate_scalar(rng, m, sub, indel) + b)
    monkeypatch.setenv("MGA_WFA_LAST_TBCAP", str(1 << 24))
    grid_env(monkeypatch, 1024, 64, 0)
    mga.wfa_seg_grid_p2_stats(reset=True)
    sc, cg = mga.wfa_batch(T, Q)
    assert mga.wfa_seg_grid_p2_stats()["problems"] == 0
    grid_env(monkeypatch, 1024, 64, 1)
    mga.wfa_seg_stats(reset=True)
    sc2, cg2 = mga.wfa_batch(T, Q)
    assert mga.wfa_seg_grid_p2_stats()["problems"] == mga.wfa_seg_stats()["problems"] > 0
    for i in range(len(T)):
        assert sc2[i] == sc[i] and np.array_equal(cg2[i], cg[i]), i
