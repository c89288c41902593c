"""The numpy statement of the semi-global aggregation (tests/sgm_numpy.py, include/spnerf_amd_sgm.h)
pinned to answers it did not produce — no GPU needed.

* Dyadic volumes: with scores, p1, p2 and ``unscored`` multiples of 1/64 and small K and grids, every
  intermediate of the definition is exactly representable in fp32, so the statement must equal, bit for
  bit, an exact implementation in integers (units of 1/64) that walks every path on its own from the cell
  whose predecessor lies outside the grid.
* Closed forms: p2 = 0 returns the scores; K = 1 returns 1 − C; a cell without any score is NaN at every
  plane and has index −1, yet a path that crosses it still carries its neighbour's plane across.
* The step scene of tests/sgm_cases.py: picking each cell on its own is wrong at exactly the 51 outlier
  cells; after the aggregation the wrong cells are the statement's known few, all within one cell of the
  step — but for the grid's corner (0, 0) at p2 = 0.5 with 8 paths: five of the eight directions begin in
  that cell, so there the aggregate is 5/8 the cell's own cost, and an outlier that beats the true plane by
  0.25 survives three penalties of 0.5 / 8 each (it does not survive p2 = 1).
"""
import numpy as np
import pytest

import sgm_cases as sc
import sgm_numpy as sg

F = np.float32


def exact(vol64, p1, p2, unscored, paths):
    """The aggregation of integer scores (units of 1/64; None where unscored) in exact integer arithmetic:
    (S (K, H, W) int, units of 1/64; scored (H, W) bool), every path walked on its own."""
    K, H, W = len(vol64), len(vol64[0]), len(vol64[0][0])
    C = [[[64 - vol64[k][j][i] if vol64[k][j][i] is not None else unscored for i in range(W)] for j in range(H)] for k in range(K)]
    S = np.zeros((K, H, W), np.int64)
    for dj, di in sg.DIRECTIONS[:paths]:
        for j0 in range(H):
            for i0 in range(W):
                if 0 <= j0 - dj < H and 0 <= i0 - di < W:
                    continue                                             # not the first cell of a path
                j, i, prev = j0, i0, None
                while 0 <= j < H and 0 <= i < W:
                    here = [C[k][j][i] for k in range(K)]
                    if prev is not None:
                        M = min(prev)
                        for k in range(K):
                            m = min([prev[k], M + p2] + ([prev[k - 1] + p1] if k >= 1 else []) + ([prev[k + 1] + p1] if k <= K - 2 else []))
                            here[k] += m - M
                    for k in range(K):
                        S[k, j, i] += here[k]
                    prev, j, i = here, j + dj, i + di
    scored = np.array([[any(vol64[k][j][i] is not None for k in range(K)) for i in range(W)] for j in range(H)])
    return S, scored


def dyadic(K, H, W):
    vol = sc.random_volume(K, H, W, dyadic=True)
    as64 = [[[int(round(float(vol[k, j, i]) * 64)) if np.isfinite(vol[k, j, i]) else None for i in range(W)] for j in range(H)]
            for k in range(K)]
    return vol, as64


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (5, 7)])
@pytest.mark.parametrize("K", [1, 2, 3, 9])
def test_the_statement_equals_exact_integer_paths_on_dyadic_volumes(K, H, W, paths):
    vol, as64 = dyadic(K, H, W)
    if H * W > 1:
        assert np.isnan(vol).any() and not np.isfinite(vol[:, H - 1, W // 2]).any()
    for p1, p2, unscored in ((8, 64, 64), (0, 32, 80), (16, 16, 64), (0, 0, 48)):
        S, scored = exact(as64, p1, p2, unscored, paths)
        want = ((64 * paths - S) / (64.0 * paths)).astype(F)             # exact: small integers over a power of two
        want[:, ~scored] = np.nan
        got = sg.aggregate(vol, p1 / 64.0, p2 / 64.0, unscored / 64.0, paths)
        assert got.dtype == F and got.tobytes() == want.tobytes(), (p1, p2, unscored)


@pytest.mark.parametrize("paths", [4, 8])
def test_closed_forms(paths):
    vol = sc.random_volume(9, 5, 7, dyadic=True)
    fin = np.isfinite(vol)
    scored = fin.any(axis=0)
    out = sg.aggregate(vol, 0.0, 0.0, 0.75, paths)                       # p2 = 0: every plane is as cheap as the cheapest
    assert np.array_equal(out[fin], vol[fin])
    assert (out[~fin & scored[None]] == F(0.25)).all() and np.isnan(out[:, ~scored]).all()
    one = sc.random_volume(1, 5, 7, dyadic=True)
    out = sg.aggregate(one, 0.125, 1.0, 1.0, paths)                      # K = 1: m = M
    assert np.array_equal(out[np.isfinite(one)], one[np.isfinite(one)]) and np.isnan(out[~np.isfinite(one)]).all()
    arb = sc.random_volume(3, 5, 7)
    out = sg.aggregate(arb, 0.0, 0.0, 1.0, paths)                        # arbitrary scores: up to the roundings of 1 − (1 − v)
    fin = np.isfinite(arb)
    assert np.abs(out[fin].astype(np.float64) - arb[fin]).max() <= 2.0 ** -22


def test_a_cell_without_scores_is_nan_yet_paths_cross_it():
    nan = np.nan
    row = np.array([[0.75, 0.0, 0.0], [0.75, 0.0, 0.0], [nan, nan, nan], [0.5, 0.25, 0.53125]], F)     # [cell][plane]
    vol = np.ascontiguousarray(row.T[:, None, :])                                                   # (3, 1, 4)
    assert sc.raw_index(vol).tolist() == [[0, 0, -1, 2]]
    out = sg.aggregate(vol, 0.125, 0.5, 1.0, 4)
    assert np.isnan(out[:, 0, 2]).all() and np.isfinite(out[:, 0, [0, 1, 3]]).all()
    # (0,+1) reaches the last cell as C + [0, 0.125, 0.25]; the other three directions begin there
    assert out[:, 0, 3].tolist() == [1.0 - 2.0 / 4, 1.0 - 3.125 / 4, 1.0 - 2.125 / 4]
    picked = sg.pick(out, vol, -10.0, 2.0)
    assert picked["index"].tolist() == [[0, 0, -1, 0]]
    assert np.isnan(picked["altitude"][0, 2]) and np.isnan(picked["score"][0, 2]) and np.isnan(picked["photo"][0, 2])
    assert picked["photo"][0, [0, 1, 3]].tolist() == [0.75, 0.75, 0.5] and picked["altitude"][0, 3] == -10.0
    alone = sg.aggregate(vol[:, :, 3:], 0.125, 0.5, 1.0, 4)                                          # without its neighbours the cell keeps plane 2
    assert sg.pick(alone, vol[:, :, 3:], -10.0, 2.0)["index"].tolist() == [[2]]
    inf = vol.copy()
    inf[0, 0, 3] = np.inf                                                                            # ±inf is unscored too: photo is NaN there
    picked = sg.pick(sg.aggregate(inf, 0.125, 0.5, -1.0, 4), inf, -10.0, 2.0)
    assert picked["index"][0, 3] == 0 and np.isnan(picked["photo"][0, 3]) and np.isfinite(picked["score"][0, 3])


STEP_CELLS = {(0.125, 1.0, 4): [], (0.125, 1.0, 8): [(3, 15), (14, 15), (16, 14)], (0.125, 0.5, 4): [(16, 14)],
              (0.125, 0.5, 8): [(0, 0), (1, 16), (3, 15), (14, 15), (16, 14)]}


def test_the_step_scene_without_aggregation_is_wrong_at_the_outliers():
    vol, truth = sc.step_scene()
    j, i = np.meshgrid(np.arange(17), np.arange(33), indexing="ij")
    wrong = sc.raw_index(vol) != truth
    assert wrong.sum() == sc.STEP_OUTLIERS == 51 and np.array_equal(wrong, (7 * j + 3 * i) % 11 == 0)
    assert np.isnan(vol).any() and (np.isnan(vol).sum(axis=0) == 4).sum() == 37


@pytest.mark.parametrize("p1,p2,paths", sorted(sc.STEP_WRONG))
def test_the_step_scene_is_recovered_but_for_the_known_cells(p1, p2, paths):
    vol, truth = sc.step_scene()
    picked = sg.pick(sc.step_reference(p1, p2, paths), vol, 0.0, 1.0)
    wrong = picked["index"] != truth
    print(f"p1 {p1} p2 {p2} paths {paths}: wrong at {np.argwhere(wrong).tolist()}")
    assert wrong.sum() == sc.STEP_WRONG[(p1, p2, paths)] < sc.STEP_OUTLIERS
    assert [tuple(c) for c in np.argwhere(wrong).tolist()] == STEP_CELLS[(p1, p2, paths)]
    corner = np.zeros_like(wrong)
    corner[0, 0] = (p2, paths) == (0.5, 8)                               # the module docstring
    assert sc.near_step(wrong & ~corner)
    assert np.array_equal(picked["photo"][~wrong], np.full((~wrong).sum(), 0.5, F))
