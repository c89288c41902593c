"""The frozen cases of the confidence tests, shared by tests/test_confidence_ref.py (CPU) and
tests/test_gpu_confidence.py: score volumes (K, cells) float32 whose first columns are the special cells below,
each built for any K >= 1, and whose other columns are random with 30 % NaN and every scored value within
4·TEMPERATURE of the best, so that every plane carries weight in ``mlm``.
"""
import numpy as np

F = np.float32
NAN = F(np.nan)
PLANE_COUNTS = (1, 2, 3, 5, 64, 65, 512)
CELL_COUNTS = (1, 63, 64, 65, 257)
GRID = (16, 17)
STEP = 0.5
TEMPERATURE = 0.1
# (tau, temperature, exclude) of the launches; exclude None stands for K (no plane is outside the pick's own peak).
# 0.0625 is exact in fp32, and so is 0.75 − 0.0625: the "tau met" cell below meets it exactly
MEASURES = ((0.05, TEMPERATURE, 1), (0.0, TEMPERATURE, 2), (0.0625, 0.02, None))
TAU_EXACT, BEST_EXACT = 0.0625, 0.75


def _low(K, value=0.25):
    return np.full(K, value, F)


def all_nan(K):
    return np.full(K, NAN, F)


def one_scored(K):
    col = all_nan(K)
    col[K // 2] = 0.5
    return col


def pick_at_bottom(K):
    return (F(0.9) - np.arange(K, dtype=F) * F(0.4 / K)).astype(F)


def pick_at_top(K):
    return pick_at_bottom(K)[::-1].copy()


def flat(K):
    return _low(K, 0.5)


def infinities(K):
    col = pick_at_top(K)
    col[0] = np.inf                                                       # unscored, though it compares above everything
    if K > 2:
        col[K - 1] = -np.inf                                              # the pick moves to K − 2, its upper neighbour unscored
    return col


def plateau(K):
    col = _low(K)
    col[K // 3:K // 3 + 3] = 0.8
    return col


def second_peak(K, offset):
    """The pick at K // 2 and a second peak ``offset`` planes above it (inside exclude 1 at 1, just outside at 2)."""
    col = _low(K)
    p = K // 2
    col[p] = 0.9
    if p + offset < K:
        col[p + offset] = 0.85
    if offset > 1 and p + 1 < K:
        col[p + 1] = 0.3
    return col


def tau_cell(K, ulps):
    """best 0.75 at plane 0 and a far peak ``ulps`` fp32 ulps of best below best − TAU_EXACT."""
    col = _low(K)
    col[0] = BEST_EXACT
    if K > 1:
        col[K - 1] = F(BEST_EXACT - TAU_EXACT) - F(ulps) * np.spacing(F(BEST_EXACT))
    return col


def unscored_neighbour(K):
    col = pick_at_top(K)
    p = K // 2
    col[p] = 0.95
    if p >= 1:
        col[p - 1] = NAN
    return col


def equal_peaks(K):
    col = _low(K)
    col[K // 4] = 0.7
    col[K - 1 - K // 4] = 0.7
    return col


def tie_with_neighbour(K):
    """Two equal values side by side at the top of a ramp: the lower plane is the pick and the only local maximum."""
    col = pick_at_top(K)
    if K > 1:
        col[K - 2] = col[K - 1]
    return col


SPECIAL = (all_nan, one_scored, pick_at_bottom, pick_at_top, flat, infinities, plateau, lambda K: second_peak(K, 1), lambda K: second_peak(K, 2),
           lambda K: tau_cell(K, 0), lambda K: tau_cell(K, 1), unscored_neighbour, equal_peaks, tie_with_neighbour)
# the column each special cell stands in (where there are that many cells)
COLUMN = {name: c for c, name in enumerate(("all_nan", "one_scored", "pick_at_bottom", "pick_at_top", "flat", "infinities", "plateau", "peak_inside",
                                            "peak_outside", "tau_met", "tau_missed", "unscored_neighbour", "equal_peaks", "tie_with_neighbour"))}
assert len(COLUMN) == len(SPECIAL)


def random_columns(K, cells, seed):
    rng = np.random.default_rng(seed)
    v = (F(0.9) - rng.uniform(0.0, 4 * TEMPERATURE, (K, cells))).astype(F)
    v[rng.uniform(size=(K, cells)) < 0.3] = NAN
    return v


def volume(K, cells):
    """(K, cells) float32: the special cells in the first columns — where there is one column, the special cell
    K mod len(SPECIAL) — and random columns behind them."""
    v = random_columns(K, cells, 1000 * K + cells)
    if cells == 1:
        v[:, 0] = SPECIAL[K % len(SPECIAL)](K)
    else:
        for c, make in enumerate(SPECIAL[:cells]):
            v[:, c] = make(K)
    return v


def measures(K):
    return [(tau, temperature, K if exclude is None else exclude) for tau, temperature, exclude in MEASURES]
