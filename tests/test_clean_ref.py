"""The numpy statement of the DSM cleaning (tests/clean_numpy.py) pinned to closed forms, and the frozen cases
(tests/clean_cases.py) to what they claim to be — no GPU needed."""
import numpy as np

import clean_cases as cc
import clean_numpy as cn

NAN = np.float32(np.nan)
F = np.float32


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_a_serpentine_is_one_component_with_label_zero():
    dsm, cells = cc.serpentine((9, 9))
    assert cells == 5 * 9 + 4 and int(np.isfinite(dsm).sum()) == cells
    assert dsm[0, 0] == 0 and dsm[8, 8] == F((cells - 1) * 0.25)          # a ramp whose ends are 12 m apart
    label, size = cn.components(dsm, 0.25)
    on = np.isfinite(dsm)
    assert (label[on] == 0).all() and (size[on] == cells).all()
    assert (label[~on] == -1).all() and (size[~on] == 0).all()
    out, _, _ = cn.speckle(dsm, 0.25, cells - 1)
    assert same(out, dsm)
    out, _, _ = cn.speckle(dsm, 0.25, cells)
    assert np.isnan(out).all()
    label, size = cn.components(dsm, 0.125)                               # no step is met: every cell alone
    assert (size[on] == 1).all() and (label[on] == np.flatnonzero(on)).all()


def test_a_checkerboard_is_one_component_per_cell():
    dsm, max_diff = cc.pattern("checkerboard", (5, 6))
    label, size = cn.components(dsm, max_diff)
    assert (size == 1).all() and (label == np.arange(30).reshape(5, 6)).all()
    out, _, _ = cn.speckle(dsm, max_diff, 0)                              # max_size 0 removes nothing
    assert same(out, dsm)
    assert np.isnan(cn.speckle(dsm, max_diff, 1)[0]).all()
    label, size = cn.components(dsm, 10.0)
    assert (size == 30).all() and (label == 0).all()


def test_squares_touching_at_a_corner_are_two_components():
    dsm = np.full((6, 6), NAN, np.float32)
    dsm[0:3, 0:3] = 4.0
    dsm[3:6, 3:6] = 4.0
    label, size = cn.components(dsm, 0.0)
    assert (label[0:3, 0:3] == 0).all() and (label[3:6, 3:6] == 3 * 6 + 3).all()
    assert (size[np.isfinite(dsm)] == 9).all() and (label[~np.isfinite(dsm)] == -1).all()
    out, _, _ = cn.speckle(dsm, 0.0, 9)
    assert np.isnan(out).all()


def test_a_ramp_of_steps_equal_to_max_diff_is_one_component_and_an_ulp_more_is_w():
    W = 40
    ramp = (np.arange(W, dtype=np.float32) * F(0.25))[None]
    label, size = cn.components(ramp, 0.25)
    assert (label == 0).all() and (size == W).all()
    above = cc.ulp_ramp(W, 0.25)[None]
    steps = above[0, 1:] - above[0, :-1]
    assert (steps > F(0.25)).all() and steps[0] == np.nextafter(F(0.25), F(1)) and (steps <= F(0.25) + np.spacing(above[0, 1:])).all()
    label, size = cn.components(above, 0.25)
    assert (label == np.arange(W)).all() and (size == 1).all()
    # holes: NaN and ±inf join nothing and keep their bytes
    holes = np.array([[1.0, np.inf, 1.0, np.nan, 1.0, -np.inf, 1.0]], np.float32)
    out, label, size = cn.speckle(holes, 100.0, 1)
    assert (label[0] == [0, -1, 2, -1, 4, -1, 6]).all() and (size[0] == [1, 0, 1, 0, 1, 0, 1]).all()
    assert same(out, np.array([[np.nan, np.inf, np.nan, np.nan, np.nan, -np.inf, np.nan]], np.float32))
    huge = np.array([[3e38, -3e38]], np.float32)                          # the difference overflows: not joined
    assert (cn.components(huge, 3e38)[1] == 1).all()


def test_the_median_of_a_known_window():
    win = np.array([[7.0, np.nan, 1.0], [np.nan, 5.0, np.nan], [3.0, np.nan, np.inf]], np.float32)   # 4 finite: 1 3 5 7
    assert cn.median(win, 1)[1, 1] == 3.0                                 # the lower median, never 4
    assert np.isnan(cn.median(win, 1, min_count=5)[1, 1]) and cn.median(win, 1, min_count=4)[1, 1] == 3.0
    win5 = win.copy()
    win5[0, 1] = 4.0                                                      # 5 finite: 1 3 4 5 7
    assert cn.median(win5, 1)[1, 1] == 4.0
    none = np.full((3, 3), NAN, np.float32)
    assert np.isnan(cn.median(none, 1, fill=True)).all() and np.isnan(cn.median(none, 1)).all()
    # a hole keeps its bytes unless fill
    out = cn.median(win, 1)
    assert np.isnan(out[0, 1]) and out[2, 2] == np.inf
    filled = cn.median(win, 1, fill=True)
    assert filled[2, 2] == 5.0 and filled[0, 1] == 5.0                    # {5} and {7, 1, 5}
    # both zeros come out as +0
    z = cn.median(np.array([[-0.0, -0.0, 0.0]], np.float32), 1)
    assert (z == 0).all() and not np.signbit(z).any()


def test_the_median_clips_its_window_at_corners_and_edges():
    dsm = np.arange(25, dtype=np.float32).reshape(5, 5)
    out = cn.median(dsm, 1)
    assert out[0, 0] == 1.0                                               # {0, 1, 5, 6}: rank 1
    assert out[0, 2] == 3.0                                               # {1, 2, 3, 6, 7, 8}: rank (6 − 1) / 2 = 2
    assert out[2, 2] == 12.0 and out[4, 4] == 19.0                        # {18, 19, 23, 24}
    assert out[2, 0] == 10.0                                              # {5, 6, 10, 11, 15, 16}: rank 2
    assert cn.median(dsm, 2)[0, 0] == 6.0                                 # {0,1,2,5,6,7,10,11,12}: rank 4
    assert cn.median(dsm, 3)[2, 2] == 12.0 and cn.median(dsm, 3, min_count=26)[2, 2] != cn.median(dsm, 3, min_count=26)[2, 2]


def test_the_fill_of_single_holes_corners_and_wide_holes():
    dsm = np.arange(25, dtype=np.float32).reshape(5, 5)
    one = dsm.copy()
    one[2, 2] = NAN
    out, filled = cn.fill(one, 1)
    assert out[2, 2] == 6.0 and filled.sum() == 1 and filled[2, 2] == 1   # the lowest of the eight neighbours is NW
    assert cn.fill(one, 1, cn.NEAREST)[0][2, 2] == 13.0                   # E comes first among the four at distance 1
    rest = np.ones((5, 5), bool)
    rest[2, 2] = False
    assert same(out[rest], dsm[rest])
    corner = dsm.copy()
    corner[0, 0] = NAN
    out, filled = cn.fill(corner, 4, min_dirs=3)
    assert out[0, 0] == 1.0 and filled[0, 0] == 1                         # E, S and SE exist; the others leave the grid at once
    out, filled = cn.fill(corner, 4, min_dirs=4)
    assert np.isnan(out[0, 0]) and filled.sum() == 0
    wide = np.zeros((9, 9), np.float32)
    wide[1:8, 1:8] = NAN                                                  # 7 x 7: the centre is 4 steps from any value
    out, filled = cn.fill(wide, 3)
    assert np.isnan(out[4, 4]) and filled[4, 4] == 0 and filled[1:8, 1:8].sum() == 48
    out, filled = cn.fill(wide, 4)
    assert out[4, 4] == 0.0 and filled[1:8, 1:8].all()
    inf = np.array([[2.0, np.inf, np.nan, np.nan]], np.float32)           # an inf is a hole: filled, and never a value
    out, filled = cn.fill(inf, 1)
    assert out[0, 1] == 2.0 and np.isnan(out[0, 2]) and (filled[0] == [0, 1, 0, 0]).all()
    assert np.isposinf(cn.fill(np.array([[np.inf, np.nan]], np.float32), 4)[0][0, 0])   # unfilled: its own bytes


def test_nearest_ties_go_to_the_earlier_direction_and_min_dirs_counts_directions():
    dsm = np.full((5, 5), NAN, np.float32)
    dsm[2, 4], dsm[0, 2] = 9.0, 1.0                                       # E and N, both two steps away
    out, _ = cn.fill(dsm, 2, cn.NEAREST)
    assert out[2, 2] == 9.0                                               # E before N
    assert cn.fill(dsm, 2, cn.LOWEST)[0][2, 2] == 1.0
    dsm[1, 3] = 5.0                                                       # NE at one diagonal step: 2 < 4
    assert cn.fill(dsm, 2, cn.NEAREST)[0][2, 2] == 5.0
    assert cn.fill(dsm, 2, cn.NEAREST, min_dirs=3)[1][2, 2] == 1 and cn.fill(dsm, 2, cn.NEAREST, min_dirs=4)[1][2, 2] == 0
    assert cn.fill(dsm, 1, cn.NEAREST, min_dirs=1)[0][2, 2] == 5.0 and cn.fill(dsm, 1, min_dirs=2)[1][2, 2] == 0
    assert [d for d in cn.DIRECTIONS[:3]] == [(0, 1), (-1, 1), (-1, 0)]   # E, NE, N with north towards row 0


def test_the_chain_marks_what_each_step_did():
    dsm = np.zeros((8, 8), np.float32)
    dsm[1, 1] = 30.0                                                      # a speckle
    dsm[5, 5] = 0.5                                                       # within max_diff: the median's
    dsm[6, 1] = 2.0
    weight = np.ones((8, 8), np.float32)
    weight[6, 1], weight[0, 7] = 0.1, np.nan
    out = cn.chain(dsm, 1.0, 3, weight=weight, min_weight=0.25, radius=1, reach=2)
    want = np.zeros((8, 8), np.uint8)
    want[6, 1] = want[0, 7] = 1
    want[1, 1] = 2
    want[5, 5] = 4
    assert same(out["rejected"], want)
    assert (out["filled"] == (want == 1) | (want == 2)).all() and same(out["dsm"], np.zeros((8, 8), np.float32))
    assert out["label"][1, 1] == 9 and out["size"][1, 1] == 1 and out["label"][6, 1] == -1
    bare = cn.chain(dsm, 1.0, 3, radius=0)
    assert np.isnan(bare["dsm"][1, 1]) and bare["dsm"][5, 5] == 0.5 and not bare["filled"].any() and bare["rejected"].sum() == 2 * 2


def test_the_frozen_cases_are_what_they_claim():
    assert cc.T == 16 and len(cc.GRIDS) == 7
    for shape in cc.GRIDS:
        for name in cc.PATTERNS:
            dsm, max_diff = cc.pattern(name, shape)
            assert not dsm.flags.writeable and max_diff >= 0
        dsm, _ = cc.pattern("serpentine", shape)
        _, size = cn.components(dsm, 0.25)
        assert size.max() == np.isfinite(dsm).sum() == cc.serpentine(shape)[1]
        dsm, md = cc.pattern("spiral", shape)
        assert cn.components(dsm, md)[1].max() == np.isfinite(dsm).sum()
        dsm, md = cc.pattern("diagonal", shape)
        assert cn.components(dsm, md)[1].max() == 1
    dsm, md = cc.pattern("walls", (65, 130))
    label, size = cn.components(dsm, md)
    # the first tile is closed off (both gaps lie beyond it); the gaps keep the other three quarters in one piece
    assert np.isnan(dsm).sum() == 65 + 130 - 1 - 2 and sorted(np.unique(label[label >= 0])) == [0, cc.T]
    assert size[0, 0] == (cc.T - 1) ** 2 and size[0, cc.T] == 65 * 130 - 192 - (cc.T - 1) ** 2
    dsm, md = cc.pattern("exact", (17, 33))
    _, size = cn.components(dsm, md)
    assert (size[0] == 33).all() and (size[2] == 1).all() and (size[1] == 0).all()
    original, corrupted, mask = cc.restoration()
    label, size = cn.components(np.where(mask, F(1.0), NAN).astype(np.float32), 0.0)
    assert mask.sum() == size[np.unique(label[label >= 0]) // 65, np.unique(label[label >= 0]) % 65].sum()
    assert len(np.unique(label[label >= 0])) == cc.SPECKLES and size.max() == cc.SPECKLE_MAX and size[mask].min() == 1
    assert ((corrupted - original)[mask] == cc.RAISED).all() and same(corrupted[~mask], original[~mask])
    grown = np.zeros_like(mask)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            grown |= np.roll(np.roll(np.pad(mask, 2), dy, 0), dx, 1)[2:-2, 2:-2]
    assert not (grown & (original != F(-16.0))).any()                     # nothing within 2 cells of the box
    out = cn.chain(corrupted, 1.0, cc.SPECKLE_MAX, radius=0, reach=8)
    assert same(out["dsm"], original) and same(out["filled"], mask.astype(np.uint8)) and same(out["rejected"], 2 * mask.astype(np.uint8))
