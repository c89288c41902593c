"""DSM registration — CPU only.  The numpy restatement (tests/dsmr_numpy.py) against what the
reference's modules/dsmr.py computed (tests/golden/dsmr.npz, made by gen_dsmr_golden.py), the
pick rule on hand-made images, and the evaluation interface of the library
(include/spnerf_amd_eval.h) without a compute call."""
import ctypes
import os
import re

import numpy as np
import pytest

import dsmr_numpy as dn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dsmr.npz")
CASES = ("a", "b", "c")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fixture_is_what_the_issue_asks_for(golden):
    assert os.path.getsize(GOLDEN) <= 632 * 1024
    shapes = {c: golden[f"{c}_u"].shape for c in CASES}
    assert shapes == {"a": (136, 120), "b": (217, 205), "c": (37, 53)}
    assert [len(golden[f"{c}_shifts"]) for c in CASES] == [2, 3, 1]
    assert tuple(golden["a_shifts"][0]) == (7, -4) and tuple(golden["b_shifts"][0]) == (-9, 6)
    assert np.isnan(golden["c_tables"][0]).any()         # shifts without any finite pair
    for c in CASES:
        assert golden[f"{c}_u"].dtype == np.float32 and golden[f"{c}_applied"].dtype == np.float32
        for t in golden[f"{c}_tables"]:                   # the argmax is far from rounding
            f = np.sort(t[np.isfinite(t)])
            assert f[-1] - f[-2] >= 1e-6
        assert golden[f"{c}_moments"][2] > 0 and golden[f"{c}_moments"][3] > 0


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_reference(golden, case):
    u, v = golden[f"{case}_u"], golden[f"{case}_v"]
    trace = []
    dx, dy, a, b, m = dn.compute_shift(u, v, scaling=True, trace=trace)
    trace = trace[::-1]                                   # finest first, like the fixture
    assert len(trace) == len(golden[f"{case}_shifts"]) == dn.levels_of(*u.shape) + 1
    for lv, (ldx, ldy, table) in enumerate(trace):
        assert (ldx, ldy) == tuple(golden[f"{case}_shifts"][lv]), lv
        ref = golden[f"{case}_tables"][lv]
        assert np.array_equal(np.isnan(table), np.isnan(ref)), lv
        assert np.nanmax(np.abs(table - ref)) <= 1e-12, lv
    gm = golden[f"{case}_moments"]
    assert m[5] == gm[5]
    assert np.all(np.abs(np.array(m[:5]) - gm[:5]) <= 1e-12 * np.abs(gm[:5]))
    gs = golden[f"{case}_shift_scaled"]
    assert (dx, dy) == (gs[0], gs[1]) and abs(a - gs[2]) <= 1e-12 * abs(gs[2]) and abs(b - gs[3]) <= 1e-12 * abs(gs[3])
    dx, dy, a, b, _ = dn.compute_shift(u, v, scaling=False)
    gp = golden[f"{case}_shift_plain"]
    assert (dx, dy, a) == (gp[0], gp[1], 1.0) and abs(b - gp[3]) <= 1e-12 * abs(gp[3])
    # downsample2x bit for bit, NaN positions included
    assert np.array_equal(dn.down2x(u), golden[f"{case}_down"], equal_nan=True)
    # the shifted image after the float32 cast, with the fixture's own transform
    out = dn.apply_shift(v, int(gp[0]), int(gp[1]), gp[2], gp[3]).astype(np.float32)
    assert np.array_equal(out, golden[f"{case}_applied"], equal_nan=True)
    with np.errstate(invalid="ignore"):
        assert abs(np.nanmean(np.abs(out.astype(np.float64) - u)) - golden[f"{case}_mae"]) <= 1e-5


def test_down2x_takes_the_block_the_reference_writes_last():
    u = np.arange(20, dtype=np.float64).reshape(4, 5)
    d = dn.down2x(u)
    assert d.shape == (2, 3)
    assert d[0, 0] == np.mean([u[1, 1], u[2, 1], u[1, 2], u[2, 2]])
    assert d[1, 2] == u[3, 4]                               # the last pixel alone
    assert d[1, 0] == np.mean([u[3, 1], u[3, 2]])           # the row below is out of range
    u[1:3, 1:3] = np.nan
    assert np.isnan(dn.down2x(u)[0, 0])
    u[2, 2] = np.inf                                        # non-finite is missing, not only NaN
    assert np.isnan(dn.down2x(u)[0, 0])


def test_pick_rule_ties_and_nans():
    # equal maxima: the first in scan order (y outer, x inner) stands
    t = np.zeros((3, 3))
    t[0, 2] = t[1, 0] = 0.5
    assert dn.pick(t, 10, 20) == (11, 19)
    # a NaN never wins, wherever it sits
    t = np.full((3, 3), np.nan)
    t[2, 1] = -0.9
    assert dn.pick(t, 0, 0) == (0, 1)
    # nothing finite: the centre stands
    assert dn.pick(np.full((3, 3), np.nan), 4, -3) == (4, -3)
    assert dn.pick(np.full((3, 3), -np.inf), 4, -3) == (4, -3)   # -inf is not > -inf either


def test_ties_and_all_nan_on_8x8_images():
    rng = np.random.default_rng(0)
    # u periodic with period 2 in x: the shifts x = -2, 0, 2 see the same pixels wherever v is
    # finite in all of them, so their correlations tie and the first in scan order is kept
    row = np.array([1.0, 3.0] * 4)
    u = np.tile(row, (8, 1)) + 3.0 * rng.standard_normal(8)[:, None]
    v = np.full((8, 8), np.nan)
    v[:, 2:6] = u[:, 2:6]
    t = dn.ncc_table(u, v, 2, 0, 0)
    assert t[2, 0] == t[2, 2] == t[2, 4] == np.nanmax(t)
    assert dn.pick(t, 0, 0) == (-2, 0) == dn.recursive_ncc(u, v, 2)
    # all-NaN v: every correlation is NaN, the initial shift stands, the moments are NaN
    u = rng.standard_normal((8, 8))
    v = np.full((8, 8), np.nan)
    assert np.isnan(dn.ncc_table(u, v, 2, 0, 0)).all()
    dx, dy, a, b, m = dn.compute_shift(u, v, irange=2, dx=1, dy=-1)
    assert (dx, dy) == (1, -1) and np.isnan(a) and np.isnan(b) and m[5] == 0 and all(np.isnan(m[:5]))
    # a constant image has zero deviation: 0 / 0, never a winner
    assert np.isnan(dn.ncc_table(np.ones((8, 8)), rng.standard_normal((8, 8)), 1, 0, 0)).all()
    # floor division on the way down: -9 // 2 = -5
    big = rng.standard_normal((120, 104))
    trace = []
    dn.recursive_ncc(big, np.full_like(big, np.nan), 1, -9, 7, trace)
    assert [(t[0], t[1]) for t in trace] == [(-5, 3), (-10, 6)]


# ---- the evaluation interface of the library ------------------------------------------------

def eval_header_symbols():
    txt = open(os.path.join(ROOT, "include", "spnerf_amd_eval.h")).read()
    return sorted(set(re.findall(r"\b(spnerf_eval_[a-z0-9_]+)\s*\(", txt)))


def test_eval_exports_match_the_header():
    from spnerf_amd import _eval_lib, _lib
    syms = eval_header_symbols()
    assert syms == ["spnerf_eval_abi_version", "spnerf_eval_dsm_apply_shift", "spnerf_eval_dsm_down2x",
                    "spnerf_eval_dsm_register", "spnerf_eval_dsm_register_workspace_bytes"]
    L = _eval_lib.lib()
    assert L is _lib.lib()                                 # one library, two signature tables
    for s in syms:
        assert hasattr(L, s), s
    assert sorted(_eval_lib.SIGNATURES) == syms, "eval signature table out of sync with the header"
    assert not set(_eval_lib.SIGNATURES) & set(_lib.SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "spnerf_amd_eval.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (SPNERF_EVAL_[A-Z_]+) (\d+)\b", hdr)}
    assert L.spnerf_eval_abi_version() == consts["SPNERF_EVAL_ABI_VERSION"] == _eval_lib.SPNERF_EVAL_ABI_VERSION
    assert consts["SPNERF_EVAL_DSM_MAX_IRANGE"] == _eval_lib.DSM_MAX_IRANGE
    assert "(2 + 2 * 256)" in hdr and _eval_lib.DSM_SUMS_DOUBLES == 2 + 2 * 256
    assert ctypes.sizeof(_eval_lib.DsmShift) == 56
    assert L.spnerf_abi_version() == 2                      # the core ABI is untouched


def test_eval_argument_errors_are_reported():
    from spnerf_amd import _eval_lib
    L = _eval_lib.lib()
    assert L.spnerf_eval_dsm_register(None, None, 64, 64, 5, 0, 0, None, None, None, None) == -1
    assert b"dsm_register: NULL" in L.spnerf_last_error()
    one = ctypes.c_void_p(256)      # never dereferenced: the arguments are refused first
    assert L.spnerf_eval_dsm_register(one, one, 0, 64, 5, 0, 0, one, None, one, None) == -1
    assert b"shape" in L.spnerf_last_error()
    assert L.spnerf_eval_dsm_register(one, one, 64, 64, -1, 0, 0, one, None, one, None) == -1
    assert b"irange" in L.spnerf_last_error()
    assert L.spnerf_eval_dsm_register_workspace_bytes(64, 64, -1) == -1
    assert L.spnerf_eval_dsm_register_workspace_bytes(64, -2, 5) == -1
    assert L.spnerf_eval_dsm_apply_shift(None, 8, 8, None, 0, 0, 0, 1.0, 0.0, None, one, None, None, None) == -1
    assert b"dsm_apply_shift: NULL" in L.spnerf_last_error()
    assert L.spnerf_eval_dsm_apply_shift(one, 8, 8, None, 0, 0, 0, 1.0, 0.0, None, None, one, None, None) == -1
    assert b"need the reference" in L.spnerf_last_error()
    # the workspace holds the pyramid and the partial sums: it grows with the image and the window
    a = L.spnerf_eval_dsm_register_workspace_bytes(100, 100, 5)
    b = L.spnerf_eval_dsm_register_workspace_bytes(101, 101, 5)
    c = L.spnerf_eval_dsm_register_workspace_bytes(101, 101, 2)
    assert 0 < c < b and 0 < a < b


def test_python_surface_refuses_cpu_tensors_and_bad_shapes():
    import torch
    from spnerf_amd import _lib, dsm
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        dsm.compute_shift(torch.zeros(8, 8), torch.zeros(8, 8))
    with pytest.raises(_lib.SpnerfError, match="MI355X"):
        dsm.dsm_mae(torch.zeros(8, 8), torch.zeros(8, 8), register="ncc")
    with pytest.raises(ValueError):
        dsm.dsm_mae(np.zeros((8, 8)), np.zeros((8, 8)), register="xy")
    assert dsm.pyramid_levels(101, 100) == 1 and dsm.pyramid_levels(101, 101) == 2
    assert dsm.pyramid_levels(217, 205) == 3 == dn.levels_of(217, 205) + 1
    # the default keeps the mean-offset MAE (oracle/dsm_ref.py) bit for bit, on the host
    from oracle import dsm_ref
    rng = np.random.default_rng(1)
    p, g = rng.standard_normal((9, 7)), rng.standard_normal((9, 7))
    p[2, 3] = np.nan
    assert dsm.dsm_mae(p, g) == dsm.dsm_mae(p, g, register="z") == dsm_ref.dsm_mae(p, g)
