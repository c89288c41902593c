"""The numpy Philox reference (oracle/philox_ref.py) on the CPU: known-answer vectors of
Philox4x32-10, the documented counter / key layout, and the distribution of the two draws.

Distribution checks use n = 2^20 draws per stream (16 384 rays x 64 indices, seed 7, step 3):
mean within 5 standard errors, variance within 1 %, Kolmogorov–Smirnov statistic below the
α = 1e-6 bound sqrt(-ln(α/2)/2)/sqrt(n) = 2.63e-3, correlations below 5/sqrt(n) = 4.9e-3."""
import math

import numpy as np
import pytest
import torch

from oracle import philox_ref as pr

SEED, STEP, RAYS, IDX = 7, 3, 16384, 64
N = RAYS * IDX
KS_BOUND = 2.63e-3
CORR_BOUND = 5.0 / math.sqrt(N)

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,out", KAT)
def test_philox4x32_10_known_answers(counter, key, out):
    assert tuple(int(w) for w in pr.philox4x32(counter, key)) == out


def test_known_answers_vectorised():
    """The three vectors as one array call (the form every other function uses)."""
    c = [np.array([k[0][j] for k in KAT], dtype=np.uint64) for j in range(4)]
    k = [np.array([k[1][j] for k in KAT], dtype=np.uint64) for j in range(2)]
    got = pr.philox4x32(c, k)
    for j in range(4):
        assert [int(x) for x in got[j]] == [kat[2][j] for kat in KAT]


def test_words_layout():
    """counter = {id lo, id hi, slot << 16 | idx, step lo}, key = {seed lo, seed hi ^ step hi}."""
    seed, step, ray0, ray, slot, idx = 0x1234_5678_9abc_def0, (5 << 32) | 9, (1 << 32) - 2, 3, 7, 129
    gid = ray0 + ray
    want = pr.philox4x32((gid & 0xffffffff, gid >> 32, (slot << 16) | idx, 9), (0x9abcdef0, 0x12345678 ^ 5))
    got = pr.words(seed, step, ray0, ray, slot, idx)
    assert [int(w) for w in got] == [int(w) for w in want]
    # every field matters: changing any one of them changes the words
    base = [int(w) for w in got]
    for other in ((seed + 1, step, ray0, ray, slot, idx), (seed ^ (1 << 40), step, ray0, ray, slot, idx),
                  (seed, step + 1, ray0, ray, slot, idx), (seed, step ^ (1 << 32), ray0, ray, slot, idx),
                  (seed, step, ray0 + 1, ray, slot, idx), (seed, step, ray0, ray + (1 << 32), slot, idx),
                  (seed, step, ray0, ray, slot + 1, idx), (seed, step, ray0, ray, slot, idx + 1)):
        assert [int(w) for w in pr.words(*other)] != base, other
    # a draw depends on ray0 + ray only
    assert [int(w) for w in pr.words(seed, step, ray0 + 3, 0, slot, idx)] == base
    with pytest.raises(ValueError):
        pr.words(0, 0, 0, 0, 0, 1 << 16)
    with pytest.raises(ValueError):
        pr.words(0, 0, 0, 0, 1 << 16, 0)


def test_draw_formulas():
    w = [int(x) for x in pr.words(SEED, STEP, 100, 5, 2, 9)]
    u = pr.uniform(SEED, STEP, 100, 6, 10, 2)
    assert u.dtype == np.float32 and u.shape == (6, 10)
    assert float(u[5, 9]) == (w[0] >> 8) / 2.0 ** 24
    z = pr.normal(SEED, STEP, 100, 6, 10, 2)
    assert z.dtype == np.float64
    want = math.sqrt(-2.0 * math.log(((w[1] >> 8) + 1) / 2.0 ** 24)) * math.cos(2.0 * math.pi * (w[2] >> 8) / 2.0 ** 24)
    assert abs(float(z[5, 9]) - want) <= 1e-14
    # rows are rays: a call starting 2 rays later draws the same numbers for the same global rays
    np.testing.assert_array_equal(pr.uniform(SEED, STEP, 102, 4, 10, 2), u[2:])


@pytest.fixture(scope="module")
def streams():
    s = {f"u{slot}": pr.uniform(SEED, STEP, 0, RAYS, IDX, slot).astype(np.float64) for slot in (0, 1, 2)}
    s.update({f"n{slot}": pr.normal(SEED, STEP, 0, RAYS, IDX, slot) for slot in (3, 4)})
    s["u0_step4"] = pr.uniform(SEED, STEP + 1, 0, RAYS, IDX, 0).astype(np.float64)
    return s


def _ks(x, cdf):
    x = np.sort(x.ravel())
    n = x.size
    F = cdf(x)
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max((i / n - F).max(), (F - (i - 1) / n).max()))


def _phi(x):
    return 0.5 * (1.0 + torch.erf(torch.from_numpy(x) / math.sqrt(2.0)).numpy())


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("name", ["u0", "u1", "u2", "u0_step4"])
def test_uniform_streams(streams, name):
    x = streams[name]
    assert x.size == N and x.min() >= 0.0 and x.max() < 1.0
    ks = _ks(x, lambda v: v)
    print(f"{name}: mean {x.mean():.6f} var {x.var():.6f} KS {ks:.2e}")
    assert abs(x.mean() - 0.5) <= 5.0 / math.sqrt(12.0 * N)
    assert abs(x.var() * 12.0 - 1.0) <= 0.01
    assert ks < KS_BOUND


@pytest.mark.parametrize("name", ["n3", "n4"])
def test_normal_streams(streams, name):
    x = streams[name]
    assert x.size == N and np.isfinite(x).all()
    ks = _ks(x, _phi)
    print(f"{name}: mean {x.mean():.6f} var {x.var():.6f} KS {ks:.2e}")
    assert abs(x.mean()) <= 5.0 / math.sqrt(N)
    assert abs(x.var() - 1.0) <= 0.01
    assert ks < KS_BOUND


def test_streams_are_uncorrelated(streams):
    names = sorted(streams)
    worst = 0.0
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            c = abs(_corr(streams[a], streams[b]))
            worst = max(worst, c)
            assert c < CORR_BOUND, (a, b, c)
    u0 = streams["u0"]
    lag_idx, lag_ray = abs(_corr(u0[:, :-1], u0[:, 1:])), abs(_corr(u0[:-1], u0[1:]))
    print(f"max |corr| between streams {worst:.2e}; slot 0 lag-1 along index {lag_idx:.2e}, along ray {lag_ray:.2e}")
    assert lag_idx < CORR_BOUND and lag_ray < CORR_BOUND


def test_render_draws_slot_table():
    """Shapes, kinds and slots of a guided + solar + fine training render, and of a plain one."""
    B, S, NI = 6, 8, 5
    valid = np.array([1, 0, 0, 1, 1, 0])
    seen = []

    def nf(slot, n):
        seen.append(slot)
        return np.full((B, n), float(slot), np.float32)

    d = pr.render_draws(SEED, STEP, 50, B, S, guided=True, valid=valid, solar=True, n_importance=NI, normal_fn=nf)
    assert [(k, a.shape) for k, a in d] == [
        ("rand", (B, S)), ("randn", (B, S)), ("rand", (B, S)), ("rand", (3, S)), ("randn", (B, 2 * S)),
        ("randn", (B, 2 * S)), ("rand", (B, NI)), ("randn", (B, 2 * S + NI)), ("randn", (B, 2 * S + NI))]
    assert seen == [1, 4, 5, 7, 8]
    np.testing.assert_array_equal(d[0][1], pr.uniform(SEED, STEP, 50, B, S, 0))
    np.testing.assert_array_equal(d[2][1], pr.uniform(SEED, STEP, 50, B, S, 2))
    np.testing.assert_array_equal(d[3][1], pr.uniform(SEED, STEP, 50, B, S, 3)[valid > 0])   # indexed by ray
    np.testing.assert_array_equal(d[6][1], pr.uniform(SEED, STEP, 50, B, NI, 6))
    # test mode: no GT rows, but the main pass still takes slot 4
    seen.clear()
    d = pr.render_draws(SEED, STEP, 0, B, S, guided=True, solar=False, normal_fn=nf)
    assert [k for k, _ in d] == ["rand", "randn", "rand", "randn"] and seen == [1, 4]
    # unguided: stratified, main, solar
    d = pr.render_draws(SEED, STEP, 0, B, S, guided=False, solar=True)
    assert [(k, a.shape) for k, a in d] == [("rand", (B, S)), ("randn", (B, S)), ("randn", (B, S))]
    np.testing.assert_array_equal(d[2][1], pr.normal(SEED, STEP, 0, B, S, 2).astype(np.float32))
