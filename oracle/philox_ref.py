"""Plain numpy model of the render path's on-device draws (``spnerf_rng``, include/spnerf_amd.h).

Written from the header's description and the layout comment of ``philox_words`` — the Philox4x32-10
of Salmon et al. (SC'11) on ``uint64`` arrays, so no 32-bit product is ever truncated — not from
the kernel's code: the GPU tests compare the kernels' draws with this file.

  counter = {id lo, id hi, slot << 16 | idx, step lo}   with id = ray0 + ray (64 bits)
  key     = {seed lo, seed hi ^ step hi}
  uniform = (w0 >> 8) · 2^-24                            (24 bits, [0, 1))
  normal  = sqrt(-2 · ln(((w1 >> 8) + 1) · 2^-24)) · cos(2π · (w2 >> 8) · 2^-24)    in float64

``render_draws`` lists the draws one ``render_rays`` call takes, slot by slot (the table is in
INTEGRATION.md), in the form ``ReplayRandom`` replays.
"""
from __future__ import annotations

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)     # round multipliers
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)     # key schedule (Weyl) increments
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32(counter, key, rounds: int = 10):
    """Philox4x32-``rounds``: counter = 4 and key = 2 arrays (or scalars) of 32-bit words, which
    broadcast against each other; returns the 4 output words as uint64 arrays below 2^32."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _LO for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _LO for k in key)
    for _ in range(rounds):
        p0, p1 = _M0 * c0, _M1 * c2                      # 32 x 32 -> 64 bits, exact in uint64
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _LO, (p0 >> _32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c0, c1, c2, c3


def words(seed: int, step: int, ray0: int, ray, slot: int, idx):
    """The four words of draw ``idx`` of ray ``ray`` (arrays broadcast) of the call whose first
    ray has the global id ``ray0``, in stream ``slot`` of render ``step``."""
    if not 0 <= int(slot) < 1 << 16:
        raise ValueError(f"slot {slot} does not fit 16 bits")
    idx = np.asarray(idx, dtype=np.uint64)
    if idx.size and int(idx.max()) >= 1 << 16:
        raise ValueError("draw index does not fit 16 bits")
    seed, step = int(seed) % (1 << 64), int(step) % (1 << 64)
    with np.errstate(over="ignore"):
        gid = np.uint64(int(ray0) % (1 << 64)) + np.asarray(ray, dtype=np.uint64)   # mod 2^64
    counter = (gid & _LO, gid >> _32, np.uint64(int(slot) << 16) | idx, step & 0xFFFFFFFF)
    key = (seed & 0xFFFFFFFF, (seed >> 32) ^ (step >> 32))
    return philox4x32(counter, key)


def _grid(n_rays: int, n: int):
    return np.arange(n_rays, dtype=np.uint64)[:, None], np.arange(n, dtype=np.uint64)[None, :]


def uniform(seed: int, step: int, ray0: int, n_rays: int, n: int, slot: int) -> np.ndarray:
    """(n_rays, n) float32 uniforms in [0, 1): exact, a 24-bit integer times 2^-24."""
    r, i = _grid(n_rays, n)
    w0 = words(seed, step, ray0, r, slot, i)[0]
    return ((w0 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def normal(seed: int, step: int, ray0: int, n_rays: int, n: int, slot: int) -> np.ndarray:
    """(n_rays, n) float64 standard normals: Box–Muller of words 1 and 2, u1 in (0, 1]."""
    r, i = _grid(n_rays, n)
    _, w1, w2, _ = words(seed, step, ray0, r, slot, i)
    u1 = ((w1 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (w2 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def render_draws(seed: int, step: int, ray0: int, B: int, S: int, *, guided: bool, valid=None, solar: bool = False,
                 n_importance: int = 0, normal_fn=None) -> list:
    """The ordered ``(kind, array)`` draws of ONE ``render_rays`` call of B rays x S samples at
    render ``step``, as ``ReplayRandom`` replays them.  Every stream takes the next slot in call order:

      slot 0            rand   (B, S)         stratified jitter
      [guided]  1       randn  (B, S)         σ noise of pass 1
                2       rand   (B, S)         predicted-depth window
                3       rand   (n_valid, S)   GT window: the rows of the rays with valid > 0 (train
                                              mode only; the slot is taken in test mode too)
      next              randn  (B, Sm)        σ noise of the main pass, Sm = 2S guided, else S
      [solar]   next    randn  (B, Sm)        σ noise of the solar pass
      [fine]    next    rand   (B, n_imp)     sample_pdf
                next    randn  (B, Sm+n_imp)  σ noise of the fine pass
        [solar] next    randn  (B, Sm+n_imp)  σ noise of the fine solar pass

    A σ-noise slot is taken whether or not noise_std lets it be drawn.  ``valid``: the (B,)
    valid_depth of a training render, None in test mode.  ``normal_fn(slot, n)`` overrides where
    the normals come from (float32 (B, n)); the default rounds this file's float64 ones."""
    if normal_fn is None:
        def normal_fn(slot, n):
            return normal(seed, step, ray0, B, n, slot).astype(np.float32)

    def rand(slot, n):
        return uniform(seed, step, ray0, B, n, slot)

    draws = [("rand", rand(0, S))]
    slot, width = 1, S
    if guided:
        draws.append(("randn", normal_fn(1, S)))
        draws.append(("rand", rand(2, S)))
        if valid is not None:
            draws.append(("rand", rand(3, S)[np.asarray(valid).reshape(-1) > 0]))
        slot, width = 4, 2 * S
    passes = [width] * (2 if solar else 1)
    if n_importance > 0:
        passes += [None] + [width + n_importance] * (2 if solar else 1)
    for n in passes:
        draws.append(("rand", rand(slot, n_importance)) if n is None else ("randn", normal_fn(slot, n)))
        slot += 1
    return draws
