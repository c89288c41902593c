"""float64 numpy statement of the ground-grid rays (csrc/ortho.hip, spnerf_amd.ortho): the inverse
transverse-Mercator projection, the ray assembly and the sub-ray reduction.

Written apart from the kernel.  The Krüger series is summed as one complex series
ζ' = ζ − Σ β_j sin(2jζ) with ζ = ξ + iη (the kernel sums its real and imaginary parts with
separate circular and hyperbolic factors), and the conformal latitude goes back to the geodetic one
through the isometric latitude ψ = asinh(tan χ) by the fixed point
φ ← atan(sinh(ψ + e·atanh(e·sin φ))), whose error shrinks by e² ≈ 0.0067 per pass (the kernel
takes Newton steps on τ = tan φ).  The β_j are Karney (2011), eq. (36), to n⁶.  ECEF uses the
constants of the reference's ``geodetic_to_ecef`` (modules/utils.py:80-100)."""
from fractions import Fraction as Fr

import numpy as np

A_WGS84 = 6378137.0
F_WGS84 = 1.0 / 298.257223563
K0 = 0.9996

# β_j as rows of rational coefficients of n^j, n^(j+1), ... n^6
_BETA = (
    (Fr(1, 2), Fr(-2, 3), Fr(37, 96), Fr(-1, 360), Fr(-81, 512), Fr(96199, 604800)),
    (Fr(1, 48), Fr(1, 15), Fr(-437, 1440), Fr(46, 105), Fr(-1118711, 3870720)),
    (Fr(17, 480), Fr(-37, 840), Fr(-209, 4480), Fr(5569, 90720)),
    (Fr(4397, 161280), Fr(-11, 504), Fr(-830251, 7257600)),
    (Fr(4583, 161280), Fr(-108847, 3991680)),
    (Fr(20648693, 638668800),),
)


def _series_constants():
    n = F_WGS84 / (2.0 - F_WGS84)
    A = A_WGS84 / (1.0 + n) * (1.0 + n ** 2 / 4.0 + n ** 4 / 64.0 + n ** 6 / 256.0)
    beta = [sum(float(c) * n ** (j + 1 + k) for k, c in enumerate(row)) for j, row in enumerate(_BETA)]
    return A, beta


def utm_inverse(easting, northing, zone, south=False):
    """(lat, lon) in degrees of WGS-84 UTM coordinates in metres."""
    e = np.asarray(easting, np.float64)
    nn = np.asarray(northing, np.float64)
    A, beta = _series_constants()
    zeta = ((nn - (1e7 if south else 0.0)) + 1j * (e - 500000.0)) / (K0 * A)
    zp = zeta.copy()
    for j, b in enumerate(beta, 1):
        zp = zp - b * np.sin(2 * j * zeta)
    xi, eta = zp.real, zp.imag
    tan_chi = np.sin(xi) / np.sqrt(np.sinh(eta) ** 2 + np.cos(xi) ** 2)     # of the conformal latitude χ
    lam = np.arctan2(np.sinh(eta), np.cos(xi))
    ecc = np.sqrt(F_WGS84 * (2.0 - F_WGS84))
    psi = np.arcsinh(tan_chi)
    phi = np.arctan(tan_chi)
    for _ in range(12):
        phi = np.arctan(np.sinh(psi + ecc * np.arctanh(ecc * np.sin(phi))))
    return np.degrees(phi), np.degrees(lam) + (6.0 * zone - 183.0)


def geodetic_to_ecef(lat, lon, alt):
    a, b = 6378137.0, 6356752.314245
    e2 = 1 - (b ** 2 / a ** 2)
    la, lo = np.radians(lat), np.radians(lon)
    N = a / np.sqrt(1 - e2 * np.sin(la) ** 2)
    return np.stack([(N + alt) * np.cos(la) * np.cos(lo), (N + alt) * np.cos(la) * np.sin(lo),
                     ((b ** 2 / a ** 2) * N + alt) * np.sin(la)], -1)


def cell_points(xoff, ytop, xsize, ysize, res, s=1, rows=None):
    """(E, N) of every sub-ray, each (n_rows, xsize, s, s): sub-ray (a, b) of cell (j, i) stands at
    E = xoff + (i + (b + ½)/s)·res, N = ytop − (j + (a + ½)/s)·res."""
    j0, j1 = (0, ysize) if rows is None else rows
    j = np.arange(j0, j1, dtype=np.float64)[:, None, None, None]
    i = np.arange(xsize, dtype=np.float64)[None, :, None, None]
    a = np.arange(s, dtype=np.float64)[None, None, :, None]
    b = np.arange(s, dtype=np.float64)[None, None, None, :]
    E = xoff + (i + (b + 0.5) / s) * res + 0 * (j + a)
    N = ytop - (j + (a + 0.5) / s) * res + 0 * (i + b)
    return E, N


def ortho_rays(xoff, ytop, xsize, ysize, res, zone, south, min_alt, max_alt, center, rng, sun=None, s=1, rows=None):
    """The (n, 8) or (n, 11) float64 rays of the grid, ray ((j·xsize + i)·s + a)·s + b: one cast to
    float32 away from the kernel's.  ``center`` and ``rng`` are taken as the float32 values the
    scene holds."""
    E, N = cell_points(xoff, ytop, xsize, ysize, res, s, rows)
    lat, lon = utm_inverse(E.ravel(), N.ravel(), zone, south)
    hi = geodetic_to_ecef(lat, lon, float(max_alt))
    lo = geodetic_to_ecef(lat, lon, float(min_alt))
    c = np.asarray(center, np.float32).astype(np.float64).reshape(1, 3)
    r = float(np.float32(rng))
    d = lo - hi
    length = np.sqrt(np.sum(d * d, -1, keepdims=True))
    cols = [(hi - c) / r, d / length, np.zeros_like(length), length / r]
    if sun is not None:
        cols.append(np.broadcast_to(np.asarray(sun, np.float32).astype(np.float64).reshape(1, 3), hi.shape))
    return np.concatenate(cols, -1)


def reduce_subrays(x, s, dtype=None):
    """Box filter over the s² contiguous sub-rays of a cell: ``x`` (..., cells·s², w) ->
    (..., cells, w).  The sum is float64 in ascending sub-ray order, one divide by s², one cast to
    ``dtype`` (x's own by default).  s = 1 is the identity."""
    x = np.asarray(x)
    if s == 1:
        return x
    dtype = x.dtype if dtype is None else dtype
    lead, n, w = x.shape[:-2], x.shape[-2], x.shape[-1]
    v = x.reshape(lead + (n // (s * s), s * s, w)).astype(np.float64)
    acc = v[..., 0, :].copy()
    for k in range(1, s * s):
        acc = acc + v[..., k, :]
    return (acc / np.float64(s * s)).astype(dtype)


def classes(logits):
    """First index of the maximum, a NaN counting as the maximum (the first NaN stands): the rule
    of the ``sem_class`` plane.  (cells, C) -> (cells,) int32."""
    x = np.asarray(logits)
    out = np.zeros(x.shape[0], np.int32)
    for r in range(x.shape[0]):
        best, cls = x[r, 0], 0
        for c in range(1, x.shape[1]):
            m = x[r, c]
            if best == best and (m > best or m != m):
                best, cls = m, c
        out[r] = cls
    return out
