"""What the relighting tests share (tests/test_relight_ref.py on the CPU, tests/test_gpu_relight.py
on the GPU): the modified weights, the five directions and the tolerances.

``first_layer_sine_init`` leaves the sun columns of ``sun_v_net.0.weight`` at about ±1/259, where a
kernel that ignored the direction would pass.  The tests scale those three columns by SUN_SCALE.
``xyz_features`` enters ``sun_v_net.0`` through weights of the same ±1/259, so on these models the
sun visibility is nearly one number per direction and the ``sun`` plane of direction k is close to
s_k·Σw: two directions separate the planes by |s_i − s_j| / s, and the smallest of the ten pairwise
separations is small for most choices of five directions (1e-3 … 4e-2 for hand-picked sets at any
scale from 10 to 1000).  The directions below were therefore searched, on the CPU with
oracle/ref_cpu.py over a grid of elevation 20°–80° (6° steps) and all azimuths (20° steps), for the
largest minimum separation over the six scenes (cases a / b / c of the view fixture at widths 64
and 256) among sets that reach elevation ≤ 26° and ≥ 74° and all four azimuth quadrants: 0.129 at
x300.  tests/test_relight_ref.py asserts it on the CPU, the GPU tests on ``render_image``'s planes.
"""
import numpy as np

from spnerf_amd.satellite import sun_direction

SUN_SCALE = 300.0
DIR_ANGLES = ((74, 220), (56, 320), (20, 100), (68, 40), (26, 180))   # (elevation, azimuth) in degrees
DIRS = np.stack([sun_direction(el, az) for el, az in DIR_ANGLES]).astype(np.float32)

FP32_RTOL, FP32_ATOL_FRAC = 1e-4, 1e-5     # the project's fp32 bound (golden_util.assert_close)
# bf16 render_image against the fp32 render_image on the modified weights, norm-relative over the
# (5, N, ...) planes, worst of the cases a / b / c at widths 64 and 256, measured on MI355X; the bound
# is twice that, rounded up to one digit (the convention of BF16_TOL_NEW in tests/test_gpu_view.py).
# relight_image bf16 measured on the same scenes beside it.
BF16_TOL = {
    "rgb": 2e-3,   # 7.19e-4 (case c, width 256); relight_image: 7.19e-4
    "sun": 4e-3,   # 1.71e-3 (case b, width 256); relight_image: 1.71e-3
    "sky": 2e-7,   # 7.90e-8 (case a, width 64): the per-direction sky MLP stays fp32; relight_image: 7.90e-8
}
SEPARATION = 20     # the oracle's sun planes differ pairwise by at least this many tolerances


def scale_sun_columns(weights: dict, width: int) -> dict:
    """A copy of a state dict (numpy arrays) with the sun columns of sun_v_net.0.weight scaled."""
    w = dict(weights)
    w["sun_v_net.0.weight"] = w["sun_v_net.0.weight"].copy()
    w["sun_v_net.0.weight"][:, width:] *= SUN_SCALE
    return w


def min_separation(sun_planes) -> float:
    """The smallest pairwise norm-relative difference of the (K, N) sun planes."""
    p = np.asarray(sun_planes, np.float64)
    return min(float(np.linalg.norm(p[i] - p[j]) / np.linalg.norm(p[j])) for i in range(len(p)) for j in range(len(p)) if i != j)
