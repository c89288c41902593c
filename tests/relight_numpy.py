"""A float64 restatement of the relighting split (csrc/relight.hip, spnerf_amd.relight) in numpy:
the base pre-activation of ``sun_v_net.0`` per point plus one vector per direction, then the rest of
``sun_v_net``, the sky, the irradiance and the ray sums.  ``p`` maps state-dict names to arrays."""
import numpy as np


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def base_preactivation(p, feat):
    """W0[:, :feat]·F + b0, (P, H): what is computed once per point."""
    W0 = np.asarray(p["sun_v_net.0.weight"], np.float64)
    return feat @ W0[:, :feat.shape[1]].T + np.asarray(p["sun_v_net.0.bias"], np.float64)


def direction_vectors(p, dirs, n_feat):
    """W0[:, feat:]·d_k, (K, H): what is computed once per direction."""
    W0 = np.asarray(p["sun_v_net.0.weight"], np.float64)
    return np.asarray(dirs, np.float64) @ W0[:, n_feat:].T


def sun_visibility(p, feat, dirs):
    """(K, P): sun_v_net on cat[feat, d_k] through the split."""
    base = base_preactivation(p, feat)
    out = []
    for v in direction_vectors(p, dirs, feat.shape[1]):
        h = np.sin(base + v)
        for j in (2, 4):
            h = np.sin(h @ np.asarray(p[f"sun_v_net.{j}.weight"], np.float64).T + np.asarray(p[f"sun_v_net.{j}.bias"], np.float64))
        out.append(sigmoid(h @ np.asarray(p["sun_v_net.6.weight"], np.float64)[0] + float(np.asarray(p["sun_v_net.6.bias"])[0])))
    return np.stack(out)


def sky_colour(p, dirs):
    """(K, 3): sky_color of the direction alone."""
    h = np.maximum(np.asarray(dirs, np.float64) @ np.asarray(p["sky_color.0.weight"], np.float64).T +
                   np.asarray(p["sky_color.0.bias"], np.float64), 0.0)
    return sigmoid(h @ np.asarray(p["sky_color.2.weight"], np.float64).T + np.asarray(p["sky_color.2.bias"], np.float64))


def relight_sums(w, albedo, sun_v, sky):
    """w (B, S), albedo (B, S, 3), sun_v (K, B, S), sky (K, 3) -> rgb (K, B, 3) clamped to [0, 1],
    sun (K, B) = Σ w·s, sky (K, B, 3) = Σ w·sky_k."""
    s = sun_v[..., None]
    irr = s + (1.0 - s) * sky[:, None, None, :]
    rgb = np.clip(np.sum(w[None, ..., None] * albedo[None] * irr, -2), 0.0, 1.0)
    return rgb, np.sum(w[None] * sun_v, -1), np.sum(w, -1)[None, :, None] * sky[:, None, :]
