"""The region-of-interest conditioning of the pose head (include/argus_hip.h: argus_roi_embed,
argus_pose_tail_roi; argus_amd/models.py: NCameraCNNConfig.roi_frame_hw), restated in numpy: float64 by default, or
every operation rounded to float32 with ``dtype=np.float32`` (the CPU tests measure how far float32 arithmetic
alone moves the result, against the bar the kernel is held to). The product path has no CPU implementation.

Image i = b * n_cams + c has region (y0, x0, eh, ew) in pixels of an Hs x Ws frame, resampled to h x w:

    rho[b][4c + 0] = (y0 + eh / 2 - Hs / 2) / Hs        rho[b][4c + 2] = ln(eh / h)
    rho[b][4c + 1] = (x0 + ew / 2 - Ws / 2) / Ws        rho[b][4c + 3] = ln(ew / w)
    z1 = output_mlp.0(g0) + rho @ w_r.T,  g1 = gelu(z1),  then the head as without the term.
"""
import math

import numpy as np

FRAME_HW, HW = (96, 128), (64, 64)
# (batch, n_cams) of the argus_roi_embed test and, for each, the bar on |z_out - ref| in units of
# S = |z_in| + sum_k |w_r[j][k] * rho[b][k]|: 4 * 16 + 1 roundings of 2^-24 on partial sums bounded by S at 16
# cameras (2^-17 covers them), 13 at three cameras and fewer (2^-19 leaves a factor of two over them)
EMBED_CASES = [(1, 1), (1, 2), (3, 2), (16, 1), (64, 2), (65, 3), (2, 16)]


def embed_bar(n_cams: int) -> float:
    return 2.0 ** -17 if n_cams == 16 else 2.0 ** -19


# rho against the float64 features, "within 4 ulp": the ulp is float32's spacing at the bound of each feature's
# domain, 2^-24 at 1/2 for the centres and 2^-23 at ln 4 for the logarithms. A bound relative to the VALUE cannot
# be met by any float32 evaluation of this definition: y0 + eh / 2 - Hs / 2 and ln(eh / h) cancel to 0 at the centre
# crop, where one rounding of y0 + eh / 2 (<= 2^-24 Hs, i.e. 2^-24 after the division) or of eh / h (2^-24 relative,
# the same absolute step of its logarithm) is arbitrarily many ulps of the result. Counted: centres <= 2^-24 + one
# division rounding (2^-26); logarithms <= 2^-24 + logf's own error (a few ulp of a value <= ln 4: <= 2 * 2^-23).
RHO_ULP = np.array([2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 2.0 ** -23])


def center_crop_roi(frame_hw=FRAME_HW, hw=HW) -> np.ndarray:
    """(y0, x0, eh, ew) of the centred crop of ``hw`` at unit scale (exactly centred when the margins are even)."""
    return np.array([(frame_hw[0] - hw[0]) / 2, (frame_hw[1] - hw[1]) / 2, hw[0], hw[1]], dtype=np.float64)


def features(rois, n_cams: int, frame_hw=FRAME_HW, hw=HW, dtype=np.float64) -> np.ndarray:
    """rois (batch * n_cams, 4) -> rho (batch, 4 * n_cams), every operation in ``dtype``."""
    r = np.asarray(rois).astype(dtype).reshape(-1, 4)
    (Hs, Ws), (h, w) = [tuple(dtype(v) for v in p) for p in (frame_hw, hw)]
    half = dtype(0.5)
    rho = np.stack([(r[:, 0] + r[:, 2] * half - Hs * half) / Hs, (r[:, 1] + r[:, 3] * half - Ws * half) / Ws,
                    np.log(r[:, 2] / h), np.log(r[:, 3] / w)], axis=1).astype(dtype)
    return rho.reshape(-1, 4 * n_cams)


def embed(z, rho, w_r, dtype=np.float64) -> np.ndarray:
    """z (batch, 128) + e, e[b][j] accumulated from 0 over k ascending, every step rounded to ``dtype``."""
    z, rho, w_r = (np.asarray(a).astype(dtype) for a in (z, rho, w_r))
    e = np.zeros_like(z)
    for k in range(rho.shape[1]):
        e = (e + w_r[None, :, k] * rho[:, k, None]).astype(dtype)
    return (z + e).astype(dtype)


def embed_scale(z, rho, w_r) -> np.ndarray:
    """S of the bar: |z_in| + sum_k |w_r[j][k] * rho[b][k]|, float64."""
    z, rho, w_r = (np.asarray(a, dtype=np.float64) for a in (z, rho, w_r))
    return np.abs(z) + np.abs(rho) @ np.abs(w_r).T


def gelu(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * x * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))


def head(g0, params, rho=None, w_r=None) -> np.ndarray:
    """float64 pred (batch, 6) of the output MLP from g0 (batch, d); params = (w0, b0, w2, b2, w4, b4)."""
    w0, b0, w2, b2, w4, b4 = (np.asarray(p, dtype=np.float64) for p in params)
    z1 = np.asarray(g0, dtype=np.float64) @ w0.T + b0
    if rho is not None:
        z1 = z1 + np.asarray(rho, dtype=np.float64) @ np.asarray(w_r, dtype=np.float64).T
    return gelu(gelu(z1) @ w2.T + b2) @ w4.T + b4


def embed_case(batch: int, n_cams: int, seed: int = 0):
    """The inputs of one argus_roi_embed case, float32: regions from ``resident.sample_rois`` (inside the served
    domain) with the exact centre crop as the first one of every case but (1, 1), w_r uniform in [-1, 1], z normal."""
    from argus_amd.resident import sample_rois

    rng = np.random.default_rng(1000 * batch + n_cams + seed)
    crop = center_crop_roi()
    rois = sample_rois(rng, batch * n_cams, FRAME_HW, HW, (int(crop[0]), int(crop[1])), scale=(0.5, 1.5),
                       shift=0.25).astype(np.float32)
    if len(rois) > 1:  # (1, 1) keeps its random region; every other case starts with the exact centre crop
        rois[0] = crop
    w_r = rng.uniform(-1.0, 1.0, (128, 4 * n_cams)).astype(np.float32)
    z = rng.standard_normal((batch, 128)).astype(np.float32)
    return rois, w_r, z
