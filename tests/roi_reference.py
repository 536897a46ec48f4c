"""fp64 restatement of the region-of-interest resampling (include/argus_hip.h, argus_frames_resample): a helper
for test_roi_host.py and test_gpu_stem_roi.py, not a test module.

Per axis, with source length S, output length n, origin o and extent e (pixel j covers [j, j + 1)):

    s = e / n, r = max(s, 1), c_i = o + (i + 0.5) * s
    taps j from max(0, floor(c_i - r + 0.5)) to min(S, floor(c_i + r + 0.5)) - 1
    t_ij = max(0, 1 - |j + 0.5 - c_i| / r), w_ij = t_ij / sum_j t_ij

written here as a dense (n, S) matrix per axis; a resampled image is Wy @ image @ Wx^T."""
import math

import torch


def axis_matrix(S: int, n: int, o: float, e: float) -> torch.Tensor:
    """(n, S) fp64: row i holds the weights w_ij of output index i."""
    s = e / n
    r = max(s, 1.0)
    m = torch.zeros(n, S, dtype=torch.float64)
    for i in range(n):
        c = o + (i + 0.5) * s
        lo, hi = max(0, math.floor(c - r + 0.5)), min(S, math.floor(c + r + 0.5))
        for j in range(lo, hi):
            m[i, j] = max(0.0, 1.0 - abs(j + 0.5 - c) / r)
        m[i] /= m[i].sum()
    return m


def resample(images: torch.Tensor, rois, hw) -> torch.Tensor:
    """``images`` (N, C, Hs, Ws), any dtype, values as the network sees them; ``rois`` N x (y0, x0, height, width);
    returns (N, C, h, w) fp64."""
    N, _, Hs, Ws = images.shape
    out = []
    for img, (y0, x0, hh, ww) in zip(images.double(), [[float(v) for v in r] for r in rois]):
        wy, wx = axis_matrix(Hs, hw[0], y0, hh), axis_matrix(Ws, hw[1], x0, ww)
        out.append(wy @ img @ wx.T)
    assert len(out) == N
    return torch.stack(out)


def exact_case(n_img: int, frame_hw, hw, origin, seed: int = 0):
    """Frames and regions whose resampled pixels are exact in fp32, bf16 and fp16: fp32 frames of integers in
    [0, 3], an even integer origin and extent 2n, so every tap weight is 1/8 or 3/8 per axis and every pixel a
    multiple of 1/64 below 4 (8 significant bits at most). Returns (frames (n_img, 3, Hs, Ws) fp32, rois)."""
    gen = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 4, (n_img, 3, *frame_hw), generator=gen).float()
    assert origin[0] % 2 == 0 and origin[1] % 2 == 0
    assert origin[0] + 2 * hw[0] <= frame_hw[0] and origin[1] + 2 * hw[1] <= frame_hw[1]
    rois = [(float(origin[0]), float(origin[1]), 2.0 * hw[0], 2.0 * hw[1])] * n_img
    return frames, rois
