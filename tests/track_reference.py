"""The definition of argus_roi_from_pose (include/argus_hip.h; csrc/track.hip), restated in numpy: float64 by
default, every operation in float32 with ``dtype=np.float32`` (the reference's own error: what separates two
correct evaluations of the formula). Also the look-at cameras and the case set the tests share. Nothing here reads
a file; nothing here is imported by the package (the product path has no CPU implementation)."""
import math

import numpy as np

FRAME_HW, HW = (96, 160), (64, 64)
HALF_EXTENT, MARGIN, Z_NEAR = (0.035, 0.035, 0.035), 1.5, 0.02
N_POSES = 4096
TOL_PX = 2.0 ** -7  # five times the fp32 restatement's largest distance from fp64 on the case set (1.5e-3 px)


def look_at_camera(eye, target, fovy_deg, frame_hw, up=(0.0, 0.0, 1.0)) -> np.ndarray:
    """The 16 floats [R row-major, t, fx, fy, cx, cy] of a pinhole camera at ``eye`` whose +z axis points at
    ``target``, +x to the right and +y down in the image; fx = fy from the vertical field of view, principal point
    at the frame's center."""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)  # down
    R = np.stack([x, y, z])  # world -> camera
    t = -R @ eye
    f = (frame_hw[0] / 2) / math.tan(math.radians(fovy_deg) / 2)
    return np.concatenate([R.reshape(9), t, [f, f, frame_hw[1] / 2, frame_hw[0] / 2]]).astype(np.float32)


def center_home(n_images: int, frame_hw=FRAME_HW, hw=HW) -> np.ndarray:
    y0, x0 = (frame_hw[0] - hw[0]) // 2, (frame_hw[1] - hw[1]) // 2
    return np.tile(np.float32([y0, x0, hw[0], hw[1]]), (n_images, 1))


def case_set(seed: int = 0):
    """(poses (4096, 7) float32, cameras (2, 16) float32, jitter (8192, 3) float32): two cameras at (0, +-0.15,
    0.13) aimed at the origin with a 70 degree vertical field of view; t ~ N(0, 0.08^2), q ~ N(0, 1)^4 unnormalised;
    the first 50 translations x 1000, then ten zero quaternions, ten NaN and ten infinite translations; jitter
    ln s in [-0.7, 0.7], shifts in [-0.5, 0.5]."""
    rng = np.random.RandomState(seed)
    poses = np.concatenate([rng.normal(0.0, 0.08, (N_POSES, 3)), rng.normal(0.0, 1.0, (N_POSES, 4))], axis=1)
    poses[:50, :3] *= 1000.0
    poses[50:60, 3:] = 0.0
    poses[60:70, rng.randint(0, 3, 10)] = np.nan
    poses[70:80, rng.randint(0, 3, 10)] = np.inf * np.where(rng.randint(0, 2, 10), 1.0, -1.0)
    cams = np.stack([look_at_camera((0.0, s * 0.15, 0.13), (0.0, 0.0, 0.0), 70.0, FRAME_HW) for s in (1.0, -1.0)])
    jit = rng.uniform([-0.7, -0.5, -0.5], [0.7, 0.5, 0.5], size=(2 * N_POSES, 3))
    return poses.astype(np.float32), cams, jit.astype(np.float32)


def _rotation(q, T):
    x, y, z, w = (q[:, i] for i in range(4))
    one, two = T(1), T(2)
    return np.stack([
        np.stack([one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)], -1),
        np.stack([two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)], -1),
        np.stack([two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)], -1)], 1)


def roi_from_pose(poses, cameras, frame_hw, hw, half_extent, margin, z_near, scale=(0.25, 4.0), smooth=1.0,
                  index=None, jitter=None, home=None, prev=None, dtype=np.float64) -> dict:
    """Steps 1-8 for ``batch = len(index) if index is not None else len(poses)`` samples of ``len(cameras)``
    cameras. Returns ``rois`` (n, 4) float32, ``valid`` (n,) int32, ``used`` (= prev), ``touched`` (n,) bool: a
    clamp of step 6 changed a value (or the image is invalid), and ``depth`` (n, 8): the corners' depths (NaN
    for an invalid pose). ``home`` defaults to the center crop, ``prev`` to ``home``."""
    T = np.dtype(dtype).type
    poses = np.asarray(poses, dtype=np.float32)
    cams = np.asarray(cameras, dtype=np.float32).reshape(-1, 16).astype(T)
    n_cams = len(cams)
    if index is not None:
        poses = poses[np.clip(np.asarray(index, dtype=np.int64), 0, len(poses) - 1)]
    B = len(poses)
    n = B * n_cams
    Hs, Ws, h, w = (int(v) for v in (*frame_hw, *hw))
    home = center_home(n, frame_hw, hw) if home is None else np.asarray(home, dtype=np.float32).reshape(n, 4)
    prev = home if prev is None else np.asarray(prev, dtype=np.float32).reshape(n, 4)
    with np.errstate(all="ignore"):
        p = np.repeat(poses.astype(T), n_cams, axis=0)  # image i = b * n_cams + c
        cam = np.tile(cams, (B, 1))
        # 1
        n2 = (p[:, 3:] * p[:, 3:]).sum(1, dtype=T)
        valid = np.isfinite(p).all(1) & np.isfinite(n2) & (n2 > 0)
        q = p[:, 3:] / np.sqrt(np.where(valid, n2, T(1)))[:, None]
        # 2
        Rq = _rotation(q, T)
        signs = np.array([[1 if k & 1 else -1, 1 if k & 2 else -1, 1 if k & 4 else -1] for k in range(8)], dtype=T)
        a = signs * np.asarray(half_extent, dtype=np.float32).astype(T)  # (8, 3)
        X = p[:, None, :3] + np.einsum("nij,kj->nki", Rq, a).astype(T)
        Rc = cam[:, :9].reshape(n, 3, 3)
        Y = (np.einsum("nij,nkj->nki", Rc, X) + cam[:, None, 9:12]).astype(T)
        depth = np.where(valid[:, None], Y[:, :, 2], np.nan)
        valid &= np.isfinite(Y).all((1, 2)) & ~(Y[:, :, 2] < T(np.float32(z_near))).any(1)
        # 3
        Yz = np.where(valid[:, None], Y[:, :, 2], T(1))
        u = cam[:, None, 12] * Y[:, :, 0] / Yz + cam[:, None, 14]
        v = cam[:, None, 13] * Y[:, :, 1] / Yz + cam[:, None, 15]
        vmin, vmax, umin, umax = v.min(1), v.max(1), u.min(1), u.max(1)
        cy, cx = T(0.5) * (vmin + vmax), T(0.5) * (umin + umax)
        sigma = T(np.float32(margin)) * np.maximum((vmax - vmin) / T(h), (umax - umin) / T(w))
        valid &= np.isfinite(sigma) & np.isfinite(cy) & np.isfinite(cx)
        # 4
        if jitter is not None:
            j = np.asarray(jitter, dtype=np.float32).reshape(n, 3).astype(T)
            sigma = sigma * np.exp(j[:, 0])
            cy = cy + j[:, 1] * sigma * T(h)
            cx = cx + j[:, 2] * sigma * T(w)
        # 5
        sm = T(np.float32(smooth))
        if sm < 1:
            pv = prev.astype(T)
            sp, py, px = pv[:, 2] / T(h), pv[:, 0] + T(0.5) * pv[:, 2], pv[:, 1] + T(0.5) * pv[:, 3]
            sigma = sp + sm * (sigma - sp)
            cy, cx = py + sm * (cy - py), px + sm * (cx - px)
        valid &= np.isfinite(sigma) & np.isfinite(cy) & np.isfinite(cx)
        sigma, cy, cx = (np.where(valid, x, T(1)) for x in (sigma, cy, cx))
        # 6
        lo = max(T(np.float32(scale[0])), T(0.25))
        hi = min(T(np.float32(scale[1])), T(4), T(Hs) / T(h), T(Ws) / T(w))
        s6 = np.minimum(np.maximum(sigma, lo), hi)
        touched = s6 != sigma
        out = np.empty((n, 4), dtype=np.float32)
        for axis, (c, nn, S) in enumerate(((cy, h, Hs), (cx, w, Ws))):
            e0 = np.minimum(s6 * T(nn), T(S)).astype(np.float32)
            e = np.minimum(np.maximum(e0, np.float32(nn / 4)), np.float32(min(4 * nn, S)))
            want = c - T(0.5) * e.astype(T)
            o = np.minimum(np.maximum(want, T(0)), T(S) - e.astype(T))
            touched |= (e != e0) | (o != want)
            o32 = o.astype(np.float32)
            over = o32.astype(np.float64) + e.astype(np.float64) > S
            o32 = np.maximum(np.where(over, np.nextafter(o32, np.float32(-1.0)), o32), np.float32(0.0))
            out[:, axis], out[:, 2 + axis] = o32, e
    # 7, 8
    out[~valid] = home[~valid]
    return {"rois": out, "valid": valid.astype(np.int32), "used": prev.copy(), "touched": touched | ~valid,
            "depth": depth}
