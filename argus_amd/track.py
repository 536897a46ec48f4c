"""Aim the region of interest from the pose: the host side of ``argus_roi_from_pose`` (csrc/track.hip).

``PoseSession(track=TrackConfig(...))`` ends every replay by writing the region the next replay resamples, from the
pose it just produced and the cameras' calibration: a closed-loop tracker with no host step. ``ResidentLoader(
roi_track=TrackConfig(...))`` draws the training regions around the labelled cube with the same launch, so the
network is trained on what the tracker will show it.

Conventions (include/argus_hip.h). A pose is ``[t(3), qx, qy, qz, qw]``: the cube's frame in the world. A camera is
world-to-camera: ``Y = R X + t`` with +x right, +y down, +z forward (the computer-vision convention), and the pixel of
``Y`` is ``(u, v) = (fx Yx / Yz + cx, fy Yy / Yz + cy)`` with ``v`` the row. The region is the bounding box of the
cube's eight projected corners, scaled by ``margin`` about its center with the network's aspect ratio kept, clamped
into ``pose_session.check_roi``'s domain.

There is no CPU implementation here (the product path has none); tests/track_reference.py restates the kernel.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import math
from typing import Optional, Sequence

import numpy as np

from argus_amd._lib import TrackCfg

__all__ = ["Camera", "TrackConfig", "camera_from_mujoco", "load_calibration", "sample_roi_jitter"]


def _floats(v, n: int, what: str) -> tuple:
    try:
        a = np.asarray(v, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: expected {n} numbers, got {v!r}") from None
    if a.size != n or not np.isfinite(a).all():
        raise ValueError(f"{what}: expected {n} finite numbers, got {v!r}")
    return tuple(float(x) for x in a)


@dataclasses.dataclass(frozen=True)
class Camera:
    """A calibrated pinhole camera, world-to-camera: ``Y = R X + t`` (+x right, +y down, +z forward), pixel
    ``(fx Yx / Yz + cx, fy Yy / Yz + cy)``. ``R``: 9 numbers row-major (or 3 x 3); ``t``: 3."""

    R: Sequence[float]
    t: Sequence[float]
    fx: float
    fy: float
    cx: float
    cy: float

    def __post_init__(self):
        object.__setattr__(self, "R", _floats(self.R, 9, "Camera R"))
        object.__setattr__(self, "t", _floats(self.t, 3, "Camera t"))
        for name in ("fx", "fy", "cx", "cy"):
            object.__setattr__(self, name, _floats(getattr(self, name), 1, f"Camera {name}")[0])
        if self.fx <= 0 or self.fy <= 0:
            raise ValueError("Camera fx, fy: focal lengths must be positive")

    def words(self) -> np.ndarray:
        """The 16 float32 the device reads: R row-major, t, fx, fy, cx, cy."""
        return np.array([*self.R, *self.t, self.fx, self.fy, self.cx, self.cy], dtype=np.float32)


def camera_from_mujoco(pos, quat_wxyz, fovy_deg: float, frame_hw: tuple) -> Camera:
    """The ``Camera`` of a MuJoCo camera given as MuJoCo states it: ``pos`` and ``quat_wxyz`` are the camera frame's
    position and orientation IN THE WORLD (camera-to-world, quaternion w first), and the camera looks along its
    own -z axis with +y up and +x right. ``Camera`` wants world-to-camera with +z forward and +y down, so the y and
    z axes are flipped and the transform is inverted: ``R = diag(1, -1, -1) R_wc^T``, ``t = -R pos``. ``fovy_deg`` is
    the vertical field of view over the ``frame_hw = (Hs, Ws)`` frame: ``fy = fx = (Hs / 2) / tan(fovy / 2)``
    (square pixels), principal point at the frame's center ``(cx, cy) = (Ws / 2, Hs / 2)``."""
    pos = np.array(_floats(pos, 3, "camera_from_mujoco pos"))
    w, x, y, z = _floats(quat_wxyz, 4, "camera_from_mujoco quat")
    n = math.sqrt(w * w + x * x + y * y + z * z)
    if n == 0.0:
        raise ValueError("camera_from_mujoco quat: the zero quaternion is no orientation")
    w, x, y, z = w / n, x / n, y / n, z / n
    Rwc = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    fovy = float(fovy_deg)
    if not 0.0 < fovy < 180.0:
        raise ValueError(f"camera_from_mujoco fovy: {fovy_deg!r} is outside (0, 180) degrees")
    Hs, Ws = int(frame_hw[0]), int(frame_hw[1])
    R = np.diag([1.0, -1.0, -1.0]) @ Rwc.T
    f = (Hs / 2) / math.tan(math.radians(fovy) / 2)
    return Camera(R.reshape(9), -R @ pos, f, f, Ws / 2, Hs / 2)


@dataclasses.dataclass(frozen=True)
class TrackConfig:
    """What ``argus_roi_from_pose`` needs beside the pose. ``cameras``: one ``Camera`` per camera image of a
    sample, in the order of the frames. ``half_extent``: the cube's half side lengths along its own axes (one number
    for all three). ``margin``: the region's size over the projected bounding box's. ``scale = (lo, hi)``: bounds on
    the region's size over the network's (the kernel also applies [1/4, 4] and the frame). ``z_near``: a corner
    nearer than this (or behind the camera) invalidates the image, which then gets ``home``. ``smooth`` in (0, 1]:
    the share of the way from the previous region to the new one taken per call (1: no memory). ``home``: the region
    of an invalid image and of ``reset_roi()``, ``(4,)`` or ``(batch, n_cams, 4)``; None: the center crop."""

    cameras: Sequence[Camera]
    half_extent: Sequence[float]
    margin: float = 1.5
    scale: tuple = (0.25, 4.0)
    z_near: float = 0.01
    smooth: float = 1.0
    home: Optional[object] = None

    def __post_init__(self):
        cams = tuple(self.cameras)
        if not cams or not all(isinstance(c, Camera) for c in cams):
            raise ValueError("TrackConfig cameras: a non-empty sequence of Camera")
        object.__setattr__(self, "cameras", cams)
        he = np.asarray(self.half_extent, dtype=np.float64).reshape(-1)
        he = np.repeat(he, 3) if he.size == 1 else he
        object.__setattr__(self, "half_extent", _floats(he, 3, "TrackConfig half_extent"))
        object.__setattr__(self, "scale", _floats(self.scale, 2, "TrackConfig scale"))
        for name in ("margin", "z_near", "smooth"):
            object.__setattr__(self, name, _floats(getattr(self, name), 1, f"TrackConfig {name}")[0])
        if min(self.half_extent) <= 0 or self.margin <= 0 or self.z_near <= 0:
            raise ValueError("TrackConfig half_extent, margin, z_near: must be positive")
        if self.scale[0] > self.scale[1]:
            raise ValueError("TrackConfig scale: (lo, hi) with lo <= hi")
        if not 0.0 < self.smooth <= 1.0:
            raise ValueError("TrackConfig smooth: must lie in (0, 1]")

    def camera_words(self) -> np.ndarray:
        """(n_cams, 16) float32: the device's camera table."""
        return np.stack([c.words() for c in self.cameras])

    def struct(self, smooth: Optional[float] = None) -> TrackCfg:
        """The ``argus_track_cfg`` of this configuration (``smooth`` overrides it: the loader forces 1)."""
        return TrackCfg((C.c_float * 3)(*self.half_extent), self.margin, self.scale[0], self.scale[1], self.z_near,
                        self.smooth if smooth is None else float(smooth))


def _key(d: dict, key: str, where: str):
    if not isinstance(d, dict) or key not in d:
        raise ValueError(f"calibration: {where}{key!r} is missing")
    return d[key]


def load_calibration(path) -> TrackConfig:
    """A ``TrackConfig`` from a JSON file holding its settings::

        {"cameras": [{"R": [9], "t": [3], "fx": .., "fy": .., "cx": .., "cy": ..},
                     {"mujoco": {"pos": [3], "quat": [w, x, y, z], "fovy": degrees}}],
         "frame_hw": [Hs, Ws],            # needed by the mujoco form only
         "half_extent": 0.035 | [3], "z_near": 0.02,
         "margin": 1.5, "scale": [0.25, 4.0], "smooth": 1.0, "home": [y0, x0, height, width]}   # optional

    ``ValueError`` names the missing or malformed key."""
    try:
        with open(path) as f:
            d = json.load(f)
    except json.JSONDecodeError as e:
        raise ValueError(f"calibration: {path} is not JSON ({e})") from None
    cams = _key(d, "cameras", "")
    if not isinstance(cams, list) or not cams:
        raise ValueError("calibration: 'cameras' must be a non-empty list")
    known = {"cameras", "frame_hw", "half_extent", "z_near", "margin", "scale", "smooth", "home"}
    unknown = sorted(set(d) - known)
    if unknown:
        raise ValueError(f"calibration: unknown key {unknown[0]!r}")
    out = []
    for i, c in enumerate(cams):
        where = f"cameras[{i}]."
        try:
            if isinstance(c, dict) and "mujoco" in c:
                m = c["mujoco"]
                where += "mujoco."
                hw = _floats(_key(d, "frame_hw", ""), 2, "'frame_hw'")
                out.append(camera_from_mujoco(_floats(_key(m, "pos", where), 3, f"{where}'pos'"),
                                              _floats(_key(m, "quat", where), 4, f"{where}'quat'"),
                                              _floats(_key(m, "fovy", where), 1, f"{where}'fovy'")[0], hw))
            else:
                out.append(Camera(*(_key(c, k, where) for k in ("R", "t", "fx", "fy", "cx", "cy"))))
        except ValueError as e:
            msg = str(e)
            raise ValueError(msg if msg.startswith("calibration") else f"calibration: {where[:-1]}: {msg}") from None
    kw = {k: d[k] for k in ("margin", "scale", "smooth", "home") if k in d}
    try:
        return TrackConfig(out, _key(d, "half_extent", ""), z_near=_key(d, "z_near", ""), **kw)
    except ValueError as e:
        msg = str(e)
        raise ValueError(msg if msg.startswith("calibration") else f"calibration: {msg}") from None


def sample_roi_jitter(rng, n_images: int, scale: tuple = (1.0, 1.0), shift: float = 0.0) -> np.ndarray:
    """The jitter of ``n_images`` tracked regions: (n_images, 3) float32 ``[ln s, dy, dx]`` with ``ln s =
    uniform(ln lo, ln hi)`` for ``scale = (lo, hi)`` and ``dy, dx = uniform(-shift, shift)`` in units of the
    region's own size. The same three ``rng.uniform`` draws per image, in the same order, as
    ``resident.sample_rois``: the two leave a generator at the same place."""
    lo, hi, f = float(scale[0]), float(scale[1]), float(shift)
    if n_images < 0 or not (0.0 < lo <= hi) or not f >= 0.0:
        raise ValueError("sample_roi_jitter: n_images >= 0, scale = (lo, hi) with 0 < lo <= hi, shift >= 0")
    low = np.array([math.log(lo), -f, -f], dtype=np.float64)
    high = np.array([math.log(hi), f, f], dtype=np.float64)
    return rng.uniform(low, high, size=(int(n_images), 3)).astype(np.float32)
