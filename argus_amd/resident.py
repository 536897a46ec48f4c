"""Device-resident dataset: decode once, keep the cropped uint8 frames in HBM, build batches on the device.

``CameraCubePoseDataset`` behind a DataLoader opens and decodes ``n_cams`` PNGs, draws the spaghetti arcs
with PIL and pickles the sample across a worker pipe, for every sample of every epoch: about a quarter
of what the fused step consumes. Here every sample is decoded ONCE (through that
same dataset, so the crop, the channel order and the pose conversion are its own), the cropped uint8
frames live in one device tensor, and a batch is one index gather + arc rasterisation launch
(``argus_batch_gather_occlude``, csrc/resident.hip):

    ds = ResidentDataset(cfg_dataset, cfg_aug, train=True, device="cuda")
    loader = ResidentLoader(ds, batch_size=64, shuffle=True, seed=42)
    for epoch in range(n):
        loader.set_epoch(epoch)
        for batch in loader:   # {"images": uint8 cuda (B, 3*n_cams, Hc, Wc), "cube_pose": fp32 cuda (B, 7)}
            ...

The arcs are the project's integer closed form of ``ImageDraw.arc`` (resident.hip; tests/arc_reference.py
restates it and measures its distance from PIL), drawn from the same ``np.random`` distributions in
the same order as ``utils.draw_spaghetti`` (``sample_arcs``), in source-frame coordinates: the reference
draws on the full frame and crops afterwards (data.py:131-137). The photometric augmentations stay where they
are (``DeviceAugmentation``). There is no CPU fallback: a non-cuda device raises.

``ResidentDataset(..., full_frames=True)`` keeps the uncropped frames instead, and ``ResidentLoader(...,
roi_jitter=(lo, hi, shift))`` then builds every camera image from a random region of interest of its frame
(``sample_rois``), occluded first and resampled with the filter ``PoseSession(roi=True)`` deploys, in one launch
(``argus_batch_gather_resample``); the batch gains ``"roi"`` (B, n_cams, 4). Off by default.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import time
from typing import Optional

import numpy as np
import torch

from argus_amd._lib import lib, ptr, stream
from argus_amd.data import AugmentationConfig, CameraCubePoseDataset, CameraCubePoseDatasetConfig, center_crop_slices
from argus_amd.track import TrackConfig, sample_roi_jitter

__all__ = ["ARC_WORDS", "MAX_FRAME", "sample_arcs", "arc_records", "sample_rois", "epoch_indices",
           "ResidentDataset", "ResidentLoader"]

ARC_WORDS = 12      # int32 words of one arc record (argus_arc_record_bytes() / 4)
MAX_FRAME = 8192    # supported source-frame side: keeps every product of the arc tests inside int64
_ONE = 1 << 20
# share of the free device memory (torch.cuda.mem_get_info) the store may take when max_bytes is None:
# the rest is the model's activations, workspaces and the allocator's slack
DEFAULT_FREE_SHARE = 0.5
MAX_DECODE_WORKERS = 16


def _sample_arcs_py(rng, n: int, src_hw: tuple, width_range: tuple) -> np.ndarray:
    """The draws of ``utils.draw_spaghetti``, one call per draw, from any ``rng`` with RandomState's
    ``randint`` / ``uniform``."""
    H, W = src_hw
    out = np.empty((n, 7), dtype=np.int32)
    for i in range(n):
        x0 = rng.randint(0, W)
        y0 = rng.randint(0, H)
        x1 = rng.randint(x0, W)
        y1 = rng.randint(y0, H)
        a0 = rng.randint(0, 360)
        a1 = rng.randint(0, 360)
        w = rng.uniform(*width_range)
        out[i] = (x0, y0, x1, y1, a0, a1, int(w))
    return out


def sample_arcs(rng, n_images: int, n_arcs: int, src_hw: tuple, width_range: tuple = (1.0, 5.0)) -> np.ndarray:
    """``ImageDraw.arc`` parameters of ``n_arcs`` spaghetti arcs for each of ``n_images`` images of a
    ``src_hw`` = (H, W) SOURCE frame: (n_images, n_arcs, 7) int32 [x0, y0, x1, y1, a0, a1, width].

    The draws are those of ``utils.draw_spaghetti`` image after image, in the same order and from the same
    distributions (randint(0, W), randint(0, H), randint(x0, W), randint(y0, H), randint(0, 360) twice,
    int(uniform(*width_range))): with ``rng = np.random.RandomState(s)`` the result is what
    ``draw_spaghetti`` consumes after ``np.random.seed(s)``, and ``rng`` is left where those calls leave it.
    A ``RandomState`` on MT19937 (the default) is advanced by the library's restatement of numpy's legacy
    algorithms (``argus_sample_arc_params``: a Python loop over 7 calls per arc costs about a train step
    per B=64 batch); any other ``rng`` with ``randint`` / ``uniform`` is called draw by draw."""
    H, W = int(src_hw[0]), int(src_hw[1])
    n = int(n_images) * int(n_arcs)
    if n < 0 or H <= 0 or W <= 0:
        raise ValueError("sample_arcs: n_images, n_arcs >= 0 and a positive frame size")
    if n == 0:
        return np.zeros((n_images, n_arcs, 7), dtype=np.int32)
    state = rng.get_state() if isinstance(rng, np.random.RandomState) else None
    if state is None or state[0] != "MT19937":
        return _sample_arcs_py(rng, n, (H, W), width_range).reshape(n_images, n_arcs, 7)
    key = np.ascontiguousarray(state[1], dtype=np.uint32).copy()
    pos = C.c_int(int(state[2]))
    out = np.empty((n, 7), dtype=np.int32)
    lib().sample_arc_params(key.ctypes.data, C.byref(pos), n, H, W, float(width_range[0]), float(width_range[1]),
                            out.ctypes.data)
    rng.set_state((state[0], key, pos.value, state[3], state[4]))
    return out.reshape(n_images, n_arcs, 7)


def arc_records(params: np.ndarray) -> np.ndarray:
    """(..., 7) arc parameters [x0, y0, x1, y1, a0, a1, width] (degrees; PIL's conventions) -> (..., 12)
    int32 device records [x0, y0, x1, y1, width, mode, sx, sy, ex, ey, 0, 0]: mode 0 nothing (a0 == a1)
    / 1 full ellipse (a1 - a0 >= 360) / 2 span <= 180 / 3 span > 180 (a1 < a0 wraps through 0); (sx, sy),
    (ex, ey) = round(2^20 (cos, sin)) of the start / end angle. width < 1 draws as 1, as in PIL."""
    p = np.asarray(params)
    a0, a1 = p[..., 4].astype(np.float64), p[..., 5].astype(np.float64)
    full = (a1 - a0) >= 360.0
    s, e = np.mod(a0, 360.0), np.mod(a1, 360.0)
    span = np.mod(e - s, 360.0)
    mode = np.where(full, 1, np.where(span == 0.0, 0, np.where(span <= 180.0, 2, 3)))
    s, e = np.where(full, 0.0, s), np.where(full, 0.0, e)
    rec = np.zeros(p.shape[:-1] + (ARC_WORDS,), dtype=np.int32)
    rec[..., 0:4] = p[..., 0:4]
    rec[..., 4] = np.maximum(p[..., 6].astype(np.int64), 1)
    rec[..., 5] = mode
    for k, (ang, f) in enumerate(((s, np.cos), (s, np.sin), (e, np.cos), (e, np.sin))):
        rec[..., 6 + k] = np.rint(_ONE * f(np.deg2rad(ang))).astype(np.int32)
    return rec


def epoch_indices(n: int, epoch: int, shuffle: bool, seed: int = 0, rank: int = 0, world: int = 1,
                  drop_last: bool = False) -> list:
    """The sample order of one rank's epoch: ``list(DistributedSampler(range(n), world, rank, shuffle,
    seed=seed, drop_last=drop_last))`` after ``set_epoch(epoch)`` (torch's algorithm: a
    ``torch.randperm`` from a generator seeded ``seed + epoch``, padded by wrapping around (or cut, with
    drop_last) to a multiple of ``world``, then every ``world``-th entry from ``rank``)."""
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside [0, {world})")
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        idx = torch.randperm(n, generator=g).tolist()
    else:
        idx = list(range(n))
    if drop_last and n % world != 0:
        total = math.ceil((n - world) / world) * world
        idx = idx[:total]
    else:
        total = math.ceil(n / world) * world
        pad = total - len(idx)
        if pad > 0:
            idx = idx + (idx * math.ceil(pad / max(1, len(idx))))[:pad]
    return idx[rank:total:world]


def sample_rois(rng, n_images: int, frame_hw: tuple, hw: tuple, crop_origin: tuple, scale: tuple = (1.0, 1.0),
                shift: float = 0.0) -> np.ndarray:
    """Random regions of interest ``(y0, x0, height, width)`` for ``n_images`` camera images of a ``frame_hw``
    frame, resampled to the network's ``hw``: (n_images, 4) float32, every one inside ``pose_session.check_roi``'s
    domain (what ``PoseSession(roi=True)`` serves).

    Per image, three ``rng.uniform`` draws in this order: ``s = exp(uniform(ln lo, ln hi))`` for ``scale = (lo,
    hi)``, clipped to [1/4, 4] and to ``min(Hs / h, Ws / w)`` (the extents are ``(s h, s w)``: the aspect ratio is
    kept); ``dy = uniform(-shift, shift) * h`` and ``dx = uniform(-shift, shift) * w``, added to the center crop's
    center (``crop_origin`` + ``hw`` / 2). The origin is clipped to [0, S - extent] per axis, and once more after
    rounding to float32. ``scale=(1, 1), shift=0`` is the center crop exactly."""
    Hs, Ws, h, w = int(frame_hw[0]), int(frame_hw[1]), int(hw[0]), int(hw[1])
    lo, hi, f = float(scale[0]), float(scale[1]), float(shift)
    if n_images < 0 or h <= 0 or w <= 0 or h > Hs or w > Ws:
        raise ValueError("sample_rois: n_images >= 0 and 0 < hw <= frame_hw")
    if not (0.0 < lo <= hi) or not f >= 0.0:
        raise ValueError("sample_rois: scale = (lo, hi) with 0 < lo <= hi, shift >= 0")
    n = int(n_images)
    low = np.array([math.log(lo), -f, -f], dtype=np.float64)
    high = np.array([math.log(hi), f, f], dtype=np.float64)
    u = rng.uniform(low, high, size=(n, 3))  # row-major: image after image, s then dy then dx
    s = np.clip(np.exp(u[:, 0]), 0.25, min(4.0, Hs / h, Ws / w))
    size = np.array([h, w], dtype=np.float64)
    frame = np.array([Hs, Ws], dtype=np.float64)
    ext = np.minimum(s[:, None] * size, frame)
    center = np.array(crop_origin, dtype=np.float64) + size / 2 + u[:, 1:] * size
    org = np.clip(center - ext / 2, 0.0, frame - ext)
    e32 = ext.astype(np.float32)
    lim = frame - e32.astype(np.float64)  # >= 0: a float32 rounding cannot pass the integer S
    o32 = np.clip(org, 0.0, lim).astype(np.float32)
    o32 = np.where(o32.astype(np.float64) > lim, np.nextafter(o32, np.float32(-1.0)), o32)
    return np.concatenate([np.maximum(o32, np.float32(0.0)), e32], axis=1).astype(np.float32)


def _require_cuda(device, what: str) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"argus_amd.{what} runs only on the MI355X HIP path: pass a cuda device (there is no "
                           "CPU fallback; the DataLoader path is CameraCubePoseDataset)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class ResidentDataset:
    """Every sample of a ``CameraCubePoseDataset`` split, decoded once and kept on ``device``:
    ``images`` (n, 3*n_cams, Hc, Wc) uint8 (center-cropped, no arcs) and ``poses`` (n, 7) fp32.

    Decoding goes through ``CameraCubePoseDataset(uint8=True)`` with the spaghetti forced off, in at most 16
    spawned (never forked: ``train.make_loaders``) DataLoader workers. ``src_hw`` is the frame size on disk
    and ``crop_origin`` the crop's (y0, x0) in it (``center_crop_slices``): the arcs are drawn in source-frame
    coordinates. Raises before allocating when the store would exceed ``max_bytes`` (default:
    ``DEFAULT_FREE_SHARE`` of the free device memory). ``dataset`` overrides the decoded dataset (any
    map-style dataset of the same samples, e.g. a ``Subset``); ``ingest_seconds`` is the one-time cost.

    ``full_frames=True`` keeps the UNCROPPED frames instead, ``images`` (n, 3*n_cams, Hs, Ws), decoded through
    ``CameraCubePoseDataset`` with the crop disabled (a ``dataset`` override must then yield uncropped samples);
    ``crop_hw`` and ``crop_origin`` keep their meaning (the network's size and the center crop's origin), and the
    memory check uses the stored shape (a 376 x 672 two-camera sample is 1.5 MB)."""

    def __init__(self, cfg_dataset: CameraCubePoseDatasetConfig, cfg_aug: Optional[AugmentationConfig] = None,
                 train: bool = True, device="cuda", max_bytes: Optional[int] = None, num_workers: int = -1,
                 dataset=None, full_frames: bool = False) -> None:
        self.device = _require_cuda(device, "ResidentDataset")
        self.cfg_aug = cfg_aug
        self.train = train
        self.full_frames = bool(full_frames)
        base = CameraCubePoseDataset(cfg_dataset, cfg_aug=None, train=train, uint8=True)  # cfg_aug None: no arcs
        decode = base if dataset is None else dataset
        if self.full_frames and dataset is None:  # the same samples with the crop disabled
            decode = CameraCubePoseDataset(dataclasses.replace(cfg_dataset, center_crop=None), cfg_aug=None,
                                           train=train, uint8=True)
        n = len(decode)
        if n == 0:
            raise ValueError("ResidentDataset: the split has no samples")
        self.n_cams = base.n_cams
        from PIL import Image

        with Image.open(f"{base.dataset_path}/{base.img_stems[0]}_a.png") as im:
            self.src_hw = (im.height, im.width)
        crop = tuple(base.center_crop) if base.center_crop else self.src_hw
        if crop == self.src_hw:
            self.crop_origin = (0, 0)
        else:
            ys, xs = center_crop_slices(self.src_hw, crop)
            self.crop_origin = (ys.start, xs.start)
        self.crop_hw = crop
        if max(self.src_hw) > MAX_FRAME:
            raise ValueError(f"ResidentDataset: frames of {self.src_hw} exceed the supported {MAX_FRAME} a side")
        stored = self.src_hw if self.full_frames else crop
        need = n * 3 * self.n_cams * stored[0] * stored[1]
        with torch.cuda.device(self.device):
            limit = int(DEFAULT_FREE_SHARE * torch.cuda.mem_get_info()[0]) if max_bytes is None else int(max_bytes)
        if need > limit:
            raise MemoryError(f"ResidentDataset: {n} samples of {3 * self.n_cams}x{stored[0]}x{stored[1]} uint8 need "
                              f"{need} bytes on the device, over the limit of {limit}; use the DataLoader path "
                              "(CameraCubePoseDataset; train without --resident-dataset) or raise max_bytes")
        t0 = time.perf_counter()
        self.images = torch.empty((n, 3 * self.n_cams, stored[0], stored[1]), dtype=torch.uint8, device=self.device)
        self.poses = torch.empty((n, 7), dtype=torch.float32, device=self.device)
        nw = MAX_DECODE_WORKERS if num_workers < 0 else min(int(num_workers), MAX_DECODE_WORKERS)
        nw = min(nw, n // 64)  # no more workers than decode batches: a spawn costs more than a small split
        kw = dict(batch_size=min(64, n), shuffle=False, num_workers=nw)
        if nw > 0:
            kw["multiprocessing_context"] = "spawn"
        at = 0
        for batch in torch.utils.data.DataLoader(decode, **kw):
            b = batch["images"].shape[0]
            if tuple(batch["images"].shape[1:]) != tuple(self.images.shape[1:]):
                raise ValueError(f"ResidentDataset: sample shape {tuple(batch['images'].shape[1:])} != "
                                 f"{tuple(self.images.shape[1:])} (frames of one size are required)")
            self.images[at:at + b].copy_(batch["images"])
            self.poses[at:at + b].copy_(batch["cube_pose"])
            at += b
        torch.cuda.synchronize(self.device)
        self.ingest_seconds = time.perf_counter() - t0

    def __len__(self) -> int:
        return self.images.shape[0]

    @property
    def num_spaghetti(self) -> int:
        return 0 if self.cfg_aug is None else max(0, int(self.cfg_aug.num_spaghetti))


class ResidentLoader:
    """Batches of a ``ResidentDataset``, built on the device. Per batch: one host draw of the arc records
    (``sample_arcs`` from a ``RandomState`` seeded ``arc_seed + 1000003 * epoch + rank`` at the start of each
    pass, so an epoch is reproducible and epochs and ranks differ; ``arc_seed`` defaults to ``seed``), one non-blocking copy from a pinned buffer
    (the batch's int64 indices followed by its records) and one launch. The sample order is
    ``epoch_indices`` (DistributedSampler's; ``drop_last`` is the sampler's, the last partial batch is
    yielded as the DataLoader's default does). Arcs are drawn for train and validation alike, as
    ``data.py`` does; ``num_spaghetti == 0`` or ``cfg_aug is None`` launches with no arcs.

    A ``ResidentDataset(full_frames=True)`` is served by ``argus_batch_gather_resample`` instead: every camera
    image is a region of interest ``(y0, x0, height, width)`` of its uncropped frame, occluded in source-frame
    coordinates and resampled to ``crop_hw`` with the filter ``PoseSession(roi=True)`` deploys. The regions are the
    center crop (the same bytes as the cropped store's launch) unless ``roi_jitter = (lo, hi, shift)`` draws them
    per batch (``sample_rois``) from a generator of their own, seeded ``roi_seed + 1000003 * epoch + rank``
    (``roi_seed`` defaults to ``arc_seed + 7919``), so the arc stream is the same with the jitter on or off. The
    regions travel in the pinned slot between the indices and the records, and the batch gains ``"roi"``:
    (B, n_cams, 4) fp32 on the device. ``roi_jitter`` on a cropped store raises ``ValueError``.

    ``roi_track=TrackConfig(...)`` (full frames only, as ``roi_jitter``) aims every region at the sample's labelled
    cube instead: one ``argus_roi_from_pose`` launch over ``ds.poses`` and the batch's device indices, with ``smooth``
    forced to 1 and the center crop as ``home``, writes the buffer the resample launch then reads: the arithmetic of
    ``PoseSession(track=...)``, so training sees what the tracker will show. With ``roi_jitter`` as well the host
    draws ``track.sample_roi_jitter`` (the three draws of ``sample_rois``, from the same generator) and its three
    floats per image travel in the regions' slot; the kernel applies them around the cube. ``batch["roi"]`` is the
    kernel's output and ``batch["roi_valid"]`` (B, n_cams) int32 says where the cube was in view (0: ``home``).

    The pinned buffers are a ring of ``RING`` slots, each guarded by an event, so the host draw of the next
    batches overlaps the device's work on the earlier ones. Yielded tensors are fresh."""

    RING = 4

    def __init__(self, ds: ResidentDataset, batch_size: int, shuffle: bool = False, seed: int = 0, rank: int = 0,
                 world: int = 1, drop_last: bool = False, arc_seed: Optional[int] = None,
                 roi_jitter: Optional[tuple] = None, roi_seed: Optional[int] = None,
                 roi_track: Optional[TrackConfig] = None) -> None:
        if not isinstance(ds, ResidentDataset):
            raise TypeError("ResidentLoader needs a ResidentDataset")
        _require_cuda(ds.device, "ResidentLoader")
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        self.full_frames = bool(getattr(ds, "full_frames", False))
        if roi_track is not None:
            if not self.full_frames:
                raise ValueError("roi_track needs a ResidentDataset(full_frames=True): a cropped store has "
                                 "nothing outside the center crop to resample from")
            if not isinstance(roi_track, TrackConfig):
                raise ValueError(f"roi_track: expected a TrackConfig, got {type(roi_track).__name__}")
            if len(roi_track.cameras) != ds.n_cams:
                raise ValueError(f"roi_track: {len(roi_track.cameras)} cameras for a dataset of {ds.n_cams}")
        self.roi_track = roi_track
        if roi_jitter is not None:
            if not self.full_frames:
                raise ValueError("roi_jitter needs a ResidentDataset(full_frames=True): a cropped store has "
                                 "nothing outside the center crop to resample from")
            if len(roi_jitter) != 3:
                raise ValueError("roi_jitter = (lo, hi, shift)")
            roi_jitter = tuple(float(v) for v in roi_jitter)
            if not (0.0 < roi_jitter[0] <= roi_jitter[1]) or not roi_jitter[2] >= 0.0:
                raise ValueError("roi_jitter = (lo, hi, shift) with 0 < lo <= hi and shift >= 0")
        self.roi_jitter = roi_jitter
        self.ds, self.batch_size, self.shuffle, self.seed = ds, int(batch_size), bool(shuffle), int(seed)
        self.rank, self.world, self.drop_last = int(rank), int(world), bool(drop_last)
        self.arc_seed = self.seed if arc_seed is None else int(arc_seed)
        self.epoch = 0
        self.n_arcs = ds.num_spaghetti
        if lib().dll.argus_arc_record_bytes() != 4 * ARC_WORDS:
            raise RuntimeError("libargus_hip arc record size != 12 int32")
        # the regions' own generator: the arc stream is the same with the jitter on or off
        self.roi_seed = self.arc_seed + 7919 if roi_seed is None else int(roi_seed)
        self._roi_words = 4 * ds.n_cams if self.full_frames else 0  # per sample, fp32 words in the int32 slot
        words = self.batch_size * (2 + self._roi_words + ds.n_cams * self.n_arcs * ARC_WORDS)
        self._host = [torch.empty(words, dtype=torch.int32).pin_memory() for _ in range(self.RING)]
        self._events = [None] * self.RING
        self._slot = 0
        if roi_track is not None:  # uploaded once: the cameras, the home region (the center crop), the settings
            with torch.cuda.device(ds.device):
                self._cameras = torch.from_numpy(roi_track.camera_words()).to(ds.device)
                home = torch.tensor([*ds.crop_origin, *ds.crop_hw], dtype=torch.float32)
                self._home = home.repeat(self.batch_size * ds.n_cams, 1).to(ds.device)
            self._track_cfg = roi_track.struct(smooth=1.0)  # a batch has no previous frame

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def indices(self) -> list:
        return epoch_indices(len(self.ds), self.epoch, self.shuffle, self.seed, self.rank, self.world, self.drop_last)

    def __len__(self) -> int:
        return -(-len(self.indices()) // self.batch_size)

    def host_generators(self) -> tuple:
        """(arc generator, region generator or None) of the current epoch: ``RandomState``s seeded ``arc_seed`` /
        ``roi_seed`` ``+ 1000003 * epoch + rank``. Two streams, so the arcs do not depend on the jitter."""
        off = 1000003 * self.epoch + self.rank
        rng = np.random.RandomState((self.arc_seed + off) % (1 << 32))
        roi_rng = None if self.roi_jitter is None else np.random.RandomState((self.roi_seed + off) % (1 << 32))
        return rng, roi_rng

    def fill_slot(self, hv: np.ndarray, idx: list, rng, roi_rng) -> int:
        """One batch's host words into the int32 array ``hv``: the int64 sample indices, the regions of a
        full-frame store ((len(idx) * n_cams, 4) fp32: ``sample_rois`` from ``roi_rng``, the center crop when it is
        None), the arc records from ``rng``. Returns the word offset of the records."""
        ds, b = self.ds, len(idx)
        a_at = b * (2 + self._roi_words)
        hv[:2 * b].view(np.int64)[:] = idx
        if self.full_frames:
            hr = hv[2 * b:a_at].view(np.float32).reshape(b * ds.n_cams, 4)
            if roi_rng is not None and self.roi_track is not None:
                # the same slot (its stride kept): 3 floats an image, packed; the tail of the slot is not read
                hr.reshape(-1)[:3 * b * ds.n_cams] = sample_roi_jitter(roi_rng, b * ds.n_cams, self.roi_jitter[:2],
                                                                      self.roi_jitter[2]).reshape(-1)
            elif roi_rng is None:
                hr[:] = np.array([*ds.crop_origin, *ds.crop_hw], dtype=np.float32)
            else:
                hr[:] = sample_rois(roi_rng, b * ds.n_cams, ds.src_hw, ds.crop_hw, ds.crop_origin,
                                    self.roi_jitter[:2], self.roi_jitter[2])
        if self.n_arcs > 0:
            rec = arc_records(sample_arcs(rng, b * ds.n_cams, self.n_arcs, ds.src_hw))
            hv[a_at:a_at + rec.size] = rec.reshape(-1)
        return a_at

    def __iter__(self):
        ds = self.ds
        order = self.indices()
        rng, roi_rng = self.host_generators()
        hc, wc = ds.crop_hw
        with torch.cuda.device(ds.device):
            for at in range(0, len(order), self.batch_size):
                idx = order[at:at + self.batch_size]
                b = len(idx)
                slot = self._slot
                self._slot = (slot + 1) % self.RING
                if self._events[slot] is not None:
                    self._events[slot].synchronize()  # the copy that last read this slot is done
                # indices, then the regions (full frames), then the arc records
                used = b * (2 + self._roi_words + ds.n_cams * self.n_arcs * ARC_WORDS)
                host = self._host[slot][:used]
                a_at = self.fill_slot(host.numpy(), idx, rng, roi_rng)
                dev = host.to(ds.device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                self._events[slot] = ev
                index = dev[:2 * b].view(torch.int64)
                arcs = dev.data_ptr() + 4 * a_at if self.n_arcs > 0 else None
                images = torch.empty((b, 3 * ds.n_cams, hc, wc), dtype=torch.uint8, device=ds.device)
                batch = {"images": images, "cube_pose": ds.poses.index_select(0, index)}
                if self.full_frames:  # the uncropped store: every image through its region (one launch)
                    roi = dev[2 * b:a_at].view(torch.float32).view(b, ds.n_cams, 4)
                    if self.roi_track is not None:  # aimed at the labelled cube: one launch in front
                        jit = ptr(roi) if self.roi_jitter is not None else None  # the slot holds (b * n_cams, 3)
                        roi = torch.empty((b, ds.n_cams, 4), dtype=torch.float32, device=ds.device)
                        valid = torch.empty((b, ds.n_cams), dtype=torch.int32, device=ds.device)
                        lib().roi_from_pose(b, ds.n_cams, ds.src_hw[0], ds.src_hw[1], hc, wc, ptr(ds.poses), len(ds),
                                            ptr(index), ptr(self._cameras), C.byref(self._track_cfg), jit,
                                            ptr(self._home), ptr(roi), None, ptr(valid), stream())
                        batch["roi_valid"] = valid
                    lib().batch_gather_resample(b, ds.n_cams, ds.src_hw[0], ds.src_hw[1], hc, wc, ptr(ds.images),
                                                len(ds), ptr(index), ptr(roi), arcs, self.n_arcs, ptr(images), stream())
                    batch["roi"] = roi
                else:
                    lib().batch_gather_occlude(b, ds.n_cams, hc, wc, ptr(ds.images), len(ds), ptr(index), arcs,
                                               self.n_arcs, ds.crop_origin[0], ds.crop_origin[1], ptr(images), stream())
                yield batch
