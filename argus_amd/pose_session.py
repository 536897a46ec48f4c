"""Frozen pose session: camera frames in, SE(3) pose out, in one replayed graph.

``PoseSession`` is an ``InferenceSession`` whose two ends are fused for the deployment case (one pose per
replay, ``batch * n_cams <= 16``, bf16 or fp16):

- front: ``argus_stem_infer`` reads the frames as they arrive (planar ``(B, 3*n_cams, Hs, Ws)`` or interleaved
  ``(B, n_cams, Hs, Ws, 3)``, uint8 or fp32, center-cropped on the fly) and writes the pooled stem output in one
  launch: no NHWC4 copy, no stem output round trip, no argmax, no host-side transpose / crop
  (argus/validate_real.py:58-75);
- back: ``argus_pool_fc_gelu`` + ``argus_pose_tail`` replace avg-pool, fc, GELU, the three MLP GEMMs and the
  se(3) exponential, so the replay itself ends in the pose (``get_pose``, argus/utils.py:179-189).

``roi=True`` gives every camera image a region of interest in source pixels (``set_roi`` / ``pose(frames,
roi=...)``), resampled to ``hw`` inside the stem launch (``argus_stem_infer_roi``) from a device buffer that
every replay reads: frames of any resolution, a cube anywhere in them, a tracker that follows it, without a
resize in front of the graph and without a re-capture.

``track=TrackConfig(...)`` closes the loop on the device: the graph ends with ``argus_roi_from_pose``, which writes
the region the next replay reads from the pose this one produced (argus_amd/track.py; 56 launches).

The graph is stem-infer, the 52 folded convs, pool-fc-gelu, pose-tail: 55 launches where the parent session has
61 in the graph and two more behind it. ``fused_stem=False`` / ``fused_head=False`` put the parent's launches
back for that end (A/B timing; bisecting a mismatch to one end). Everything else (``refresh()``, the fp16 range
check, snapshot semantics) is inherited.
"""
from __future__ import annotations

import ctypes as C

import torch

from argus_amd._lib import FrameSrc, ptr, stream
from argus_amd.data import center_crop_slices
from argus_amd.infer import InferenceSession, _require_cuda
from argus_amd.models import NCameraCNN
from argus_amd.track import TrackConfig
from argus_amd.utils import se3_exp

MAX_ROWS = 16  # argus_pool_fc_gelu / argus_pose_tail serve batch * n_cams <= 16


def check_roi(roi, frame_hw: tuple, hw: tuple) -> torch.Tensor:
    """``roi`` as the float32 CPU tensor the device will read, or ValueError naming the rule it breaks.

    ``roi``: ``(4,)`` or ``(batch, n_cams, 4)`` host values ``(y0, x0, height, width)`` in pixels of a
    ``frame_hw`` frame, fractional values allowed. Served (include/argus_hip.h, argus_stem_infer_roi): finite; per
    axis ``0 <= origin``, ``origin + extent <= frame``, ``n / 4 <= extent <= 4 n`` for the output length ``n`` of
    ``hw``. The rules are applied to the values rounded to float32. Needs no GPU."""
    t = torch.as_tensor(roi, dtype=torch.float64, device="cpu")
    if t.shape[-1:] != (4,) or t.dim() not in (1, 3):
        raise ValueError(f"roi shape: expected (4,) or (batch, n_cams, 4) values (y0, x0, height, width), got "
                         f"{tuple(t.shape)}")
    t = t.to(torch.float32)
    if not bool(torch.isfinite(t).all()):
        raise ValueError("roi finite: every value must be finite")
    v = t.double().reshape(-1, 4)
    for axis, name in ((0, "y"), (1, "x")):
        o, e, S, n = v[:, axis], v[:, 2 + axis], int(frame_hw[axis]), int(hw[axis])
        if bool((o < 0).any()):
            raise ValueError(f"roi origin: {name}0 = {o.min().item()} is negative")
        if bool((e < n / 4).any()) or bool((e > 4 * n).any()):
            bad = e[(e < n / 4) | (e > 4 * n)][0].item()
            raise ValueError(f"roi scale: the {name} extent {bad} is outside [{n / 4}, {4 * n}] (a quarter to four "
                             f"times the network's {n})")
        if bool((o + e > S).any()):
            raise ValueError(f"roi inside the frame: {name}0 + extent = {(o + e).max().item()} exceeds the frame's {S}")
    return t


class PoseSession(InferenceSession):
    """``session.pose(frames) -> (batch, 7)`` and ``session(frames) -> (batch, 6)`` from one replay.

    ``hw``: the size the network sees; ``frame_hw``: the size of the frames handed in (default ``hw``), center
    cropped to ``hw`` as kornia does (``data.center_crop_slices``). ``layout``: "chw" for ``(B, 3*n_cams, Hs,
    Ws)``, "hwc" for ``(B, n_cams, Hs, Ws, 3)``. ``session.frames[dtype]`` are the static input buffers (uint8 and
    float32): ``pose(None)`` replays on what the caller wrote there.

    ``roi=True``: each camera image has a region of interest ``(y0, x0, height, width)`` in frame pixels (see
    ``check_roi``), resampled to ``hw`` with the antialiased triangle filter of ``F.interpolate(mode="bilinear",
    antialias=True)``. It starts as the center crop at unit scale (the bits of ``roi=False``) and is changed by
    ``set_roi`` or ``pose(frames, roi=...)`` between replays: the graph reads it from device memory.

    ``track=TrackConfig(...)`` (implies ``roi=True``; needs ``fused_head``): the forward ends with
    ``argus_roi_from_pose`` on the pose it just wrote, in place on that buffer, so every replay aims the region the
    next one reads at the cube: a closed-loop tracker with no host step between replays. An image whose pose puts a
    corner behind (or too near) its camera, or is not finite, goes back to ``home``. ``last_roi`` / ``roi_valid``
    report the region the last frame was seen through and whether the new one was aimed; ``reset_roi()`` returns to
    ``home``; ``set_roi`` still overrides (an external detector re-acquiring the cube)."""

    def __init__(self, model: NCameraCNN, batch: int, hw: tuple, compute_dtype: str | None = None,
                 graph: bool = True, frame_hw: tuple | None = None, layout: str = "chw", fused_stem: bool = True,
                 fused_head: bool = True, roi: bool = False, track: TrackConfig | None = None):
        self.roi_frame_hw = getattr(model, "roi_frame_hw", None)
        if self.roi_frame_hw is not None:  # a model conditioned on the region each camera saw
            if not roi and track is None:
                raise ValueError(f"PoseSession: the model is built with roi_frame_hw = {self.roi_frame_hw}, its head "
                                 f"reads the region of interest: pass roi=True (or track=)")
            fhw = tuple(int(v) for v in (hw if frame_hw is None else frame_hw))
            if fhw != self.roi_frame_hw:
                raise ValueError(f"PoseSession: frame_hw {fhw} is not the model's roi_frame_hw {self.roi_frame_hw}: "
                                 f"the region features are measured in that frame")
        if track is not None:
            if not isinstance(track, TrackConfig):
                raise ValueError(f"PoseSession track: expected a TrackConfig, got {type(track).__name__}")
            if not fused_head:
                raise ValueError("PoseSession(track=...) needs fused_head=True: the pose has to be produced inside "
                                 "the graph for the graph to aim the next region from it")
            if len(track.cameras) != model.n_cams:
                raise ValueError(f"PoseSession track: {len(track.cameras)} cameras for a model of {model.n_cams}")
            roi = True
        self.track = track
        _require_cuda(model)
        dtype = model.compute_dtype if compute_dtype is None else compute_dtype
        if dtype not in ("bf16", "fp16"):
            raise ValueError(f"PoseSession serves compute_dtype 'bf16' and 'fp16', got {dtype!r}: use "
                             f"InferenceSession for 'fp32'")
        if int(batch) * model.n_cams > MAX_ROWS:
            raise ValueError(f"PoseSession serves batch * n_cams <= {MAX_ROWS} (the deployment path), got "
                             f"{int(batch) * model.n_cams}: use InferenceSession for larger batches")
        if layout not in ("chw", "hwc"):
            raise ValueError(f"PoseSession layout is 'chw' or 'hwc', got {layout!r}")
        self.frame_hw = (int(hw[0]), int(hw[1])) if frame_hw is None else (int(frame_hw[0]), int(frame_hw[1]))
        self.layout, self.fused_stem, self.fused_head = layout, bool(fused_stem), bool(fused_head)
        self.has_roi = bool(roi)
        if self.frame_hw[0] < hw[0] or self.frame_hw[1] < hw[1]:
            raise ValueError(f"PoseSession: frame_hw {self.frame_hw} is smaller than hw {tuple(hw)}")
        if not self.fused_stem and not self.has_roi and (layout != "chw" or self.frame_hw != (int(hw[0]), int(hw[1]))):
            raise ValueError("PoseSession(fused_stem=False) takes pre-cropped 'chw' frames only: the 'hwc' layout "
                             "and the crop are argus_stem_infer's")
        ys, xs = center_crop_slices(self.frame_hw, hw)
        self.crop = (ys.start, xs.start)
        super().__init__(model, batch, hw, dtype, graph)

    # ------------------------------------------------------------------ construction
    _serves_roi = True

    def _plan(self) -> None:
        super()._plan()
        self.launches_per_forward = (1 if self.fused_stem else 3) + len(self.convs) + (2 if self.fused_head else 6)
        if self.roi_frame_hw is not None and not self.fused_head:
            self.launches_per_forward += 1  # argus_roi_embed behind output_mlp.0's GEMM
        if self.track is not None:
            self.launches_per_forward += 1  # argus_roi_from_pose behind argus_pose_tail

    def _alloc_activations(self, max_elems: int) -> None:
        if not self.fused_stem:
            return super()._alloc_activations(max_elems)
        # no NHWC4 copy, no stem output, no argmax: the pooled stem output is the first block's input
        N, (H2, W2) = self.N, self.pool_hw
        blocks = max(N * H2 * W2 * 64, self._block_elems)
        self.pool = [self._empty(blocks) for _ in range(5)]
        self.ws = torch.zeros(max(max(cv.ws_bytes for cv in self.convs.values()), 16), dtype=torch.uint8,
                              device=self.device)
        self.activation_bytes = sum(t.numel() * t.element_size() for t in self.pool)

    def _plan_convs(self) -> int:
        self._block_elems = super()._plan_convs()
        return self._block_elems

    def _alloc_head(self) -> None:
        super()._alloc_head()
        L, N, B, D = self.L, self.N, self.batch, self.n_cams * self.rdim
        self.pose_out = self._empty(B, 7, dtype=torch.float32)
        # ticket words zeroed here once; every launch leaves them zero
        self.fc_ws = torch.zeros(L.dll.argus_pool_fc_gelu_workspace_bytes(N, 2048, self.rdim), dtype=torch.uint8,
                                 device=self.device)
        self.tail_ws = torch.zeros(L.dll.argus_pose_tail_workspace_bytes(B, D), dtype=torch.uint8, device=self.device)
        if not self.fc_ws.numel() or not self.tail_ws.numel():
            raise RuntimeError(f"argus_pool_fc_gelu / argus_pose_tail do not serve rows {N}, rdim {self.rdim}")

    def _alloc_inputs(self) -> None:
        B, n, (Hs, Ws) = self.batch, self.n_cams, self.frame_hw
        shape = (B, 3 * n, Hs, Ws) if self.layout == "chw" else (B, n, Hs, Ws, 3)
        self.frames = {dt: self._empty(*shape, dtype=dt) for dt in (torch.float32, torch.uint8)}
        self.static_in = self.frames
        self._src = {}
        for dt, t in self.frames.items():
            st = (3 * Hs * Ws, Hs * Ws, Ws, 1) if self.layout == "chw" else (3 * Hs * Ws, 1, 3 * Ws, 3)
            # with a region of interest the origin is in the region, not in the descriptor
            self._src[dt] = FrameSrc(ptr(t), 0 if dt == torch.uint8 else 1, *st, Hs, Ws,
                                     *((0, 0) if self.has_roi else self.crop))
        if self.has_roi:
            center = torch.tensor([*self.crop, *self.hw], dtype=torch.float32)
            self._roi = center.repeat(self.N, 1).to(self.device)  # (batch * n_cams, 4): what every replay reads
        if self.track is not None:
            tr = self.track
            home = center if tr.home is None else check_roi(tr.home, self.frame_hw, self.hw)
            if home.dim() == 3 and tuple(home.shape) != (B, n, 4):
                raise ValueError(f"TrackConfig home: expected (4,) or {(B, n, 4)}, got {tuple(home.shape)}")
            self._home = home.expand(B, n, 4).reshape(self.N, 4).contiguous().to(self.device)
            self._roi.copy_(self._home)
            self._cameras = torch.from_numpy(tr.camera_words()).to(self.device)  # (n_cams, 16), uploaded once
            self._track_cfg = tr.struct()
            # what argus_roi_from_pose reports: the region the frame just processed was seen through, its validity
            self._roi_used = self._home.clone()
            self._roi_valid = torch.ones(self.N, dtype=torch.int32, device=self.device)

    # ------------------------------------------------------------------ region of interest
    @property
    def roi(self) -> torch.Tensor | None:
        """The regions the next replay resamples: a (batch, n_cams, 4) float32 CPU tensor (None without ``roi``)."""
        return self._roi.view(self.batch, self.n_cams, 4).cpu() if self.has_roi else None

    def set_roi(self, roi) -> None:
        """Validate ``roi`` (``check_roi``: ``(4,)`` for every image, or ``(batch, n_cams, 4)``) and copy it into
        the device buffer the captured graph reads: the next replay uses it, nothing is re-captured."""
        if not self.has_roi:
            raise ValueError("PoseSession.set_roi: the session was built without roi=True")
        t = check_roi(roi, self.frame_hw, self.hw)
        if t.dim() == 3 and tuple(t.shape) != (self.batch, self.n_cams, 4):
            raise ValueError(f"roi shape: expected (4,) or {(self.batch, self.n_cams, 4)}, got {tuple(t.shape)}")
        with torch.cuda.device(self.device):
            self._roi.copy_(t.expand(self.batch, self.n_cams, 4).reshape(self.N, 4))

    def reset_roi(self) -> None:
        """Back to ``home`` (the center crop unless ``TrackConfig.home`` says otherwise): the next replay reads it."""
        if self.track is None:
            raise ValueError("PoseSession.reset_roi: the session was built without track=")
        with torch.cuda.device(self.device):
            self._roi.copy_(self._home)

    @property
    def last_roi(self) -> torch.Tensor | None:
        """The regions the LAST replay resampled its frames through: (batch, n_cams, 4) float32 on the CPU (None
        without ``track``; ``home`` before the first replay). ``roi`` is what the next one will read."""
        return None if self.track is None else self._roi_used.view(self.batch, self.n_cams, 4).cpu()

    @property
    def roi_valid(self) -> torch.Tensor | None:
        """(batch, n_cams) int32 on the CPU: 1 where the last replay's pose put the whole cube in front of the
        camera and ``roi`` was aimed at it, 0 where ``roi`` fell back to ``home`` (None without ``track``)."""
        return None if self.track is None else self._roi_valid.view(self.batch, self.n_cams).cpu()

    # ------------------------------------------------------------------ forward
    def _to_nhwc4(self, x: torch.Tensor, s) -> None:
        if not self.has_roi:
            return super()._to_nhwc4(x, s)
        H, W = self.hw
        self.L.frames_resample(self.dt, self.N, H, W, C.byref(self._src[x.dtype]), ptr(self._roi), ptr(self.x0), s)

    def _forward(self, x: torch.Tensor, probe=None) -> torch.Tensor:
        """The launches of one forward from the static frame buffer ``x`` into self.pred and self.pose_out."""
        if not self.fused_stem:
            return super()._forward(x, probe)
        L, dt, s, N = self.L, self.dt, stream(), self.N
        H, W = self.hw
        _, h, blocks = self._buffers()
        if self.has_roi:
            L.stem_infer_roi(dt, N, H, W, 64, C.byref(self._src[x.dtype]), ptr(self._roi), ptr(self.stem_wf),
                             ptr(self.stem_coef[0]), ptr(self.stem_coef[1]), ptr(h), s)
        else:
            L.stem_infer(dt, N, H, W, 64, C.byref(self._src[x.dtype]), ptr(self.stem_wf), ptr(self.stem_coef[0]),
                         ptr(self.stem_coef[1]), ptr(h), s)
        if probe is not None:
            probe(h, N * self.pool_hw[0] * self.pool_hw[1] * 64)
        for (c1, c2, c3, ds), (a1, a2, out, yd) in zip(self.schedule, blocks):
            self._conv(c1, h, a1, None, 1, s, probe)
            self._conv(c2, a1, a2, None, 1, s, probe)
            res = h
            if ds is not None:
                self._conv(ds, h, yd, None, 0, s, probe)
                res = yd
            self._conv(c3, a2, out, res, 1, s, probe)
            h = out
        return self._head(h)

    def _mlp0(self, ws, wsn, s) -> None:
        """``fused_head=False``: output_mlp.0 of a conditioned model is the GEMM with the bias epilogue, then
        argus_roi_embed on the regions the stem read in this forward (the second implementation the fused tail is
        compared with)."""
        if self.roi_frame_hw is None:
            return super()._mlp0(ws, wsn, s)
        L, B, D, hd = self.L, self.batch, self.n_cams * self.rdim, self.head
        L.gemm_f32(B, 128, D, ptr(self.g0), D, 0, ptr(hd["output_mlp.0", "weight"]), D, 1, ptr(self.h1), 128,
                   ptr(hd["output_mlp.0", "bias"]), 1, None, ws, wsn, s)
        L.roi_embed(B, self.n_cams, *self.frame_hw, *self.hw, ptr(self._roi), ptr(hd["roi_embed", "weight"]),
                    ptr(self.h1), ptr(self.g1), None, s)

    def _head(self, h: torch.Tensor) -> torch.Tensor:
        if not self.fused_head:
            return super()._head(h)
        L, s, N, B = self.L, stream(), self.N, self.batch
        hf, wf = self.final_hw
        hd, D = self.head, self.n_cams * self.rdim
        L.pool_fc_gelu(self.dt, N, hf * wf, 2048, ptr(h), ptr(hd["resnet.fc", "weight"]), ptr(hd["resnet.fc", "bias"]),
                       self.rdim, ptr(self.g0), ptr(self.fc_ws), self.fc_ws.numel(), s)
        mlp = (ptr(hd["output_mlp.0", "weight"]), ptr(hd["output_mlp.0", "bias"]),
               ptr(hd["output_mlp.2", "weight"]), ptr(hd["output_mlp.2", "bias"]),
               ptr(hd["output_mlp.4", "weight"]), ptr(hd["output_mlp.4", "bias"]), ptr(self.pred), ptr(self.pose_out), 0)
        if self.roi_frame_hw is None:
            L.pose_tail(B, D, ptr(self.g0), *mlp, ptr(self.tail_ws), self.tail_ws.numel(), s)
        else:  # self._roi: the regions the stem read in this forward; argus_roi_from_pose overwrites them BEHIND this
            L.pose_tail_roi(B, D, ptr(self.g0), *mlp, self.n_cams, *self.frame_hw, *self.hw, ptr(self._roi),
                            ptr(hd["roi_embed", "weight"]), ptr(self.tail_ws), self.tail_ws.numel(), s)
        if self.track is not None:  # the region the NEXT forward reads, in place: the tracker's only step
            L.roi_from_pose(B, self.n_cams, *self.frame_hw, *self.hw, ptr(self.pose_out), B, None, ptr(self._cameras),
                            C.byref(self._track_cfg), None, ptr(self._home), ptr(self._roi), ptr(self._roi_used),
                            ptr(self._roi_valid), s)
        return self.pred

    def _check_images(self, images, who: str) -> None:
        want = tuple(self.frames[torch.uint8].shape)
        name = f"{type(self).__name__}.{who}"
        if not isinstance(images, torch.Tensor) or tuple(images.shape) != want:
            raise ValueError(f"{name} expects {self.layout!r} frames of shape {want}, got "
                             f"{tuple(images.shape) if isinstance(images, torch.Tensor) else type(images).__name__}")
        if images.dtype not in self.frames:
            raise ValueError(f"{name} expects float32 or uint8 frames, got {images.dtype}")

    def _replay(self, frames, dtype=None) -> None:
        """One forward on ``frames`` (copied into the static buffer of their dtype), or with ``frames`` None on
        what ``self.frames[dtype]`` holds (default: uint8)."""
        if frames is None:
            dtype = torch.uint8 if dtype is None else dtype
        else:
            self._check_images(frames, "pose")
            dtype = frames.dtype
        x = self.frames[dtype]
        with torch.cuda.device(self.device), torch.no_grad():
            if frames is not None:
                x.copy_(frames)
            if not self.graph:
                self._forward(x)
                return
            g = self._graphs.get(("forward", dtype))
            if g is None:
                side = torch.cuda.Stream(self.device)
                side.wait_stream(torch.cuda.current_stream())
                keep = self._tracker_state()
                with torch.cuda.stream(side):  # untimed warm-up outside the capture
                    self._forward(x)
                torch.cuda.current_stream().wait_stream(side)
                self._restore_tracker(keep)  # the warm-up ran the launches for real: the tracker must not advance
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._forward(x)
                self._graphs["forward", dtype] = g
            g.replay()

    def _tracker_state(self):
        """Clones of what argus_roi_from_pose writes (None without ``track``), for forwards that must not count."""
        if self.track is None:
            return None
        return self._roi.clone(), self._roi_used.clone(), self._roi_valid.clone()

    def _restore_tracker(self, keep) -> None:
        if keep is not None:
            for dst, src in zip((self._roi, self._roi_used, self._roi_valid), keep):
                dst.copy_(src)

    def __call__(self, frames: torch.Tensor | None, dtype=None, roi=None) -> torch.Tensor:
        """frames (fp32 in [0, 1] or uint8 in [0, 255]) -> (batch, 6) se(3), a fresh tensor. ``roi``: ``set_roi``
        first."""
        if roi is not None:
            self.set_roi(roi)
        self._replay(frames, dtype)
        return self.pred.clone()

    def pose(self, frames: torch.Tensor | None, dtype=None, roi=None) -> torch.Tensor:
        """(batch, 7) [t, qx, qy, qz, qw], a fresh tensor: written by the replay itself (``fused_head``), else
        ``utils.se3_exp`` of the prediction as the parent session. ``roi``: ``set_roi`` first."""
        if roi is not None:
            self.set_roi(roi)
        self._replay(frames, dtype)
        if not self.fused_head:
            return se3_exp(self.pred.clone())
        return self.pose_out.clone()

    def activation_peak(self, frames: torch.Tensor) -> float:
        """As the parent's, with the pooled stem output probed in place of the stem output (which no longer
        exists): the largest |activation| of one eager forward of ``frames``."""
        self._check_images(frames, "activation_peak")
        peak = torch.zeros((), dtype=torch.float32, device=self.device)

        def probe(buf, elements):
            torch.maximum(peak, buf[:elements].abs().max().float(), out=peak)

        with torch.cuda.device(self.device), torch.no_grad():
            x = self.frames[frames.dtype]
            x.copy_(frames)
            keep = self._tracker_state()
            self._forward(x, probe)
            self._restore_tracker(keep)  # a measurement, not a frame of the sequence
        return float(peak.item())
