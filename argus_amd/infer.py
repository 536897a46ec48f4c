"""Frozen inference session: the deployed form of ``NCameraCNN`` (two camera frames in, one pose out).

``model.eval()`` runs the training schedule with running statistics: every call converts all conv weights
again, launches ``bn_eval_coeffs`` per BatchNorm, keeps every activation for a backward that never comes
and picks tiles for tens of thousands of GEMM rows. A session freezes the model instead:

- every non-stem BatchNorm is folded into its conv once (``argus_conv_fold_bn``: ``w * scale`` rounded
  once to the compute dtype, ``shift`` as an fp32 bias); the stem keeps its LDS-patch kernel with the
  coefficients computed once (``argus_bn_eval_coeffs``) and applied by the fused max-pool;
- each conv is one launch of ``argus_conv_infer`` with bias + residual + ReLU in its epilogue, its
  reduction split over workgroups where the tile count leaves the chip idle;
- activations rotate through five buffers, nothing is saved per layer;
- everything is issued on one stream in program order, so the captured graph is a linear chain.

``compute_dtype="fp16"`` (chosen explicitly; there is no fp16 training) runs the same launches on IEEE half
tensors: bf16's MFMA rate and bytes with 8x smaller rounding steps, at the price of range. Every fp16 store
saturates to +-65504, ``refresh()`` refuses a checkpoint whose folded weights do not fit, and
``activation_peak`` reports the headroom of the activations on given frames.

The session is a snapshot: later changes to the model show only after ``refresh()``, and the session never
writes to the model. It replaces ``self.resnet(x)`` + the head of ``NCameraCNN.forward`` in eval mode
(argus/models.py:66-90) behind ``get_pose`` (argus/utils.py:179-189).
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from argus_amd._lib import BF16, F16, F32, ConvDesc, lib, ptr, stream
from argus_amd.engine import _out, resnet50_blocks
from argus_amd.models import NCameraCNN
from argus_amd.utils import se3_exp

SERVED = ("fp32", "bf16", "fp16")
_DT = {"fp32": (F32, torch.float32), "bf16": (BF16, torch.bfloat16), "fp16": (F16, torch.float16)}
F16_MAX = 65504.0  # the largest finite fp16: every fp16 store of the library saturates to it


class _Conv:
    """One folded conv: descriptor, the master weight / BN names it is folded from, folded weight + bias."""

    def __init__(self, name, bn, desc, wf, bias, splits, ws_bytes):
        self.name, self.bn, self.desc, self.wf, self.bias = name, bn, desc, wf, bias
        self.splits, self.ws_bytes = splits, ws_bytes


def _require_cuda(model):
    """The model's first parameter; a model that is not on a cuda device is refused (no CPU fallback)."""
    p0 = next(model.parameters())
    if p0.device.type != "cuda":
        raise RuntimeError("argus_amd.InferenceSession runs only on the MI355X HIP path: move the model to a "
                           "cuda device (there is no CPU fallback)")
    return p0


def _refuse_roi(model, who: str) -> None:
    """Only PoseSession serves a model conditioned on the region of interest (NCameraCNNConfig.roi_frame_hw)."""
    if getattr(model, "roi_frame_hw", None) is not None:
        raise ValueError(f"{who} does not serve a model built with roi_frame_hw = {model.roi_frame_hw}: it has no "
                         f"region-of-interest input (PoseSession(roi=True) does)")


class InferenceSession:
    """``session(images) -> (batch, 6)`` for a fixed ``batch`` and image size ``hw``.

    ``compute_dtype``: "fp32", "bf16" or "fp16" (default: the model's; "fp16" only when asked for). ``graph``: capture the forward once per
    input dtype (fp32 / uint8) and replay it per call; False issues the same launches eagerly."""

    _serves_roi = False  # a conditioned model (roi_frame_hw) is refused; PoseSession overrides

    def __init__(self, model: NCameraCNN, batch: int, hw: tuple, compute_dtype: str | None = None,
                 graph: bool = True):
        if not self._serves_roi:
            _refuse_roi(model, type(self).__name__)
        dtype = model.compute_dtype if compute_dtype is None else compute_dtype
        if dtype not in SERVED:
            raise ValueError(f"InferenceSession serves compute_dtype 'fp32' and 'bf16' (and 'fp16' when passed "
                             f"explicitly), got {dtype!r}")
        p0 = _require_cuda(model)
        self.model, self.device = model, p0.device
        self.batch, self.hw, self.compute_dtype, self.graph = int(batch), (int(hw[0]), int(hw[1])), dtype, bool(graph)
        self.n_cams, self.rdim = model.n_cams, model.resnet_output_dim
        self.L = lib()
        self.dt, self.tdt = _DT[dtype]
        self._graphs: dict = {}
        with torch.cuda.device(self.device):
            self._plan()
            self.refresh()

    # ------------------------------------------------------------------ construction
    def _empty(self, *shape, dtype=None):
        return torch.empty(shape, dtype=dtype or self.tdt, device=self.device)

    def _plan(self) -> None:
        L, dt = self.L, self.dt
        B, (H, W) = self.batch, self.hw
        N = self.N = B * self.n_cams
        H1, W1 = _out(H, 7, 2, 3), _out(W, 7, 2, 3)
        H2, W2 = _out(H1, 3, 2, 1), _out(W1, 3, 2, 1)
        self.stem_hw, self.pool_hw = (H1, W1), (H2, W2)
        self.stem_desc = ConvDesc(N, H, W, 3, 64, 7, 7, 2, 3, H1, W1, 1)
        self.stem_wf = self._empty(64, 256)
        self.stem_coef = self._empty(2, 64, dtype=torch.float32)  # scale, shift of resnet.bn1
        max_elems = self._plan_convs()
        self._alloc_activations(max(max_elems, N * H1 * W1 * 64))
        self._alloc_head()
        self._alloc_inputs()
        # images -> NHWC4, stem conv, max-pool, the convs, avg-pool, fc, GELU, three MLP GEMMs
        self.launches_per_forward = 3 + len(self.convs) + 6

    def _plan_convs(self) -> int:
        """The 52 folded convs and the block schedule; returns the elements of the largest block activation."""
        L, dt, N = self.L, self.dt, self.N
        h, w = self.pool_hw
        self.convs: dict[str, _Conv] = {}
        self.schedule = []  # per block: (conv1, conv2, conv3, downsample | None)

        def add(name, bn, n, h, w, c, k, ks, s, p):
            d = ConvDesc(n, h, w, c, k, ks, ks, s, p, _out(h, ks, s, p), _out(w, ks, s, p), 0)
            splits = L.dll.argus_conv_infer_splits(C.byref(d), dt)
            if splits < 1:
                raise RuntimeError(f"argus_conv_infer does not serve {name}: "
                                   f"{L.dll.argus_last_error().decode(errors='replace')}")
            cv = _Conv(name, bn, d, self._empty(k, ks * ks * c), self._empty(k, dtype=torch.float32), splits,
                       L.dll.argus_conv_infer_workspace_bytes(C.byref(d), dt, splits))
            self.convs[name] = cv
            return cv

        max_elems = 0
        for b in resnet50_blocks():
            pf = b.prefix
            c1 = add(pf + ".conv1", pf + ".bn1", N, h, w, b.cin, b.width, 1, 1, 0)
            c2 = add(pf + ".conv2", pf + ".bn2", N, h, w, b.width, b.width, 3, b.stride, 1)
            ho, wo = c2.desc.ho, c2.desc.wo
            c3 = add(pf + ".conv3", pf + ".bn3", N, ho, wo, b.width, b.cout, 1, 1, 0)
            ds = add(pf + ".downsample.0", pf + ".downsample.1", N, h, w, b.cin, b.cout, 1, b.stride, 0) if b.has_ds \
                else None
            self.schedule.append((c1, c2, c3, ds))
            max_elems = max(max_elems, N * h * w * b.cin, N * h * w * b.width, N * ho * wo * b.cout)
            h, w = ho, wo
        self.final_hw = (h, w)
        return max_elems

    def _alloc_activations(self, max_elems: int) -> None:
        # activations: the block input / output pair, a1, a2 and yd (the stem output borrows the a1 buffer)
        N, (H, W), (H2, W2) = self.N, self.hw, self.pool_hw
        self.x0 = self._empty(N, H, W, 4)
        self.pool = [self._empty(max_elems) for _ in range(5)]
        self.amax = self._empty(N * H2 * W2 * 64, dtype=torch.uint8)
        # one split workspace for the largest request, its tickets zeroed here once (every call leaves them zero)
        self.ws = torch.zeros(max(max(cv.ws_bytes for cv in self.convs.values()), 16), dtype=torch.uint8,
                              device=self.device)
        self.activation_bytes = (self.x0.numel() * self.x0.element_size()
                                 + sum(t.numel() * t.element_size() for t in self.pool) + self.amax.numel())

    def _alloc_head(self) -> None:
        # head (fp32), as ResNetEngine
        L, N, B = self.L, self.N, self.batch
        D = self.n_cams * self.rdim
        f = lambda *s: self._empty(*s, dtype=torch.float32)  # noqa: E731
        self.feat, self.h0, self.g0 = f(N, 2048), f(N, self.rdim), f(B, D)
        self.h1, self.g1, self.h2, self.g2, self.pred = f(B, 128), f(B, 128), f(B, 128), f(B, 128), f(B, 6)
        hws = max(L.dll.argus_gemm_f32_workspace_bytes(*s) for s in
                  [(N, self.rdim, 2048), (B, 128, D), (B, 128, 128), (B, 6, 128)])
        self.gemm_ws = self._empty(max(hws, 16), dtype=torch.uint8)
        self.head = {}
        self.activation_bytes += 4 * sum(t.numel() for t in (self.feat, self.h0, self.g0, self.h1, self.g1, self.h2,
                                                             self.g2, self.pred))

    def _alloc_inputs(self) -> None:
        B, (H, W) = self.batch, self.hw
        self.static_in = {torch.float32: self._empty(B, 3 * self.n_cams, H, W, dtype=torch.float32),
                          torch.uint8: self._empty(B, 3 * self.n_cams, H, W, dtype=torch.uint8)}

    def refresh(self) -> None:
        """Re-fold from the model's current parameters and buffers (reads the model, never writes it)."""
        L, dt = self.L, self.dt
        with torch.cuda.device(self.device), torch.no_grad():
            s = stream()
            P = dict(self.model.named_parameters())
            Bf = dict(self.model.named_buffers())
            eps = {n: m.eps for n, m in self.model.named_modules() if isinstance(m, nn.BatchNorm2d)}
            for t in list(P.values()) + list(Bf.values()):
                if t.device != self.device or (t.is_floating_point() and t.dtype != torch.float32):
                    raise RuntimeError("argus_amd.InferenceSession: model parameters must be fp32 on one cuda device")
            w = P["resnet.conv1.weight"]
            st = (C.c_int64 * 4)(*w.stride())
            L.conv_weight_prep(C.byref(self.stem_desc), dt, ptr(w), st, ptr(self.stem_wf), None, s)
            L.bn_eval_coeffs(64, ptr(P["resnet.bn1.weight"]), ptr(P["resnet.bn1.bias"]),
                             ptr(Bf["resnet.bn1.running_mean"]), ptr(Bf["resnet.bn1.running_var"]),
                             C.c_float(eps["resnet.bn1"]), ptr(self.stem_coef[0]), ptr(self.stem_coef[1]), s)
            for cv in self.convs.values():
                w = P[cv.name + ".weight"]
                self._fold(cv, (ptr(w), (C.c_int64 * 4)(*w.stride()), ptr(P[cv.bn + ".weight"]),
                                ptr(P[cv.bn + ".bias"]), ptr(Bf[cv.bn + ".running_mean"]),
                                ptr(Bf[cv.bn + ".running_var"]), C.c_float(eps[cv.bn])), s)
            if self.compute_dtype == "fp16":
                self._check_f16_range()
            names = [(n, k) for n in ("resnet.fc", "output_mlp.0", "output_mlp.2", "output_mlp.4")
                     for k in ("weight", "bias")]
            if "roi_embed.weight" in P:
                names.append(("roi_embed", "weight"))
            for n, k in names:
                src = P[f"{n}.{k}"].detach()
                if (n, k) in self.head:
                    self.head[n, k].copy_(src)  # in place: captured graphs keep reading these tensors
                else:
                    self.head[n, k] = src.clone().contiguous()
        self.weight_bytes = (self.stem_wf.numel() * self.stem_wf.element_size() + 8 * 64
                             + sum(cv.wf.numel() * cv.wf.element_size() + 4 * cv.bias.numel()
                                   for cv in self.convs.values())
                             + 4 * sum(t.numel() for t in self.head.values()))

    def _fold(self, cv: _Conv, master, s) -> None:
        """Fold ``cv`` from ``master``: (weight, strides, gamma, beta, running mean, running var, eps), the
        arguments every fold entry point takes between the dtype and its outputs."""
        self.L.conv_fold_bn(C.byref(cv.desc), self.dt, *master, ptr(cv.wf), ptr(cv.bias), s)

    def _check_f16_range(self) -> None:
        """fp16 cannot hold a checkpoint whose folded weight overflows: the fold saturated it to +-65504 (or the
        master was not finite). Say so here, once per refresh, not through a pose."""
        for name, wf in [("resnet.conv1", self.stem_wf)] + [(cv.name, cv.wf) for cv in self.convs.values()]:
            a = wf.abs().max().item()
            if not a < F16_MAX:  # 65504 (saturated), inf or NaN
                raise ValueError(f"InferenceSession(compute_dtype='fp16'): the folded weight of {name} reaches "
                                 f"{a} (fp16 holds magnitudes below {F16_MAX}); serve this checkpoint in 'bf16' "
                                 f"or 'fp32'")

    # ------------------------------------------------------------------ forward
    def _conv(self, cv: _Conv, x, out, res, relu: int, s, probe=None) -> None:
        self.L.conv_infer(C.byref(cv.desc), self.dt, ptr(x), ptr(cv.wf), ptr(cv.bias), ptr(res), relu, ptr(out),
                          cv.splits, ptr(self.ws), self.ws.numel(), s)
        if probe is not None:
            probe(out, cv.desc.n * cv.desc.ho * cv.desc.wo * cv.desc.k)

    def _buffers(self):
        """Where a forward writes: the stem output, the max-pool output and per block (a1, a2, out, yd); a block's
        ``out`` is the next block's input. Here: five rotating buffers, the stem output borrowing a1's."""
        h, a1, a2, yd, out = self.pool
        blocks = []
        for _ in self.schedule:
            blocks.append((a1, a2, out, yd))
            h, out = out, h
        return a1, self.pool[0], blocks

    def _to_nhwc4(self, x: torch.Tensor, s) -> None:
        """The first launch of a forward: ``x`` as the stem conv reads it, into self.x0."""
        L, dt, N, (H, W) = self.L, self.dt, self.N, self.hw
        if x.dtype == torch.uint8:
            L.images_u8_to_nhwc4(dt, N, H, W, ptr(x), ptr(self.x0), s)
        else:
            L.images_to_nhwc4(dt, N, H, W, ptr(x), ptr(self.x0), s)

    def _forward(self, x: torch.Tensor, probe=None) -> torch.Tensor:
        """The launches of one forward from the contiguous (batch, 3*n_cams, H, W) tensor ``x`` into self.pred.
        ``probe(buffer, elements)``: called after every launch that writes an activation (activation_peak)."""
        L, dt, s, N = self.L, self.dt, stream(), self.N
        self._to_nhwc4(x, s)
        y0, h, blocks = self._buffers()
        H1, W1 = self.stem_hw
        L.conv_fwd(C.byref(self.stem_desc), dt, ptr(self.x0), ptr(self.stem_wf), ptr(y0), None, None, None, s)
        if probe is not None:
            probe(y0, N * H1 * W1 * 64)
        L.maxpool_fwd(dt, N, H1, W1, 64, ptr(y0), ptr(self.stem_coef[0]), ptr(self.stem_coef[1]), ptr(h),
                      ptr(self.amax), s)
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

    def _head(self, h: torch.Tensor) -> torch.Tensor:
        """Average pool of the last block's output ``h``, fc, GELU and the MLP into self.pred (fp32)."""
        L, dt, s, N = self.L, self.dt, stream(), self.N
        hf, wf = self.final_hw
        L.avgpool_fwd(dt, N, hf * wf, 2048, ptr(h), ptr(self.feat), s)
        B, D, R = self.batch, self.n_cams * self.rdim, self.rdim
        hd, ws, wsn = self.head, ptr(self.gemm_ws), self.gemm_ws.numel()
        L.gemm_f32(N, R, 2048, ptr(self.feat), 2048, 0, ptr(hd["resnet.fc", "weight"]), 2048, 1, ptr(self.h0), R,
                   ptr(hd["resnet.fc", "bias"]), 1, None, ws, wsn, s)
        L.gelu_f32(B * D, ptr(self.h0), ptr(self.g0), s)
        self._mlp0(ws, wsn, s)
        L.gemm_f32(B, 128, 128, ptr(self.g1), 128, 0, ptr(hd["output_mlp.2", "weight"]), 128, 1, ptr(self.g2), 128,
                   ptr(hd["output_mlp.2", "bias"]), 2, ptr(self.h2), ws, wsn, s)
        L.gemm_f32(B, 6, 128, ptr(self.g2), 128, 0, ptr(hd["output_mlp.4", "weight"]), 128, 1, ptr(self.pred), 6,
                   ptr(hd["output_mlp.4", "bias"]), 1, None, ws, wsn, s)
        return self.pred

    def _mlp0(self, ws, wsn, s) -> None:
        """g1 = gelu(h1), h1 = output_mlp.0(g0): one GEMM with the bias + GELU epilogue."""
        L, B, D, hd = self.L, self.batch, self.n_cams * self.rdim, self.head
        L.gemm_f32(B, 128, D, ptr(self.g0), D, 0, ptr(hd["output_mlp.0", "weight"]), D, 1, ptr(self.g1), 128,
                   ptr(hd["output_mlp.0", "bias"]), 2, ptr(self.h1), ws, wsn, s)

    def _check_images(self, images, who: str) -> None:
        want = (self.batch, 3 * self.n_cams, *self.hw)
        name = f"{type(self).__name__}.{who}"
        if not isinstance(images, torch.Tensor) or tuple(images.shape) != want:
            raise ValueError(f"{name} expects images of shape {want}, got "
                             f"{tuple(images.shape) if isinstance(images, torch.Tensor) else type(images).__name__}")
        if images.dtype not in self.static_in:
            raise ValueError(f"{name} expects float32 or uint8 images, got {images.dtype}")

    def _run(self, kind: str, images: torch.Tensor, body) -> None:
        """``body(x)`` eagerly on ``images``, or captured once per (kind, input dtype) and replayed."""
        with torch.cuda.device(self.device), torch.no_grad():
            if not self.graph:
                body(images.to(self.device).contiguous())
                return
            x = self.static_in[images.dtype]
            x.copy_(images)
            g = self._graphs.get((kind, images.dtype))
            if g is None:
                side = torch.cuda.Stream(self.device)
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):  # untimed warm-up outside the capture
                    body(x)
                torch.cuda.current_stream().wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    body(x)
                self._graphs[kind, images.dtype] = g
            g.replay()

    def __call__(self, images: torch.Tensor) -> torch.Tensor:
        """(batch, 3*n_cams, H, W) fp32 images in [0, 1] or uint8 in [0, 255] -> (batch, 6) se(3), a fresh tensor."""
        self._check_images(images, "__call__")
        self._run("forward", images, self._forward)
        return self.pred.clone()

    def activation_peak(self, images: torch.Tensor) -> float:
        """The largest |activation| one forward of ``images`` writes to any activation buffer (stem output,
        max-pool output, every conv output), from one eager forward outside the graph. A diagnostic, not the
        hot path: in fp16 it shows the headroom under 65504 (a saturated activation reads exactly 65504)."""
        self._check_images(images, "activation_peak")
        peak = torch.zeros((), dtype=torch.float32, device=self.device)

        def probe(buf, elements):
            torch.maximum(peak, buf[:elements].abs().max().float(), out=peak)

        with torch.cuda.device(self.device), torch.no_grad():
            self._forward(images.to(self.device).contiguous(), probe)
        return float(peak.item())

    def pose(self, images: torch.Tensor) -> torch.Tensor:
        """(batch, 7) [t, qx, qy, qz, qw]: ``utils.se3_exp`` of the prediction, as ``get_pose``."""
        return se3_exp(self(images))
