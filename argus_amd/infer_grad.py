"""Frozen gradient session: eval-mode image gradients of the deployed ``NCameraCNN``.

``utils.image_gradient`` differentiates the train-mode forward: every BatchNorm renormalises with the
statistics of the batch at hand (two images at the batch sizes a model is deployed at) and the forward
overwrites the running statistics of the checkpoint under inspection. The question "what does the deployed
model look at on this frame" is about the eval-mode function, which the reference answers with
``model.eval()`` + ``torch.autograd.grad`` with respect to the images (argus/models.py:66-90).

A ``GradientSession`` is an ``InferenceSession`` that keeps what the backward reads and adds that backward:

- the forward is the frozen forward, launch for launch (same kernels, same splits, bit-identical
  prediction); instead of rotating through five buffers it keeps the stem output and argmax, the max-pool
  output, ``a1`` / ``a2`` / ``out`` of every block and the head pre-activations;
- with BN folded the network is conv + bias + ReLU, so the backward is one ``argus_conv_infer_dgrad`` per
  conv over a second folded weight copy in data-gradient layout (``argus_conv_fold_bn_dgrad``), the
  producer's ReLU derivative and the residual branch's gradient in its epilogue. Per block:
  ``dm2 = dgrad(conv3, dm3) * (a2 > 0)``, ``dm1 = dgrad(conv2, dm2) * (a1 > 0)``, then
  ``(dgrad(conv1, dm1) + addend) * (h > 0)`` with ``addend = dm3`` (identity residual) or
  ``dgrad(downsample, dm3)``, which is the previous block's ``dm3``;
- the head runs backward on ``argus_gemm_f32`` (epilogue 3), ``argus_avgpool_bwd_relu`` applies the last
  block's mask, the stem tail is ``argus_maxpool_bwd_bn`` + ``argus_conv_stem_dgrad`` with the eval-mode BN
  derivative ``{ca = scale, cb = 0, cc = 0}`` as its apply prologue;
- no weight gradients, no BN reductions, no side stream: a linear chain on one stream, captured with the
  forward (and the loss) as one graph per input dtype.

fp32 and bf16 only: fp16 gradients would need loss scaling to stay above the subnormals. The session never
writes the model: no running statistics, no ``num_batches_tracked``, no ``.grad``.
"""
from __future__ import annotations

import ctypes as C

import torch

from argus_amd._lib import BnBwdPrologue, ptr, stream
from argus_amd.infer import InferenceSession, _refuse_roi
from argus_amd.models import NCameraCNN

SERVED = ("fp32", "bf16")


class GradientSession(InferenceSession):
    """``session(images) -> (batch, 6)`` as ``InferenceSession``; ``vjp`` and ``image_gradient`` differentiate it.

    ``debug=True`` runs eagerly and keeps a copy of every backward launch's output in ``session.debug``, keyed by
    role (``head.*``, ``bwd.avgpool``, ``bwd.<block>.conv3|conv2|downsample|conv1``, ``bwd.maxpool``, ``bwd.dx``)."""

    def __init__(self, model: NCameraCNN, batch: int, hw: tuple, compute_dtype: str | None = None,
                 graph: bool = True, debug: bool = False):
        _refuse_roi(model, type(self).__name__)
        dtype = model.compute_dtype if compute_dtype is None else compute_dtype
        if dtype not in SERVED:
            raise ValueError(f"GradientSession serves compute_dtype 'fp32' and 'bf16', got {dtype!r} (no fp16, fp8 "
                             f"or bf16x3 gradients)")
        if next(model.parameters()).device.type != "cuda":
            raise RuntimeError("argus_amd.GradientSession runs only on the MI355X HIP path: move the model to a "
                               "cuda device (there is no CPU fallback)")
        self.debug: dict | None = {} if debug else None
        super().__init__(model, batch, hw, dtype, graph and not debug)

    # ------------------------------------------------------------------ construction
    def _plan(self) -> None:
        super()._plan()
        L, dt, N, B = self.L, self.dt, self.N, self.batch
        (H, W), (H1, W1), (H2, W2) = self.hw, self.stem_hw, self.pool_hw
        ws_bytes = self.ws.numel()
        for cv in self.convs.values():
            d = cv.desc
            sp, mx, nb = C.c_int(0), C.c_int(0), C.c_size_t(0)
            L.conv_infer_dgrad_plan(C.byref(d), dt, 0, C.byref(sp), C.byref(mx), C.byref(nb))
            cv.wfd = self._empty(d.c, d.r * d.s * d.k)  # the second folded copy, [C][R*S*K]
            cv.bwd_splits, cv.bwd_ws_bytes = sp.value, nb.value
            ws_bytes = max(ws_bytes, nb.value)
        # one split workspace for the forward and the backward (one stream, in order), tickets zeroed once
        self.ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=self.device)
        # what the backward reads: stem output, max-pool output, a1 / a2 / out of every block (the five pool
        # buffers now rotate the gradients; the downsample output, which no backward reads, borrows one)
        self.y0, self.p0 = self._empty(N, H1, W1, 64), self._empty(N, H2, W2, 64)
        self.acts = []
        for c1, c2, c3, _ in self.schedule:
            self.acts.append(tuple(self._empty(cv.desc.n, cv.desc.ho, cv.desc.wo, cv.desc.k) for cv in (c1, c2, c3)))
        f = lambda *s: self._empty(*s, dtype=torch.float32)  # noqa: E731
        D = self.n_cams * self.rdim
        self.dh2, self.dh1, self.dh0, self.dfeat = f(B, 128), f(B, 128), f(B, D), f(N, 2048)
        self.target, self.dpred, self.loss = f(B, 7), f(B, 6), f(B)
        self.dx = f(B, 3 * self.n_cams, H, W)
        # the stem tail reuses the train-mode maxpool backward: its BN-reduction partials go to a scratch
        # row buffer nobody reads (mean 0, invstd 1 keep them finite)
        rows = L.dll.argus_maxpool_bwd_bn_rows(dt, N, H1, W1, 64)
        self.mp_part = f(max(rows, 1), 64, 2)
        self.zero64, self.one64 = torch.zeros(64, device=self.device), torch.ones(64, device=self.device)
        hws = max(L.dll.argus_gemm_f32_workspace_bytes(*s) for s in
                  [(B, 128, 6), (B, 128, 128), (B, D, 128), (N, 2048, self.rdim)])
        if hws > self.gemm_ws.numel():
            self.gemm_ws = self._empty(hws, dtype=torch.uint8)
        self.saved_bytes = sum(t.numel() * t.element_size() for t in
                               [self.y0, self.p0] + [t for a in self.acts for t in a])
        # head: three GELU-backward GEMMs + the fc data gradient; avg-pool; the convs; max-pool; stem
        self.launches_per_backward = 4 + 1 + len(self.convs) + 2

    def refresh(self) -> None:
        """Re-fold both weight copies from the model's current parameters and buffers (never writes the model)."""
        super().refresh()
        self.weight_bytes += sum(cv.wfd.numel() * cv.wfd.element_size() for cv in self.convs.values())

    def _fold(self, cv, master, s) -> None:
        super()._fold(cv, master, s)
        self.L.conv_fold_bn_dgrad(C.byref(cv.desc), self.dt, *master, ptr(cv.wfd), s)

    def _buffers(self):
        """Every activation the backward reads goes to its own tensor (yd, which it does not read, borrows one)."""
        return self.y0, self.p0, [(*acts, self.pool[3]) for acts in self.acts]

    # ------------------------------------------------------------------ backward
    def _keep(self, role: str, t: torch.Tensor, shape=None) -> None:
        if self.debug is not None:
            self.debug[role] = (t if shape is None else t[:shape.numel()].view(shape)).clone()

    def _dgrad(self, cv, dy, addend, mask, dx, s, role: str) -> None:
        d = cv.desc
        self.L.conv_infer_dgrad(C.byref(d), self.dt, ptr(dy), ptr(cv.wfd), ptr(addend), ptr(mask), ptr(dx),
                                cv.bwd_splits, ptr(self.ws), self.ws.numel(), s)
        self._keep(role, dx, torch.Size((d.n, d.h, d.w, d.c)))

    def _backward(self, dpred: torch.Tensor) -> torch.Tensor:
        """The launches of one backward from the contiguous fp32 (batch, 6) cotangent ``dpred`` of self.pred into
        self.dx, reading what the last _forward kept."""
        L, dt, s, N, B = self.L, self.dt, stream(), self.N, self.batch
        D, R = self.n_cams * self.rdim, self.rdim
        hd, ws, wsn = self.head, ptr(self.gemm_ws), self.gemm_ws.numel()
        w0, w2, w4 = hd["output_mlp.0", "weight"], hd["output_mlp.2", "weight"], hd["output_mlp.4", "weight"]
        # MLP and fc, as ResNetEngine.backward: each GEMM applies the GELU derivative at its pre-activation
        L.gemm_f32(B, 128, 6, ptr(dpred), 6, 0, ptr(w4), 128, 0, ptr(self.dh2), 128, None, 3, ptr(self.h2), ws, wsn, s)
        self._keep("head.dh2", self.dh2)
        L.gemm_f32(B, 128, 128, ptr(self.dh2), 128, 0, ptr(w2), 128, 0, ptr(self.dh1), 128, None, 3, ptr(self.h1), ws,
                   wsn, s)
        self._keep("head.dh1", self.dh1)
        L.gemm_f32(B, D, 128, ptr(self.dh1), 128, 0, ptr(w0), D, 0, ptr(self.dh0), D, None, 3, ptr(self.h0), ws, wsn, s)
        self._keep("head.dh0", self.dh0)
        L.gemm_f32(N, 2048, R, ptr(self.dh0), R, 0, ptr(hd["resnet.fc", "weight"]), 2048, 0, ptr(self.dfeat), 2048,
                   None, 0, None, ws, wsn, s)
        self._keep("head.dfeat", self.dfeat)
        dm3, dm2, dm1, dd, dx = self.pool
        hf, wf = self.final_hw
        last = self.acts[-1][2]
        L.avgpool_bwd_relu(dt, N, hf * wf, 2048, ptr(self.dfeat), ptr(last), ptr(dm3), s)
        self._keep("bwd.avgpool", dm3, last.shape)
        for i in range(len(self.schedule) - 1, -1, -1):
            c1, c2, c3, ds = self.schedule[i]
            a1, a2, _ = self.acts[i]
            h = self.acts[i - 1][2] if i else self.p0
            pf = c1.name[:-len(".conv1")]
            self._dgrad(c3, dm3, None, a2, dm2, s, f"bwd.{pf}.conv3")
            self._dgrad(c2, dm2, None, a1, dm1, s, f"bwd.{pf}.conv2")
            addend = dm3
            if ds is not None:
                self._dgrad(ds, dm3, None, None, dd, s, f"bwd.{pf}.downsample")
                addend = dd
            self._dgrad(c1, dm1, addend, h, dx, s, f"bwd.{pf}.conv1")
            dm3, dx = dx, dm3
        # stem: max-pool backward through the stem's ReLU (dm0 = dz * (y0 * scale + shift > 0)), then the stem data
        # gradient of scale * dm0, the eval-mode BatchNorm derivative, formed while staging
        H1, W1 = self.stem_hw
        dm0 = dm2
        L.maxpool_bwd_bn(dt, N, H1, W1, 64, ptr(dm3), ptr(self.amax), ptr(dm0), ptr(self.y0), ptr(self.stem_coef[0]),
                         ptr(self.stem_coef[1]), ptr(self.zero64), ptr(self.one64), ptr(self.mp_part), s)
        self._keep("bwd.maxpool", dm0, self.y0.shape)
        ap = BnBwdPrologue(ptr(self.y0), ptr(self.stem_coef[0]), ptr(self.zero64), ptr(self.zero64), None)
        L.conv_stem_dgrad(C.byref(self.stem_desc), dt, ptr(dm0), ptr(self.stem_wf), C.byref(ap), ptr(self.dx), s)
        self._keep("bwd.dx", self.dx)
        return self.dx

    # ------------------------------------------------------------------ public
    def vjp(self, images: torch.Tensor, dpred: torch.Tensor) -> torch.Tensor:
        """d<session(images), dpred>/d images: fp32 (batch, 3*n_cams, H, W), a fresh tensor. ``images`` as
        ``session(images)`` takes them (uint8: the gradient with respect to the /255 image); ``dpred`` a
        (batch, 6) floating cotangent. The prediction of this forward stays in ``session.pred``."""
        self._check_images(images, "vjp")
        if not isinstance(dpred, torch.Tensor) or tuple(dpred.shape) != (self.batch, 6) or \
                not dpred.is_floating_point():
            raise ValueError(f"GradientSession.vjp expects a floating dpred of shape {(self.batch, 6)}")
        self.dpred.copy_(dpred)

        def body(x):
            self._forward(x)
            self._backward(self.dpred)

        self._run("vjp", images, body)
        return self.dx.clone()

    def image_gradient(self, images: torch.Tensor, target: torch.Tensor) -> tuple:
        """(losses (batch,), grad) with grad = d(mean SE(3) loss)/d images at the deployed weights and running
        statistics: ``utils.image_gradient``'s contract for the eval-mode function. ``target``: (batch, 7) poses.
        The loss kernel's cotangent (grad_scale 1/batch) stays in ``session.dpred``."""
        self._check_images(images, "image_gradient")
        if not isinstance(target, torch.Tensor) or tuple(target.shape) != (self.batch, 7) or \
                not target.is_floating_point():
            raise ValueError(f"GradientSession.image_gradient expects a floating target of shape {(self.batch, 7)}")
        self.target.copy_(target)

        def body(x):
            self._forward(x)
            self.L.se3_loss(self.batch, ptr(self.pred), ptr(self.target), ptr(self.loss), ptr(self.dpred),
                            C.c_float(1.0 / self.batch), stream())
            self._backward(self.dpred)

        self._run("image_gradient", images, body)
        return self.loss.clone(), self.dx.clone()
