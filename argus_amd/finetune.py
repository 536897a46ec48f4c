"""Frozen-BatchNorm fine-tuning: one optimisation step of the eval-mode ``NCameraCNN``.

``FusedTrainer`` trains with train-mode BatchNorm: every BN renormalises with the batch at hand and every
forward overwrites the running statistics. Adapting a trained checkpoint to a few real frames (two to sixteen
images per step) needs the opposite: the statistics the checkpoint was validated with stay frozen and only the
parameters move. The reference does this with ``model.eval()`` + ``loss.backward()`` + ``clip_grad_norm_`` +
``Adam.step()`` (argus/models.py:66-90, argus/train.py:298-321).

A ``FineTuneSession`` is a ``GradientSession`` that adds the parameter gradients and the optimizer:

- the parameters live in a ``step.FlatParams`` (the model's parameters become views of it, as under
  ``FusedTrainer``; one they are already views of is taken over), the folds read those masters, the head reads them
  directly;
- ``step()`` re-folds both weight copies of the trainable convs from the masters (one table-driven launch,
  ``argus_conv_fold_bn_batch``), runs the frozen forward, ``argus_se3_loss`` and the ``GradientSession`` backward;
  while a block's operands are alive, each conv's ``argus_conv_wgrad`` writes dL/d(w_fold) straight into the flat
  gradient slot and ``argus_bias_grad`` sums dm into dL/d(bias); after the block loop one
  ``argus_conv_fold_bn_bwd_batch`` applies the chain rule through every fold in place, giving the gradients of
  (w, gamma, beta). The stem, which is not folded, uses the training entries (``argus_maxpool_bwd_bn`` with the
  running mean and invstd, ``argus_bn_bwd_finalize``, ``argus_conv_wgrad_apply``); the head is
  ``ResNetEngine.backward``'s ``head_wgrads``. ``argus_global_norm`` closes the graph: a linear chain on one
  stream, captured once per input dtype;
- ``argus_adam_step`` (clip + Adam, lr and bias corrections by value) is launched after the replay, then a
  second small graph re-folds, so ``session(images)``, ``pose``, ``vjp`` and ``image_gradient`` see the
  updated parameters.

``trainable="layerK"`` trains ``resnet.layerK`` .. ``resnet.layer4``, ``resnet.fc`` and ``output_mlp`` (stock PyTorch:
``requires_grad_(False)`` on everything before, ``model.eval()``, ``clip_grad_norm_`` and ``Adam`` over the rest). The
flat buffer is in model order, so that is a suffix of it, as the head is: norm and Adam run over the suffix, the
backward's block loop stops at ``layerK.0`` (whose conv1 and downsample get no data gradient: nobody reads it), and
nothing of the stem's backward is launched. The forward and everything the session serves stay at full depth.

The session writes parameters only through Adam: never a BN buffer, never ``num_batches_tracked``, and it
never calls ``model.train()``. fp32 and bf16, one process (no data-parallel fine-tuning).
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.distributed as dist
import torch.nn as nn

from argus_amd._lib import FOLD_ENTRY_BYTES, BnBwdPrologue, FoldSrc, ptr, stream
from argus_amd.infer import _refuse_roi
from argus_amd.infer_grad import SERVED, GradientSession
from argus_amd.models import NCameraCNN
from argus_amd.step import FlatParams

STAGES = ("layer1", "layer2", "layer3", "layer4")
TRAINABLE = ("all", "head") + STAGES
HEAD = ("resnet.fc", "output_mlp.0", "output_mlp.2", "output_mlp.4")


def _adopt_flat(model: nn.Module) -> FlatParams | None:
    """The ``FlatParams`` the model's parameters are already views of (a ``FusedTrainer`` made one: pre-training and
    fine-tuning then share one parameter and one gradient buffer), rebuilt from the views; None when they are not."""
    params = list(model.named_parameters())
    p0 = params[0][1]
    if p0.grad is None:
        return None
    ps, gs = p0.untyped_storage(), p0.grad.untyped_storage()
    flat = FlatParams.__new__(FlatParams)
    flat.slots, flat.offset, flat.G = [], {}, {}
    end = 0
    for n, p in params:
        g = p.grad
        ohwi = (lambda t: t.permute(0, 2, 3, 1)) if p.dim() == 4 else (lambda t: t)
        if g is None or p.dtype != torch.float32 or g.dtype != torch.float32 or g.shape != p.shape or \
                p.untyped_storage().data_ptr() != ps.data_ptr() or g.untyped_storage().data_ptr() != gs.data_ptr() or \
                not ohwi(p).is_contiguous() or not ohwi(g).is_contiguous() or \
                p.storage_offset() != g.storage_offset() or p.storage_offset() % FlatParams.ALIGN or \
                p.storage_offset() < end:
            return None
        o = p.storage_offset()
        end = o + p.numel()
        flat.slots.append((n, p, o, p.numel()))
        flat.offset[n] = o
        flat.G[n] = ohwi(g)
    flat.total = (end + FlatParams.ALIGN - 1) // FlatParams.ALIGN * FlatParams.ALIGN
    if ps.nbytes() < 4 * flat.total or gs.nbytes() < 4 * flat.total:
        return None
    flat.param = torch.empty(0, dtype=torch.float32, device=p0.device).set_(ps, 0, (flat.total,))
    flat.grad = torch.empty(0, dtype=torch.float32, device=p0.device).set_(gs, 0, (flat.total,))
    return flat


class _OptState:
    """What the sessions of one model share: the flat parameters, Adam's moments and its step count."""

    def __init__(self, model: nn.Module):
        self.flat = _adopt_flat(model) or FlatParams(model)
        self.exp_avg = torch.zeros_like(self.flat.param)
        self.exp_avg_sq = torch.zeros_like(self.flat.param)
        self.step_count = 0

    def owns(self, model: nn.Module) -> bool:
        """True while every parameter of the model is still the view of the flat buffer it was made."""
        base = self.flat.param.data_ptr()
        return all(p.data_ptr() == base + 4 * o for _, p, o, _ in self.flat.slots) and \
            [n for n, _ in model.named_parameters()] == [s[0] for s in self.flat.slots]


def _opt_state(model: nn.Module) -> _OptState:
    """The model's optimizer state: an existing one if its parameters are already views of one (a second
    session of another batch size continues the same Adam moments), else a fresh one."""
    st = model.__dict__.get("_finetune_state")
    if st is None or not st.owns(model):
        st = _OptState(model)
        model.__dict__["_finetune_state"] = st
    return st


class FineTuneSession(GradientSession):
    """``step(images, target) -> losses (batch,)``: one clip + Adam step of the eval-mode function; everything a
    ``GradientSession`` serves, at the current parameters.

    ``trainable="head"`` trains ``resnet.fc`` and ``output_mlp`` only: no conv data gradient, weight gradient or
    fold is launched, the backbone gradients stay zero and its parameters bit-identical. ``trainable="layerK"``
    (K = 1..4) trains ``resnet.layerK`` and everything behind it; the stem and the earlier stages are frozen: their
    parameters, gradient slots and Adam moments are never written. A step re-folds what its own session trains:
    after a session that trains more has stepped on the same model, ``refresh()`` this one first. ``launch_plan``
    counts the launches of a step by kind. ``debug=True`` runs eagerly and adds ``wgrad.<conv>`` (dL/d w_fold),
    ``dbias.<conv>`` and ``fold_bwd.<conv>`` (a tuple dw, dgamma, dbeta) to ``session.debug``, beside ``stem.*`` and
    ``head.*``, for what was launched. ``lr`` is writable."""

    def __init__(self, model: NCameraCNN, batch: int, hw: tuple, compute_dtype: str | None = None,
                 lr: float = 1e-4, max_grad_norm: float = 1.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, trainable: str = "all", graph: bool = True, debug: bool = False):
        _refuse_roi(model, type(self).__name__)
        dtype = model.compute_dtype if compute_dtype is None else compute_dtype
        if dtype not in SERVED:
            raise ValueError(f"FineTuneSession serves compute_dtype 'fp32' and 'bf16', got {dtype!r} (no fp16, fp8 "
                             f"or bf16x3 fine-tuning)")
        if trainable not in TRAINABLE:
            raise ValueError(f"FineTuneSession: trainable must be one of {', '.join(map(repr, TRAINABLE))}, got "
                             f"{trainable!r}")
        if next(model.parameters()).device.type != "cuda":
            raise RuntimeError("argus_amd.FineTuneSession runs only on the MI355X HIP path: move the model to a "
                               "cuda device (there is no CPU fallback)")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise RuntimeError("FineTuneSession is single-process: data-parallel fine-tuning is not served "
                               f"(the process group has {dist.get_world_size()} ranks)")
        self.lr, self.max_grad_norm, self.betas, self.eps = float(lr), float(max_grad_norm), tuple(betas), float(eps)
        self.weight_decay, self.trainable = float(weight_decay), trainable
        super().__init__(model, batch, hw, dtype, graph, debug)

    # ------------------------------------------------------------------ construction
    def _plan(self) -> None:
        self.state = _opt_state(self.model)  # before the first fold: it re-homes the parameters
        self.flat = self.state.flat
        super()._plan()
        L, dt, N, B = self.L, self.dt, self.N, self.batch
        H1, W1 = self.stem_hw
        D, R = self.n_cams * self.rdim, self.rdim
        names = [s[0] for s in self.flat.slots]
        h0 = names.index("resnet.fc.weight")
        if any(not n.startswith(HEAD) for n in names[h0:]) or any(n.startswith(HEAD) for n in names[:h0]):
            raise RuntimeError("FineTuneSession: the head parameters must be the last slots of the flat buffer")
        # what Adam steps over: everything, or a suffix of the flat buffer (model order: a stage's first
        # parameter follows the last one of the stage before it, the head follows layer4)
        first = {"all": names[0], "head": "resnet.fc.weight"}.get(self.trainable,
                                                                  f"resnet.{self.trainable}.0.conv1.weight")
        self.opt_begin = self.flat.offset[first]
        self.opt_count = self.flat.total - self.opt_begin
        # the blocks the backward visits: schedule[first_block:], none for "head"; the stem only under "all"
        self.first_block = len(self.schedule)
        if self.trainable != "head":
            self.first_block = next(i for i, (c1, *_) in enumerate(self.schedule) if c1.name + ".weight" == first) \
                if self.trainable in STAGES else 0
        self.train_convs = [cv for blk in self.schedule[self.first_block:] for cv in blk if cv is not None]
        trained = {cv.name for cv in self.train_convs} | {cv.bn for cv in self.train_convs}
        i0 = names.index(first)
        if self.trainable in STAGES and (
                any(n.rsplit(".", 1)[0] not in trained and not n.startswith(HEAD) for n in names[i0:]) or
                any(n.rsplit(".", 1)[0] in trained for n in names[:i0])):
            raise RuntimeError(f"FineTuneSession: {self.trainable} and everything behind it must be the last slots "
                               f"of the flat buffer")
        self.norm = self._empty(1, dtype=torch.float32)
        self.norm_ws = self._empty(max(L.dll.argus_sumsq_workspace_bytes(self.opt_count), 16), dtype=torch.uint8)
        hws = max(L.dll.argus_gemm_f32_workspace_bytes(*s) for s in
                  [(6, 128, B), (128, 128, B), (128, D, B), (R, 2048, N)])
        if hws > self.gemm_ws.numel():
            self.gemm_ws = self._empty(hws, dtype=torch.uint8)
        # by kind; their sum is launches_per_step. head: the three GELU-backward GEMMs and the eight gradients
        self.launch_plan = {"forward": self.launches_per_forward, "loss": 1, "head": 3 + 8, "norm": 1, "adam": 1}
        self.launches_per_step = sum(self.launch_plan.values())
        self.launches_per_refold = 0
        self._fold_n = 0
        if self.trainable == "head":
            return
        ws_bytes, wg_bytes = self.ws.numel(), L.dll.argus_conv_wgrad_workspace_bytes(C.byref(self.stem_desc), dt)
        for cv in self.convs.values():
            d = cv.desc
            sp, mx, nb = C.c_int(0), C.c_int(0), C.c_size_t(0)
            L.bias_grad_plan(dt, d.n * d.ho * d.wo, d.k, 0, C.byref(sp), C.byref(mx), C.byref(nb))
            cv.db_splits = sp.value
            ws_bytes = max(ws_bytes, nb.value)
            wg_bytes = max(wg_bytes, L.dll.argus_conv_wgrad_workspace_bytes(C.byref(d), dt))
        if ws_bytes > self.ws.numel():  # (tickets zeroed once; every call leaves them zero)
            self.ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=self.device)
        self.wg_ws = self._empty(max(wg_bytes, 16), dtype=torch.uint8)
        # stem BN: the running mean and invstd for argus_maxpool_bwd_bn's partials, the finalize's workspace
        # (zeroed once) and its apply coefficients, which nobody reads
        self.stem_rows = L.dll.argus_maxpool_bwd_bn_rows(dt, N, H1, W1, 64)
        self.stem_invstd = self._empty(64, dtype=torch.float32)
        self.bn_ws = torch.zeros(L.dll.argus_bn_workspace_bytes(64), dtype=torch.uint8, device=self.device)
        self.stem_cabc = self._empty(3, 64, dtype=torch.float32)
        all_, n = self.trainable == "all", len(self.train_convs)
        n_ds = sum(1 for *_, ds in self.schedule[self.first_block:] if ds is not None)
        # the device table of argus_conv_fold_bn_batch / _bwd_batch over the trainable convs (filled by refresh)
        self._fold_n = n
        self._fold_table = torch.zeros(n * FOLD_ENTRY_BYTES, dtype=torch.uint8, device=self.device)
        # the stem copy and its BN coefficients (under "all"), one batched fold
        self.launches_per_refold = (2 if all_ else 0) + 1
        # the boundary block of a stage suffix launches no data gradient for conv1 and the downsample
        boundary = 0 if all_ else 1 + (self.schedule[self.first_block][3] is not None)
        self.launch_plan.update({
            "refold": self.launches_per_refold, "fc_dgrad": 1, "avgpool_bwd": 1, "dgrad": n - boundary,
            "wgrad": 2 * n,  # (+ its split reduce)
            "bias_grad": n - n_ds, "fold_bwd": n if self.debug is not None else 1,
            "stem": 4 if all_ else 0})  # max-pool backward, BN finalize, weight gradient (+ its reduce)
        self.launches_per_step = sum(self.launch_plan.values())

    def refresh(self) -> None:
        """Re-fold both weight copies from the masters; the head reads the masters themselves."""
        super().refresh()
        P = dict(self.model.named_parameters())
        Bf = dict(self.model.named_buffers())
        for n in HEAD:
            for k in ("weight", "bias"):
                self.head[n, k] = P[f"{n}.{k}"].detach()  # views of the flat buffer: never stale
        self.weight_bytes -= 4 * sum(t.numel() for t in self.head.values())
        eps = {n: m.eps for n, m in self.model.named_modules() if isinstance(m, nn.BatchNorm2d)}
        w = P["resnet.conv1.weight"]
        self._stem_master = (ptr(w), (C.c_int64 * 4)(*w.stride()))
        self._bn1 = (ptr(P["resnet.bn1.weight"]), ptr(P["resnet.bn1.bias"]), ptr(Bf["resnet.bn1.running_mean"]),
                     ptr(Bf["resnet.bn1.running_var"]), C.c_float(eps["resnet.bn1"]))
        self._masters = {}
        for cv in self.convs.values():
            w = P[cv.name + ".weight"]
            self._masters[cv.name] = (ptr(w), (C.c_int64 * 4)(*w.stride()), ptr(P[cv.bn + ".weight"]),
                                      ptr(P[cv.bn + ".bias"]), ptr(Bf[cv.bn + ".running_mean"]),
                                      ptr(Bf[cv.bn + ".running_var"]), C.c_float(eps[cv.bn]))
        if self.trainable == "all":
            with torch.no_grad():
                torch.rsqrt(Bf["resnet.bn1.running_var"] + eps["resnet.bn1"], out=self.stem_invstd)
        if self._fold_n:
            self._fill_fold_table()

    def _fill_fold_table(self) -> None:
        """The table of both batched fold entries from the recorded master pointers, into the device tensor the
        captured graphs read (its address never changes; the pointers in it only when the model was re-homed)."""
        G, n = self.flat.G, self._fold_n
        src = (FoldSrc * n)()
        ds_of = {ds.name: c3 for _, _, c3, ds in self.schedule if ds is not None}
        for e, cv in zip(src, self.train_convs):
            w, st, gamma, beta, rm, rv, eps = self._masters[cv.name]
            gw, gg, gb = G[cv.name + ".weight"], G[cv.bn + ".weight"], G[cv.bn + ".bias"]
            db = G[ds_of[cv.name].bn + ".bias"] if cv.name in ds_of else gb  # the downsample shares conv3's bias sum
            e.desc, e.w_master, e.strides = cv.desc, w, C.cast(st, C.POINTER(C.c_int64))
            e.gamma, e.beta, e.running_mean, e.running_var, e.eps = gamma, beta, rm, rv, eps.value
            e.w_fold, e.bias, e.w_fold_dgrad = ptr(cv.wf), ptr(cv.bias), ptr(cv.wfd)
            e.dwf, e.dw, e.db, e.dgamma, e.dbeta = ptr(gw), ptr(gw), ptr(db), ptr(gg), ptr(gb)
        host = torch.zeros(n * FOLD_ENTRY_BYTES, dtype=torch.uint8)
        nf, nb = C.c_int(0), C.c_int(0)
        self.L.conv_fold_bn_table(n, src, host.data_ptr(), host.numel(), C.byref(nf), C.byref(nb))
        self._fold_blocks, self._fold_bwd_blocks = nf.value, nb.value
        self._fold_table.copy_(host)

    def _refold(self) -> None:
        """refresh()'s launches from the recorded master pointers: capturable, nothing else."""
        L, dt, s = self.L, self.dt, stream()
        if self.trainable == "all":
            L.conv_weight_prep(C.byref(self.stem_desc), dt, *self._stem_master, ptr(self.stem_wf), None, s)
            L.bn_eval_coeffs(64, *self._bn1, ptr(self.stem_coef[0]), ptr(self.stem_coef[1]), s)
        L.conv_fold_bn_batch(dt, self._fold_n, ptr(self._fold_table), self._fold_blocks, s)

    # ------------------------------------------------------------------ parameter gradients
    def _head_grads(self, dpred: torch.Tensor) -> None:
        """ResNetEngine.backward's head_wgrads on this session's buffers."""
        L, s, N, B = self.L, stream(), self.N, self.batch
        D, R, G = self.n_cams * self.rdim, self.rdim, self.flat.G
        ws, wsn = ptr(self.gemm_ws), self.gemm_ws.numel()
        L.gemm_f32(6, 128, B, ptr(dpred), 6, 1, ptr(self.g2), 128, 0, ptr(G["output_mlp.4.weight"]), 128, None, 0,
                   None, ws, wsn, s)
        L.colsum_f32(B, 6, ptr(dpred), 6, ptr(G["output_mlp.4.bias"]), s)
        L.gemm_f32(128, 128, B, ptr(self.dh2), 128, 1, ptr(self.g1), 128, 0, ptr(G["output_mlp.2.weight"]), 128, None,
                   0, None, ws, wsn, s)
        L.colsum_f32(B, 128, ptr(self.dh2), 128, ptr(G["output_mlp.2.bias"]), s)
        L.gemm_f32(128, D, B, ptr(self.dh1), 128, 1, ptr(self.g0), D, 0, ptr(G["output_mlp.0.weight"]), D, None, 0,
                   None, ws, wsn, s)
        L.colsum_f32(B, 128, ptr(self.dh1), 128, ptr(G["output_mlp.0.bias"]), s)
        L.gemm_f32(R, 2048, N, ptr(self.dh0), R, 1, ptr(self.feat), 2048, 0, ptr(G["resnet.fc.weight"]), 2048, None, 0,
                   None, ws, wsn, s)
        L.colsum_f32(N, R, ptr(self.dh0), R, ptr(G["resnet.fc.bias"]), s)
        if self.debug is not None:
            for n in HEAD:
                for k in ("weight", "bias"):
                    self._keep(f"head.grad.{n}.{k}", G[f"{n}.{k}"])

    def _conv_grads(self, cv, x, dm, s, db_from=None) -> None:
        """dL/d(w_fold) and dL/d(bias) of the folded conv ``cv`` from its input ``x`` and masked output gradient
        ``dm``, into the flat slots of (w, beta). ``db_from``: the BN whose beta slot already holds sum(dm) (the
        downsample shares conv3's dm). The fold's derivative then turns them into the gradients of (w, gamma,
        beta) in place: one batched launch for all convs after the block loop, or here, per conv, under
        ``debug`` (which keeps dL/d(w_fold) before it and the three gradients after it)."""
        L, dt, d, G = self.L, self.dt, cv.desc, self.flat.G
        gw, gg, gb = G[cv.name + ".weight"], G[cv.bn + ".weight"], G[cv.bn + ".bias"]
        L.conv_wgrad(C.byref(d), dt, ptr(x), None, None, ptr(dm), ptr(gw), ptr(self.wg_ws), self.wg_ws.numel(), s)
        self._keep("wgrad." + cv.name, gw)
        db = gb
        if db_from is None:
            L.bias_grad(dt, d.n * d.ho * d.wo, d.k, ptr(dm), ptr(gb), cv.db_splits, ptr(self.ws), self.ws.numel(), s)
        else:
            db = G[db_from + ".bias"]
        self._keep("dbias." + cv.name, db)
        if self.debug is None:
            return
        w, st, gamma, _, rm, rv, eps = self._masters[cv.name]
        L.conv_fold_bn_bwd(C.byref(d), w, st, gamma, rm, rv, eps, ptr(gw), ptr(db), ptr(gw), ptr(gg), ptr(gb), s)
        self.debug["fold_bwd." + cv.name] = (gw.clone(), gg.clone(), gb.clone())

    def _backward_params(self, dpred: torch.Tensor) -> None:
        """GradientSession._backward's launches with every parameter gradient issued while its operands are alive
        (trainable "head": the head's data path down to dh0 and its eight gradients, nothing else)."""
        L, dt, s, N, B = self.L, self.dt, stream(), self.N, self.batch
        D, R, G = self.n_cams * self.rdim, self.rdim, self.flat.G
        hd, ws, wsn = self.head, ptr(self.gemm_ws), self.gemm_ws.numel()
        w0, w2, w4 = hd["output_mlp.0", "weight"], hd["output_mlp.2", "weight"], hd["output_mlp.4", "weight"]
        L.gemm_f32(B, 128, 6, ptr(dpred), 6, 0, ptr(w4), 128, 0, ptr(self.dh2), 128, None, 3, ptr(self.h2), ws, wsn, s)
        self._keep("head.dh2", self.dh2)
        L.gemm_f32(B, 128, 128, ptr(self.dh2), 128, 0, ptr(w2), 128, 0, ptr(self.dh1), 128, None, 3, ptr(self.h1), ws,
                   wsn, s)
        self._keep("head.dh1", self.dh1)
        L.gemm_f32(B, D, 128, ptr(self.dh1), 128, 0, ptr(w0), D, 0, ptr(self.dh0), D, None, 3, ptr(self.h0), ws, wsn, s)
        self._keep("head.dh0", self.dh0)
        self._head_grads(dpred)
        if self.trainable == "head":
            return
        L.gemm_f32(N, 2048, R, ptr(self.dh0), R, 0, ptr(hd["resnet.fc", "weight"]), 2048, 0, ptr(self.dfeat), 2048,
                   None, 0, None, ws, wsn, s)
        self._keep("head.dfeat", self.dfeat)
        dm3, dm2, dm1, dd, dx = self.pool
        hf, wf = self.final_hw
        last = self.acts[-1][2]
        L.avgpool_bwd_relu(dt, N, hf * wf, 2048, ptr(self.dfeat), ptr(last), ptr(dm3), s)
        self._keep("bwd.avgpool", dm3, last.shape)
        all_ = self.trainable == "all"
        for i in range(len(self.schedule) - 1, self.first_block - 1, -1):
            c1, c2, c3, ds = self.schedule[i]
            a1, a2, _ = self.acts[i]
            h = self.acts[i - 1][2] if i else self.p0
            pf = c1.name[:-len(".conv1")]
            self._dgrad(c3, dm3, None, a2, dm2, s, f"bwd.{pf}.conv3")
            self._dgrad(c2, dm2, None, a1, dm1, s, f"bwd.{pf}.conv2")
            if all_ or i > self.first_block:  # (nobody reads the block input's gradient below a stage suffix)
                addend = dm3
                if ds is not None:
                    self._dgrad(ds, dm3, None, None, dd, s, f"bwd.{pf}.downsample")
                    addend = dd
                self._dgrad(c1, dm1, addend, h, dx, s, f"bwd.{pf}.conv1")
            # dm3, dm2, dm1 and the saved a2, a1, h are all alive until the rotation below
            self._conv_grads(c3, a2, dm3, s)
            self._conv_grads(c2, a1, dm2, s)
            self._conv_grads(c1, h, dm1, s)
            if ds is not None:
                self._conv_grads(ds, h, dm3, s, db_from=c3.bn)
            dm3, dx = dx, dm3
        if self.debug is None:  # the fold's derivative of every trainable conv, in place in the flat slots
            L.conv_fold_bn_bwd_batch(self._fold_n, ptr(self._fold_table), self._fold_bwd_blocks, s)
        if not all_:
            return
        # stem: the max-pool backward through bn1's ReLU with the running mean / invstd, so that its partials are
        # {sum dm0, sum dm0 * xhat} = (dbeta, dgamma) of the eval-mode BN; then conv1's gradient of scale * dm0
        H1, W1 = self.stem_hw
        dm0 = dm2
        mean = self._bn1[2]
        L.maxpool_bwd_bn(dt, N, H1, W1, 64, ptr(dm3), ptr(self.amax), ptr(dm0), ptr(self.y0), ptr(self.stem_coef[0]),
                         ptr(self.stem_coef[1]), mean, ptr(self.stem_invstd), ptr(self.mp_part), s)
        self._keep("bwd.maxpool", dm0, self.y0.shape)
        L.bn_bwd_finalize(64, self.stem_rows, ptr(self.mp_part), N * H1 * W1, self._bn1[0], mean,
                          ptr(self.stem_invstd), ptr(G["resnet.bn1.weight"]), ptr(G["resnet.bn1.bias"]),
                          ptr(self.stem_cabc[0]), ptr(self.stem_cabc[1]), ptr(self.stem_cabc[2]), ptr(self.bn_ws), s)
        ap = BnBwdPrologue(ptr(self.y0), ptr(self.stem_coef[0]), ptr(self.zero64), ptr(self.zero64), None)
        L.conv_wgrad_apply(C.byref(self.stem_desc), dt, ptr(self.x0), ptr(dm0), C.byref(ap),
                           ptr(G["resnet.conv1.weight"]), ptr(self.wg_ws), self.wg_ws.numel(), s)
        if self.debug is not None:
            for n in ("resnet.conv1.weight", "resnet.bn1.weight", "resnet.bn1.bias"):
                self._keep("stem.grad." + n, G[n])

    # ------------------------------------------------------------------ public
    def _replay(self, key: str, fn) -> None:
        """``fn()`` eagerly, or captured once under ``key`` and replayed (a graph without an image input)."""
        with torch.cuda.device(self.device), torch.no_grad():
            if not self.graph:
                fn()
                return
            g = self._graphs.get(key)
            if g is None:
                side = torch.cuda.Stream(self.device)
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    fn()
                torch.cuda.current_stream().wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fn()
                self._graphs[key] = g
            g.replay()

    def step(self, images: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """One optimisation step on ``images`` (as ``session(images)`` takes them) towards ``target`` (batch, 7)
        poses; returns the per-sample losses (batch,) of the forward before the update, a fresh tensor. The
        gradient stays in ``session.flat.grad``, its norm before clipping in ``session.norm``."""
        self._check_images(images, "step")
        if not isinstance(target, torch.Tensor) or tuple(target.shape) != (self.batch, 7) or \
                not target.is_floating_point():
            raise ValueError(f"FineTuneSession.step expects a floating target of shape {(self.batch, 7)}")
        if self.model.training:
            raise RuntimeError("FineTuneSession.step needs model.eval(): it is the eval-mode function that is "
                               "trained (FusedTrainer.step is the train-mode step)")
        if not self.state.owns(self.model):
            raise RuntimeError("FineTuneSession: the model's parameters were re-homed after this session was built")
        self.target.copy_(target)
        L, flat, st = self.L, self.flat, self.state
        folds = self.trainable != "head"

        def body(x):
            if folds:
                self._refold()
            self._forward(x)
            L.se3_loss(self.batch, ptr(self.pred), ptr(self.target), ptr(self.loss), ptr(self.dpred),
                       C.c_float(1.0 / self.batch), stream())
            self._backward_params(self.dpred)
            L.global_norm(self.opt_count, ptr(flat.grad) + 4 * self.opt_begin, ptr(self.norm), ptr(self.norm_ws),
                          stream())

        self._run("step", images, body)
        st.step_count += 1
        b1, b2 = self.betas
        t, o = st.step_count, 4 * self.opt_begin
        with torch.cuda.device(self.device), torch.no_grad():
            L.adam_step(self.opt_count, ptr(flat.param) + o, ptr(flat.grad) + o, ptr(st.exp_avg) + o,
                        ptr(st.exp_avg_sq) + o, ptr(self.norm), C.c_float(1.0), C.c_float(self.max_grad_norm),
                        C.c_float(self.lr), C.c_float(b1), C.c_float(b2), C.c_float(self.eps),
                        C.c_float(self.weight_decay), C.c_float(1 - b1**t), C.c_float(1 - b2**t), stream())
        if folds:  # the head reads the masters; the folded copies follow them
            self._replay("refold", self._refold)
        return self.loss.clone()

    def grad_norm(self) -> torch.Tensor:
        """Total gradient norm of the last step, before clipping."""
        return self.norm.clone()


class FrozenTrainer:
    """``FusedTrainer``'s ``step`` / ``lr`` seam over fine-tune sessions (``train --freeze-bn``): one
    ``FineTuneSession`` per batch shape met (the last, partial batch of an epoch gets its own), all on the model's
    one optimizer state; ``lr`` (what ``PlateauScheduler`` drives) is handed to the session at every step."""

    def __init__(self, model: NCameraCNN, lr: float = 1e-4, max_grad_norm: float = 1.0, **session_kw):
        self.model, self.lr, self.max_grad_norm, self.session_kw = model, lr, max_grad_norm, session_kw
        self.sessions: dict = {}

    def step(self, images: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        key = (images.shape[0], images.shape[2], images.shape[3])
        session = self.sessions.get(key)
        if session is None:
            session = FineTuneSession(self.model, key[0], key[1:], lr=self.lr, max_grad_norm=self.max_grad_norm,
                                      **self.session_kw)
            self.sessions[key] = session
        session.lr = self.lr
        return session.step(images, targets.float())
