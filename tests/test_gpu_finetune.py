"""GPU: FineTuneSession, one optimisation step of the eval-mode function (frozen BatchNorm statistics).

Reference: oracle.ncamera in .eval() under CPU autograd, clip_grad_norm_ and torch.optim.Adam, which is what the
reference does with model.eval() + loss.backward() + Adam.step() (argus/models.py:66-90, argus/train.py:298-321).

Bars. Stage checks compare every parameter-gradient launch with an fp64 re-derivation from the GPU tensors that
launch reads, at test_gpu_frozen_grad.py's STAGE bars relative to the maximum (2e-5 fp32, 1e-2 bf16) for the GEMM
shaped ones (conv, stem and head weight gradients); column sums (bn1's dgamma / dbeta, the head biases) at the same
STAGE figure times the sum of the magnitudes of their terms, because a sum of mixed signs can be far smaller than
its terms; argus_bias_grad and argus_conv_fold_bn_bwd at their kernel bars (test_gpu_finetune_kernels.py), which
do not depend on the compute dtype: their inputs are exact. The whole gradient against the fp64 oracle is a
gross-error check as in test_gpu_frozen_grad.py (a deep random ReLU net is chaotic in its masks): the bar is twice
the CPU reference's own bf16-autocast distance from its fp32 gradient, per parameter group.
"""
import copy

import pytest
import torch
import torch.nn as nn

from argus_amd.finetune import FineTuneSession
from argus_amd.profiling import KernelTimer

pytestmark = pytest.mark.gpu

STAGE = {"fp32": 2e-5, "bf16": 1e-2}
KERNEL = 2e-5
HEAD = ("resnet.fc", "output_mlp.0", "output_mlp.2", "output_mlp.4")
LR = 1e-4


def _randomize_bn(model):
    """tests/test_gpu_infer.py's recipe: non-trivial BN parameters and running statistics from one generator."""
    g = torch.Generator().manual_seed(7)
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            c = m.num_features
            m.weight.data = 0.5 + torch.rand(c, generator=g)
            m.bias.data = 0.1 * torch.randn(c, generator=g)
            m.running_mean.data = 0.1 * torch.randn(c, generator=g)
            m.running_var.data = 0.5 + torch.rand(c, generator=g)


@pytest.fixture(scope="module")
def oracle():
    from oracle.ncamera import build_reference_model

    ref = build_reference_model(42)
    _randomize_bn(ref)
    return ref.eval()


def _images(hw, seed=1234, batch=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (batch, 6, *hw), generator=g, dtype=torch.uint8)


def _target(batch=2):
    from oracle.se3 import random_targets

    return random_targets(batch, torch.Generator().manual_seed(3), sigma=0.3)


def _product(oracle, cuda, dtype):
    from argus_amd.models import NCameraCNN

    m = NCameraCNN(compute_dtype=dtype)
    m.load_state_dict(oracle.state_dict())
    return m.to(cuda).eval()


def _groups(model):
    """name -> group of every parameter: conv weights, BN gamma, BN beta, head."""
    bn = {n for n, m in model.named_modules() if isinstance(m, nn.BatchNorm2d)}
    out = {}
    for n, p in model.named_parameters():
        mod, leaf = n.rsplit(".", 1)
        out[n] = "head" if mod in HEAD else "conv" if p.dim() == 4 else "gamma" if leaf == "weight" else "beta"
        assert out[n] in ("head", "conv") or mod in bn
    return out


def _f64(t):
    return t.detach().double().cpu()


def _rel_max(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---- stages -------------------------------------------------------------------------------------------------
def _dw64(d, x, dm):
    """dL/d(w_fold) [k][r*s*c] of conv ``d`` from NHWC x (n, h, w, c) and dm (n, ho, wo, k), fp64."""
    g = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2).contiguous(), (d.k, d.c, d.r, d.s),
                                    dm.permute(0, 3, 1, 2).contiguous(), stride=d.stride, padding=d.pad)
    return g.permute(0, 2, 3, 1).reshape(d.k, -1)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("hw", [(64, 64), (72, 104)], ids=["64x64", "72x104"])
def test_stage_by_stage(cuda, oracle, dt, hw):
    model = _product(oracle, cuda, dt)
    s = FineTuneSession(model, 2, hw, lr=0.0, debug=True)
    assert s.graph is False
    x = (_images(hw).float() / 255.0).to(cuda)
    for _, _, o, k in s.flat.slots:  # (the alignment padding between slots stays zero: the norm reads it)
        s.flat.grad[o:o + k] = float("nan")
    s.step(x, _target().to(cuda))
    assert not torch.isnan(s.flat.grad).any()  # every slot was written by a kernel
    dbg = s.debug
    P, Bf = dict(model.named_parameters()), dict(model.named_buffers())
    eps = {n: m.eps for n, m in model.named_modules() if isinstance(m, nn.BatchNorm2d)}
    N, B, D, R = s.N, s.batch, s.n_cams * s.rdim, s.rdim
    worst = {"wgrad": 0.0, "dbias": 0.0, "dw": 0.0, "dgamma": 0.0, "stem": 0.0, "head": 0.0, "sums": 0.0}

    def conv_stage(cv, xin, dm):
        d = cv.desc
        xin, dm = _f64(xin), dm.reshape(d.n, d.ho, d.wo, d.k)
        dwf = _f64(dbg["wgrad." + cv.name]).view(d.k, -1)
        worst["wgrad"] = max(worst["wgrad"], _rel_max(dwf, _dw64(d, xin, dm)) / STAGE[dt])
        assert _rel_max(dwf, _dw64(d, xin, dm)) <= STAGE[dt], cv.name
        db = _f64(dbg["dbias." + cv.name])
        mag = dm.abs().sum((0, 1, 2))
        e = (db - dm.sum((0, 1, 2))).abs()
        worst["dbias"] = max(worst["dbias"], float((e / mag.clamp_min(1e-300)).max()) / KERNEL)
        assert bool((e <= KERNEL * mag).all()), cv.name
        dw, dg, dbe = (_f64(t) for t in dbg["fold_bwd." + cv.name])
        w = _f64(P[cv.name + ".weight"]).permute(0, 2, 3, 1).reshape(d.k, -1)
        gamma, rm, rv = _f64(P[cv.bn + ".weight"]), _f64(Bf[cv.bn + ".running_mean"]), _f64(Bf[cv.bn + ".running_var"])
        inv = 1.0 / torch.sqrt(rv + eps[cv.bn])
        rw = dwf * (gamma * inv)[:, None]
        worst["dw"] = max(worst["dw"], _rel_max(dw.view(d.k, -1), rw) / KERNEL)
        assert _rel_max(dw.view(d.k, -1), rw) <= KERNEL, cv.name
        rg = inv * ((dwf * w).sum(1) - rm * db)
        gmag = inv * ((dwf * w).abs().sum(1) + (rm * db).abs())
        worst["dgamma"] = max(worst["dgamma"], float(((dg - rg).abs() / gmag.clamp_min(1e-300)).max()) / KERNEL)
        assert bool(((dg - rg).abs() <= KERNEL * gmag).all()), cv.name
        assert torch.equal(dbe, db), cv.name
        # and that is what the flat gradient holds
        assert torch.equal(_f64(P[cv.name + ".weight"].grad).permute(0, 2, 3, 1).reshape(d.k, -1), dw.view(d.k, -1))
        assert torch.equal(_f64(P[cv.bn + ".weight"].grad), dg) and torch.equal(_f64(P[cv.bn + ".bias"].grad), dbe)

    dm3 = _f64(dbg["bwd.avgpool"])
    for i in range(len(s.schedule) - 1, -1, -1):
        c1, c2, c3, ds = s.schedule[i]
        a1, a2, _ = s.acts[i]
        h = s.acts[i - 1][2] if i else s.p0
        pf = c1.name[:-len(".conv1")]
        conv_stage(c3, a2, dm3)
        conv_stage(c2, a1, _f64(dbg[f"bwd.{pf}.conv3"]))
        conv_stage(c1, h, _f64(dbg[f"bwd.{pf}.conv2"]))
        if ds is not None:
            conv_stage(ds, h, dm3)
        dm3 = _f64(dbg[f"bwd.{pf}.conv1"])
    # the stem: conv1's gradient of scale * dm0 over the staged images, bn1's sums of dm0 and dm0 * xhat
    dm0, y0 = _f64(dbg["bwd.maxpool"]), _f64(s.y0)
    scale = _f64(s.stem_coef[0])
    H, W = s.hw
    x0 = _f64(s.x0)[..., :3].permute(0, 3, 1, 2).contiguous()
    ref = torch.nn.grad.conv2d_weight(x0, (64, 3, 7, 7), (dm0 * scale).permute(0, 3, 1, 2).contiguous(), stride=2,
                                      padding=3)
    got = _f64(P["resnet.conv1.weight"].grad)
    worst["stem"] = _rel_max(got, ref) / STAGE[dt]
    assert _rel_max(got, ref) <= STAGE[dt]
    rm, rv = _f64(Bf["resnet.bn1.running_mean"]), _f64(Bf["resnet.bn1.running_var"])
    xhat = (y0 - rm) / torch.sqrt(rv + eps["resnet.bn1"])
    for name, terms in (("resnet.bn1.weight", dm0 * xhat), ("resnet.bn1.bias", dm0)):
        e = (_f64(P[name].grad) - terms.sum((0, 1, 2))).abs()
        mag = terms.abs().sum((0, 1, 2))
        worst["sums"] = max(worst["sums"], float((e / mag.clamp_min(1e-300)).max()) / STAGE[dt])
        assert bool((e <= STAGE[dt] * mag).all()), name
    # the head: eight gradients from the activations and cotangents the session kept
    dp, dh2, dh1, dh0 = _f64(s.dpred), _f64(dbg["head.dh2"]), _f64(dbg["head.dh1"]), _f64(dbg["head.dh0"]).view(N, R)
    g2, g1, g0, feat = _f64(s.g2), _f64(s.g1), _f64(s.g0).view(B, D), _f64(s.feat)
    for name, dy, act in (("output_mlp.4", dp, g2), ("output_mlp.2", dh2, g1), ("output_mlp.0", dh1, g0),
                          ("resnet.fc", dh0, feat)):
        gw, gb = _f64(P[name + ".weight"].grad), _f64(P[name + ".bias"].grad)
        worst["head"] = max(worst["head"], _rel_max(gw, dy.t() @ act) / STAGE[dt])
        assert _rel_max(gw, dy.t() @ act) <= STAGE[dt], name
        e, mag = (gb - dy.sum(0)).abs(), dy.abs().sum(0)
        worst["sums"] = max(worst["sums"], float((e / mag.clamp_min(1e-300)).max()) / STAGE[dt])
        assert bool((e <= STAGE[dt] * mag).all()), name
    print(f"finetune stages {dt} {hw}: worst error / bar = " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- the whole gradient, the optimizer, the trajectory --------------------------------------------------------
def _oracle_step_grads(model, x, target, autocast=False):
    """name -> d(mean loss)/d(parameter) of the eval-mode oracle under CPU autograd, and the per-sample losses."""
    from oracle.se3 import geometric_loss

    model.zero_grad(set_to_none=True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        pred = model(x)
    losses = geometric_loss(pred.to(x.dtype), target.to(x.dtype))
    losses.mean().backward()
    return {n: p.grad.detach().double().clone() for n, p in model.named_parameters()}, losses.detach().double()


@pytest.fixture(scope="module")
def oracle_param_grads(oracle):
    """hw -> (g64, d_ref per group, d32 per group): computed once per size, shared, never modified."""
    cache = {}

    def dist(a, b, names):
        num = sum(float((a[n] - b[n]).pow(2).sum()) for n in names)
        return (num / sum(float(b[n].pow(2).sum()) for n in names)) ** 0.5

    def get(hw):
        if hw not in cache:
            x, T = _images(hw).float() / 255.0, _target()
            m32 = copy.deepcopy(oracle).eval()
            g64, _ = _oracle_step_grads(copy.deepcopy(oracle).double().eval(), x.double(), T.double())
            g32, _ = _oracle_step_grads(m32, x, T)
            g16, _ = _oracle_step_grads(m32, x, T, autocast=True)
            groups = _groups(oracle)
            d_ref, d32 = {}, {}
            for grp in ("conv", "gamma", "beta", "head"):
                names = [n for n, v in groups.items() if v == grp]
                d_ref[grp], d32[grp] = dist(g16, g32, names), dist(g32, g64, names)
            cache[hw] = (g64, d_ref, d32, dist)
        return cache[hw]

    return get


@pytest.mark.parametrize("hw", [(64, 64), (72, 104)], ids=["64x64", "72x104"])
def test_gradient_matches_the_fp64_oracle(cuda, oracle, oracle_param_grads, hw):
    """A gross-error check: relative L2 distance of flat.grad from the oracle's fp64 eval-mode autograd per parameter
    group, bar 2 * d_ref (d_ref: the CPU reference's bf16-autocast distance from its fp32 gradient; 2 * d_ref < 1 keeps
    a zero or sign-flipped gradient out). Measured on an MI355X, 64x64: fp32 3.0e-6 .. 4.0e-6, bf16 0.20 / 0.22 / 0.25 /
    0.032 against d_ref 0.233 / 0.256 / 0.340 / 0.056 (conv / gamma / beta / head); 72x104: fp32 3.2e-6 .. 6.7e-4 (ReLU
    masks across zero), bf16 0.10 / 0.090 / 0.073 / 0.020 against 0.118 / 0.106 / 0.082 / 0.051."""
    g64, d_ref, d32, dist = oracle_param_grads(hw)
    groups = _groups(oracle)
    x, T = (_images(hw).float() / 255.0).to(cuda), _target().to(cuda)
    for dt in ("fp32", "bf16"):
        model = _product(oracle, cuda, dt)
        s = FineTuneSession(model, 2, hw, lr=0.0)
        s.step(x, T)
        got = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters()}
        for grp in ("conv", "gamma", "beta", "head"):
            names = [n for n, v in groups.items() if v == grp]
            e = dist(got, g64, names)
            print(f"finetune gradient vs fp64 oracle {hw} {dt} {grp}: e = {e:.3e}, d_ref = {d_ref[grp]:.3f} "
                  f"(CPU fp32 reference: {d32[grp]:.1e})")
            assert 2 * d_ref[grp] < 1, (grp, d_ref[grp])
            assert e <= 2 * d_ref[grp], (dt, hw, grp, e, d_ref[grp])


@pytest.mark.parametrize("trainable", ["all", "head"])
def test_step_is_clip_and_adam_of_its_own_gradient(cuda, oracle, trainable):
    hw = (64, 64)
    model = _product(oracle, cuda, "fp32")
    s = FineTuneSession(model, 2, hw, lr=LR, max_grad_norm=1.0, trainable=trainable)
    before = s.flat.param.clone()
    x, T = _images(hw).to(cuda), _target().to(cuda)
    for t in (1, 2):
        p0 = s.flat.param.double().cpu()
        m0, v0 = s.state.exp_avg.double().cpu(), s.state.exp_avg_sq.double().cpu()
        s.step(x, T)
        g = s.flat.grad.double().cpu()
        o = s.opt_begin
        norm = g[o:].norm()
        assert abs(float(s.norm) - float(norm)) <= 1e-6 * float(norm) and float(norm) > 1.0  # clipping is active
        gc = g * min(1.0, 1.0 / (float(norm) + 1e-6))
        m, v = 0.9 * m0 + 0.1 * gc, 0.999 * v0 + 0.001 * gc * gc
        ref = p0 - LR * (m / (1 - 0.9 ** t)) / ((v / (1 - 0.999 ** t)).sqrt() + 1e-8)
        got = s.flat.param.double().cpu()
        assert float((got[o:] - ref[o:]).abs().max()) < 2e-6  # tests/test_gpu_kernels.py::test_norm_and_adam's
        assert torch.equal(got[:o], p0[:o])
    assert not torch.equal(s.flat.param[s.opt_begin:], before[s.opt_begin:])


def _cpu_trajectory(model, x, T, steps):
    """Per step, the per-sample losses (batch,) in double of the eval-mode oracle under clip 1.0 + Adam lr 1e-4."""
    from oracle.se3 import geometric_loss

    opt = torch.optim.Adam(model.parameters(), lr=LR, betas=(0.9, 0.999), eps=1e-8)
    out = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        losses = geometric_loss(model(x), T)
        losses.mean().backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        out.append(losses.detach().double())
    return out


def test_fp32_trajectory_follows_the_fp64_oracle(cuda, oracle):
    """Three steps on one fixed batch; the losses step() returns, (batch,) per step, against the fp64 oracle under the
    same recipe (eval mode, clip 1.0, Adam lr 1e-4) on the CPU: at every step the deviation max_i |loss_i - fp64_i| is
    within twice the CPU fp32 reference's own deviation at that step.

    The deviation is taken over the per-sample losses, not over their mean. An earlier version compared the batch means
    and failed at step 0, and the measurement showed why that metric is wrong: the per-sample errors have opposite
    signs and cancel in the mean by chance (CPU fp32 reference +2.74e-5 and -2.89e-5, mean -7.7e-7; session +2.17e-5
    and -3.27e-5, mean -5.5e-6), so the reference's "deviation" came out 35 times smaller than its actual error and
    below one fp32 ulp of the loss (1.9e-6 at 21.6), while the session's prediction at step 0 is closer to fp64 than
    the reference's (max |pred - fp64| 4.9e-6 against 8.0e-6). The means are still printed.

    Measured on an MI355X (session deviation / CPU fp32 reference deviation): step 0 3.3e-5 / 2.9e-5, step 1 2.1e-3 /
    2.2e-2, step 2 1.4e-4 / 3.4e-3."""
    hw = (64, 64)
    x, T = _images(hw).float() / 255.0, _target()
    l64 = _cpu_trajectory(copy.deepcopy(oracle).double().eval(), x.double(), T.double(), 3)
    l32 = _cpu_trajectory(copy.deepcopy(oracle).eval(), x, T, 3)
    s = FineTuneSession(_product(oracle, cuda, "fp32"), 2, hw, lr=LR)
    got = [s.step(x.to(cuda), T.to(cuda)).double().cpu() for _ in range(3)]
    dev = [float((got[t] - l64[t]).abs().max()) for t in range(3)]
    ref = [float((l32[t] - l64[t]).abs().max()) for t in range(3)]
    for t in range(3):
        print(f"finetune trajectory step {t}: fp64 {l64[t].tolist()}, session dev {dev[t]:.2e}, CPU fp32 dev {ref[t]:.2e}; "
              f"means: fp64 {float(l64[t].mean()):.9f}, session {float(got[t].mean()):.9f}, CPU fp32 "
              f"{float(l32[t].mean()):.9f}")
    for t in range(3):
        assert dev[t] <= 2 * ref[t], (t, dev[t], ref[t])


def test_bf16_trajectory_descends_and_is_reproducible(cuda, oracle):
    hw = (64, 64)
    x, T = _images(hw).to(cuda), _target().to(cuda)
    runs = []
    for _ in range(2):
        s = FineTuneSession(_product(oracle, cuda, "bf16"), 2, hw, lr=LR)
        runs.append(torch.stack([s.step(x, T) for _ in range(3)]))
    a = runs[0]
    assert torch.isfinite(a).all() and float(a[-1].mean()) < float(a[0].mean()), a
    assert torch.equal(runs[0], runs[1])


# ---- semantics ------------------------------------------------------------------------------------------------
def test_session_semantics(cuda, oracle):
    from argus_amd.infer import InferenceSession
    from argus_amd.infer_grad import GradientSession

    hw = (64, 64)
    u8 = _images(hw, 1)
    xa = (u8.float() / 255.0).to(cuda)  # the division on the CPU
    u8, T = u8.to(cuda), _target().to(cuda)
    cot = torch.randn(2, 6, generator=torch.Generator().manual_seed(99)).to(cuda)

    def run(images, **kw):
        model = _product(oracle, cuda, "fp32")
        parent = GradientSession(model, 2, hw)
        parent_vjp = parent.vjp(xa, cot)  # the parent's contract, before any step
        parent_losses = parent.image_gradient(xa, T)[0]
        buffers = {k: v.clone() for k, v in model.named_buffers()}
        s = FineTuneSession(model, 2, hw, lr=LR, **kw)
        assert torch.equal(s.vjp(xa, cot), parent_vjp)
        losses = [s.step(images, T) for _ in range(2)]
        assert torch.equal(losses[0], parent_losses)  # the first step's forward and loss are the frozen session's
        assert not model.training
        after = dict(model.named_buffers())
        assert all(torch.equal(buffers[k], after[k]) for k in buffers) and "resnet.bn1.num_batches_tracked" in buffers
        assert "resnet.layer4.2.bn3.running_var" in buffers
        return model, s, torch.stack(losses), s.flat.param.clone()

    model, s, lg, pg = run(xa)
    # after step(), every served function sees the updated parameters
    fresh = InferenceSession(model, 2, hw)
    assert torch.equal(s(xa), fresh(xa)) and torch.equal(s.pose(xa), fresh.pose(xa))
    assert torch.equal(s.vjp(xa, cot), GradientSession(model, 2, hw).vjp(xa, cot))
    _, _, le, pe = run(xa, graph=False)
    assert torch.equal(le, lg) and torch.equal(pe, pg)  # graph == eager
    _, _, lu, pu = run(u8)
    assert torch.equal(lu, lg) and torch.equal(pu, pg)  # uint8 == its /255 float batch
    # lr is writable and read at every step
    s.lr = 0.0
    before = s.flat.param.clone()
    s.step(xa, T)
    assert torch.equal(s.flat.param, before)
    # refusals
    with pytest.raises(ValueError, match="shape"):
        s.step(xa[:1], T)
    with pytest.raises(ValueError, match="target"):
        s.step(xa, T[:, :6])
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        s.step(xa, T)
    model.eval()


def test_session_takes_over_an_existing_flat_buffer(cuda, oracle):
    """Parameters that are already views of a FlatParams (a FusedTrainer's) stay where they are: the session writes
    the trainer's own parameter and gradient buffers, with the gradient of a session that made its own."""
    from argus_amd.step import FusedTrainer

    hw = (64, 64)
    x, T = _images(hw).to(cuda), _target().to(cuda)
    model = _product(oracle, cuda, "fp32")
    trainer = FusedTrainer(model)
    s = FineTuneSession(model, 2, hw, lr=LR)
    assert s.flat.param.data_ptr() == trainer.flat.param.data_ptr() and s.flat.total == trainer.flat.total
    assert s.flat.grad.data_ptr() == trainer.flat.grad.data_ptr() and s.flat.offset == trainer.flat.offset
    own = FineTuneSession(_product(oracle, cuda, "fp32"), 2, hw, lr=LR)
    assert torch.equal(s.step(x, T), own.step(x, T))
    assert torch.equal(trainer.flat.grad, own.flat.grad) and torch.equal(trainer.flat.param, own.flat.param)
    assert FineTuneSession(model, 2, (72, 104)).state is s.state  # and later sessions share the optimizer state


def test_trainable_head_leaves_the_backbone_alone(cuda, oracle):
    hw = (64, 64)
    x, T = _images(hw).to(cuda), _target().to(cuda)
    barred = ("conv_infer_dgrad_kernel", "wgrad", "fold_bn_bwd", "bias_grad", "fold_bn_kernel")
    model = _product(oracle, cuda, "fp32")
    s = FineTuneSession(model, 2, hw, lr=LR, trainable="head", graph=False)
    before = s.flat.param.clone()
    o = s.opt_begin
    assert 0 < o == s.flat.offset["resnet.fc.weight"]
    with KernelTimer() as timer:
        losses = [s.step(x, T) for _ in range(3)]
    names = set(timer.summary())
    assert names and not [n for n in names if any(b in n for b in barred)], names
    assert torch.equal(s.flat.param[:o], before[:o]) and int((s.flat.grad[:o] != 0).sum()) == 0
    assert not torch.equal(s.flat.param[o:], before[o:])
    for n in ("resnet.fc.weight", "output_mlp.4.bias"):
        assert not torch.equal(s.flat.param[s.flat.offset[n]:s.flat.offset[n] + 6], before[s.flat.offset[n]:][:6]), n
    assert torch.isfinite(torch.stack(losses)).all()
    # the same timer does see those kernels when everything is trained
    s2 = FineTuneSession(_product(oracle, cuda, "fp32"), 2, hw, lr=LR, graph=False)
    with KernelTimer() as timer:
        s2.step(x, T)
    names = set(timer.summary())
    for b in ("conv_infer_dgrad_kernel", "wgrad", "fold_bn_bwd_kernel", "bias_grad_kernel"):
        assert any(b in n for n in names), (b, names)


# ---- CLI --------------------------------------------------------------------------------------------------------
def test_train_freeze_bn_from_a_checkpoint(cuda, tmp_path):
    """train(cfg) with --freeze-bn and --init-checkpoint, two epochs on tests/test_gpu_train.py's dummy dataset (10
    training samples at batch 4: a partial last batch, so two sessions on one optimizer state)."""
    from conftest import make_dummy_dataset

    from argus_amd.data import CameraCubePoseDatasetConfig
    from argus_amd.models import NCameraCNN, NCameraCNNConfig
    from argus_amd.train import TrainConfig, train

    data = make_dummy_dataset(tmp_path / "data", hw=(64, 64))
    torch.manual_seed(11)
    init = NCameraCNN()
    _randomize_bn(init)
    sd0 = {k: v.clone() for k, v in init.state_dict().items()}
    ckpt = tmp_path / "init.pth"
    torch.save({"module." + k: v for k, v in sd0.items()}, ckpt)  # a DDP checkpoint's keys
    saves = []
    for run in range(2):
        save = tmp_path / f"ckpt{run}"
        cfg = TrainConfig(batch_size=4, learning_rate=1e-4, n_epochs=2, device="cuda", max_grad_norm=1.0, random_seed=42,
                          val_epochs=1, print_epochs=1, save_epochs=1, save_dir=str(save),
                          model_config=NCameraCNNConfig(n_cams=2),
                          dataset_config=CameraCubePoseDatasetConfig(dataset_path=data, center_crop=(64, 64)),
                          compile_model=False, wandb_log=False, num_workers=0, init_checkpoint=str(ckpt),
                          freeze_bn=True)
        train(cfg)
        (pth,) = list(save.glob("*.pth"))
        saves.append(torch.load(pth, weights_only=True))
    sd1, sd2 = saves
    assert set(sd1) == set(sd0)
    buffers = [k for k in sd0 if "running_" in k or "num_batches_tracked" in k]
    assert len(buffers) == 3 * 53 and all(torch.equal(sd1[k], sd0[k]) for k in buffers)
    weights = [k for k in sd0 if k not in buffers]
    assert all(not torch.equal(sd1[k], sd0[k]) for k in weights)
    assert all(torch.equal(sd1[k], sd2[k]) for k in sd1)  # deterministic kernels: bit-identical reruns
