"""GPU: stage-wise frozen fine-tuning, ``FineTuneSession(trainable="layerK")``: ``resnet.layerK`` .. ``layer4``, the
fc and the MLP train, the stem and the earlier stages are frozen (``requires_grad_(False)`` on the prefix,
``model.eval()``, ``clip_grad_norm_`` and ``Adam`` over the trained parameters in stock PyTorch).

The recipes are tests/test_gpu_finetune.py's: the ``oracle.ncamera`` model with seed 42 and randomised BatchNorm,
its images and targets, B=2 at 64x64 (``layer3`` also at 72x104: ragged 9x13 / 5x7 / 3x4 grids). What is new is pinned
exactly: the frozen prefix is never written (bit patterns and sentinels), the suffix gradient equals the one a
``trainable="all"`` session computes bit for bit (the same launches and splits produce it; the batched fold-backward
against the per-conv one of a ``debug`` session), the launch schedule is counted, and the step is clip + Adam of its
own gradient over the suffix (test_step_is_clip_and_adam_of_its_own_gradient's check and its 2e-6 bar). Against the
fp64 oracle with the prefix frozen the bar is that file's gross-error bar, twice the CPU reference's own bf16-autocast
distance from its fp32 gradient, per parameter group over the trained parameters."""
import copy
import re

import pytest
import torch
import torch.nn as nn

from argus_amd.finetune import FineTuneSession
from argus_amd.profiling import KernelTimer

pytestmark = pytest.mark.gpu

HEAD = ("resnet.fc", "output_mlp.0", "output_mlp.2", "output_mlp.4")
STAGES = ("layer1", "layer2", "layer3", "layer4")
DGRADS = {"layer4": 8, "layer3": 27, "layer2": 40, "layer1": 50}
LR = 1e-4
HW = (64, 64)


def _randomize_bn(model):
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


def _first(stage):
    return f"resnet.{stage}.0.conv1.weight"


# ---- the frozen prefix ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("stage", STAGES)
def test_prefix_is_never_written_and_every_trained_slot_is(cuda, oracle, stage, dt):
    model = _product(oracle, cuda, dt)
    s = FineTuneSession(model, 2, HW, compute_dtype=dt, lr=LR, trainable=stage)
    o = s.opt_begin
    assert s.trainable == stage and 0 < o == s.flat.offset[_first(stage)] and s.opt_count == s.flat.total - o
    params0 = {n: p.detach().clone() for n, p in model.named_parameters()}
    buffers0 = {n: b.clone() for n, b in model.named_buffers()}
    st = s.state
    for t, v in ((s.flat.grad, 3.25), (st.exp_avg, -1.5), (st.exp_avg_sq, 7.75)):  # sentinels on the prefix
        t[:o] = v
    for n, _, off, k in s.flat.slots:  # (the alignment padding between slots stays zero: the norm reads it)
        if off >= o:
            s.flat.grad[off:off + k] = float("nan")
    x, T = _images(HW).to(cuda), _target().to(cuda)
    losses = torch.stack([s.step(x, T) for _ in range(3)])
    assert torch.isfinite(losses).all()
    assert bool((s.flat.grad[:o] == 3.25).all()) and bool((st.exp_avg[:o] == -1.5).all()) and \
        bool((st.exp_avg_sq[:o] == 7.75).all())
    assert not torch.isnan(s.flat.grad[o:]).any()  # every trained slot was written by a kernel
    names = [n for n, _ in model.named_parameters()]
    i0 = names.index(_first(stage))
    for i, (n, p) in enumerate(model.named_parameters()):
        assert torch.equal(p.detach(), params0[n]) == (i < i0), n  # the prefix bit-identical, every trained tensor moved
    after = dict(model.named_buffers())
    assert all(torch.equal(after[n], b) for n, b in buffers0.items()) and "resnet.bn1.num_batches_tracked" in after
    assert f"resnet.{stage}.0.bn1.running_var" in after and not model.training


# ---- the same gradient as "all" -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grad_of_all(cuda, oracle):
    """(dt, hw) -> flat.grad of one lr=0 step of a trainable="all" session: computed once, shared, never modified."""
    cache = {}

    def get(dt, hw):
        if (dt, hw) not in cache:
            s = FineTuneSession(_product(oracle, cuda, dt), 2, hw, lr=0.0)
            s.step(_images(hw).to(cuda), _target().to(cuda))
            cache[dt, hw] = (s.flat.grad.clone(), dict(s.flat.offset))
        return cache[dt, hw]

    return get


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("stage,hw", [(st, HW) for st in STAGES] + [("layer3", (72, 104))],
                         ids=[*STAGES, "layer3-72x104"])
def test_suffix_gradient_is_the_gradient_of_all_bit_for_bit(cuda, oracle, grad_of_all, stage, hw, dt):
    g_all, offset = grad_of_all(dt, hw)
    x, T = _images(hw).to(cuda), _target().to(cuda)
    got = []
    for kw in ({}, {"graph": False}, {"debug": True}):  # batched fold-backward (graph, eager); per conv (debug)
        s = FineTuneSession(_product(oracle, cuda, dt), 2, hw, lr=0.0, trainable=stage, **kw)
        assert s.flat.offset == offset
        s.step(x, T)
        got.append(s)
    o = got[0].opt_begin
    for s in got:
        assert torch.equal(s.flat.grad[o:].view(torch.int32), g_all[o:].view(torch.int32))
        assert int((s.flat.grad[:o] != 0).sum()) == 0  # the prefix slots are zero: nothing was launched for them
    dbg = got[2].debug
    convs = {cv.name for cv in got[2].train_convs}
    for kind in ("wgrad", "dbias", "fold_bwd"):  # debug keys only for what was launched
        assert {k[len(kind) + 1:] for k in dbg if k.startswith(kind + ".")} == convs, kind
    b0 = _first(stage)[:-len(".conv1.weight")]
    assert f"bwd.{b0}.conv2" in dbg and f"bwd.{b0}.conv1" not in dbg and f"bwd.{b0}.downsample" not in dbg
    assert "bwd.maxpool" not in dbg and not [k for k in dbg if k.startswith("stem.")]
    assert sum(k.startswith("bwd.resnet.") for k in dbg) == DGRADS[stage]


# ---- the launch schedule --------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", STAGES)
def test_launch_counts_of_one_eager_step(cuda, oracle, stage):
    s = FineTuneSession(_product(oracle, cuda, "fp32"), 2, HW, lr=LR, trainable=stage, graph=False)
    x, T = _images(HW).to(cuda), _target().to(cuda)
    s.step(x, T)
    with KernelTimer() as timer:
        s.step(x, T)
    got = {n: v["launches"] for n, v in timer.summary().items()}
    print(f"finetune {stage}: timed launches {got}")

    def count(pattern):
        return sum(v for n, v in got.items() if re.search(pattern, n))

    plan, n = s.launch_plan, len(s.train_convs)
    assert count(r"conv_infer_dgrad_kernel") == DGRADS[stage] == plan["dgrad"]
    # nothing of the stem's backward: its data gradient, its weight gradient (the others are in no timed kernel's
    # name either: the debug keys of the test above and the sentinels of the first pin them)
    assert not [k for k in got if re.search(r"stem_dgrad|stem_wgrad|maxpool_bwd|bwd_finalize|fold_bn_bwd_kernel<", k)]
    assert count(r"fold_bn_bwd_kernel_batch") == 1 == plan["fold_bwd"]
    assert count(r"fold_bn_kernel_batch") == 2 and plan["refold"] == s.launches_per_refold == 1  # before and after
    assert count(r"bias_grad_kernel") == plan["bias_grad"] == n - sum(cv.name.endswith("downsample.0")
                                                                      for cv in s.train_convs)
    assert count(r"::wgrad") == n and plan["wgrad"] == 2 * n  # (the plan counts a split reduce per weight gradient)
    assert count(r"conv_infer_kernel") == len(s.convs)
    # every timed launch is one of the kinds above or the stem's forward, and the plan adds up to the session's count
    timed = sum(got.values())
    assert timed == 1 + len(s.convs) + DGRADS[stage] + 1 + 2 + plan["bias_grad"] + n, got
    assert sum(plan.values()) == s.launches_per_step
    assert plan["stem"] == 0 and plan["forward"] == s.launches_per_forward
    all_ = FineTuneSession(_product(oracle, cuda, "fp32"), 2, HW, trainable="all", graph=False)
    assert all_.launches_per_refold == 3 and all_.launch_plan["fold_bwd"] == 1 and all_.launch_plan["dgrad"] == 52
    assert all_.launches_per_step == 443 - 2 * 52 + 1 - 52 + 1  # per-conv: two folds and a fold-backward each


# ---- the step ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", ["layer2", "layer4"])
def test_step_is_clip_and_adam_of_its_own_gradient_over_the_suffix(cuda, oracle, stage):
    x, T = _images(HW).to(cuda), _target().to(cuda)
    s = FineTuneSession(_product(oracle, cuda, "fp32"), 2, HW, lr=LR, max_grad_norm=1.0, trainable=stage)
    before = s.flat.param.clone()
    o = s.opt_begin
    losses = []
    for t in (1, 2):
        p0 = s.flat.param.double().cpu()
        m0, v0 = s.state.exp_avg[o:].double().cpu(), s.state.exp_avg_sq[o:].double().cpu()
        mp = s.state.exp_avg[:o].clone()
        losses.append(s.step(x, T))
        g = s.flat.grad[o:].double().cpu()
        norm = g.norm()
        assert abs(float(s.norm) - float(norm)) <= 1e-6 * float(norm) and float(norm) > 1.0  # clipping is active
        gc = g * min(1.0, 1.0 / (float(norm) + 1e-6))
        m, v = 0.9 * m0 + 0.1 * gc, 0.999 * v0 + 0.001 * gc * gc
        ref = p0[o:] - LR * (m / (1 - 0.9 ** t)) / ((v / (1 - 0.999 ** t)).sqrt() + 1e-8)
        got = s.flat.param.double().cpu()
        assert float((got[o:] - ref).abs().max()) < 2e-6  # tests/test_gpu_kernels.py::test_norm_and_adam's
        assert torch.equal(got[:o], p0[:o])
        assert torch.equal(s.state.exp_avg[:o], mp) and int((s.flat.grad[:o] != 0).sum()) == 0
    assert not torch.equal(s.flat.param[o:], before[o:])
    # graph == eager: the same losses and the same parameters after the two steps
    e = FineTuneSession(_product(oracle, cuda, "fp32"), 2, HW, lr=LR, max_grad_norm=1.0, trainable=stage, graph=False)
    le = [e.step(x, T) for _ in (1, 2)]
    assert torch.equal(torch.stack(le), torch.stack(losses)) and torch.equal(e.flat.param, s.flat.param)


# ---- against the oracle ---------------------------------------------------------------------------------------
def _groups(model):
    bn = {n for n, m in model.named_modules() if isinstance(m, nn.BatchNorm2d)}
    out = {}
    for n, p in model.named_parameters():
        mod, leaf = n.rsplit(".", 1)
        out[n] = "head" if mod in HEAD else "conv" if p.dim() == 4 else "gamma" if leaf == "weight" else "beta"
        assert out[n] in ("head", "conv") or mod in bn
    return out


def _oracle_grads(model, stage, x, target, autocast=False):
    """name -> d(mean loss)/d(parameter) (None on the frozen prefix) of the eval-mode oracle under CPU autograd."""
    from oracle.se3 import geometric_loss

    names = [n for n, _ in model.named_parameters()]
    i0 = names.index(_first(stage))
    for i, p in enumerate(model.parameters()):
        p.requires_grad_(i >= i0)
    model.zero_grad(set_to_none=True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        pred = model(x)
    geometric_loss(pred.to(x.dtype), target.to(x.dtype)).mean().backward()
    return {n: None if p.grad is None else p.grad.detach().double().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("stage", ["layer1", "layer4"])
def test_gradient_matches_the_fp64_oracle_with_a_frozen_prefix(cuda, oracle, stage):
    """Relative L2 distance of the suffix of flat.grad from the oracle's fp64 eval-mode autograd with
    requires_grad_(False) on the prefix, per parameter group over the trained parameters; bar 2 * d_ref (d_ref: the
    CPU reference's bf16-autocast distance from its fp32 gradient over the same parameters; 2 * d_ref < 1 keeps a zero
    or sign-flipped gradient out)."""
    x, T = _images(HW).float() / 255.0, _target()
    m32 = copy.deepcopy(oracle).eval()
    g64 = _oracle_grads(copy.deepcopy(oracle).double().eval(), stage, x.double(), T.double())
    g32 = _oracle_grads(m32, stage, x, T)
    g16 = _oracle_grads(m32, stage, x, T, autocast=True)
    names = list(g64)
    i0 = names.index(_first(stage))
    assert all(g64[n] is None for n in names[:i0]) and all(g64[n] is not None for n in names[i0:])
    groups = _groups(oracle)

    def dist(a, b, ns):
        num = sum(float((a[n] - b[n]).pow(2).sum()) for n in ns)
        return (num / sum(float(b[n].pow(2).sum()) for n in ns)) ** 0.5

    for dt in ("fp32", "bf16"):
        model = _product(oracle, cuda, dt)
        s = FineTuneSession(model, 2, HW, lr=0.0, trainable=stage)
        s.step(x.to(cuda), T.to(cuda))
        got = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters()}
        assert all(int((got[n] != 0).sum()) == 0 for n in names[:i0])  # where the oracle has no gradient: zero
        for grp in ("conv", "gamma", "beta", "head"):
            ns = [n for n in names[i0:] if groups[n] == grp]
            d_ref, e = dist(g16, g32, ns), dist(got, g64, ns)
            print(f"finetune {stage} gradient vs fp64 oracle {dt} {grp}: e = {e:.3e}, d_ref = {d_ref:.3f} "
                  f"(CPU fp32 reference: {dist(g32, g64, ns):.1e})")
            assert ns and 2 * d_ref < 1, (grp, d_ref)
            assert e <= 2 * d_ref, (dt, stage, grp, e, d_ref)


# ---- serving and sharing --------------------------------------------------------------------------------------
def test_a_suffix_session_serves_at_full_depth_and_shares_the_optimizer_state(cuda, oracle):
    from argus_amd.infer import InferenceSession
    from argus_amd.infer_grad import GradientSession

    xa = (_images(HW, 1).float() / 255.0).to(cuda)
    T = _target().to(cuda)
    model = _product(oracle, cuda, "fp32")
    s4 = FineTuneSession(model, 2, HW, lr=LR, trainable="layer4")
    for _ in range(2):
        s4.step(xa, T)
    assert torch.equal(s4(xa), InferenceSession(model, 2, HW)(xa))
    l, g = s4.image_gradient(xa, T)
    fl, fg = GradientSession(model, 2, HW).image_gradient(xa, T)
    assert torch.equal(l, fl) and torch.equal(g, fg) and float(g.abs().max()) > 0
    # a head session on the same model: one optimizer state, one step count; a slot's moments advance only in the
    # steps that train it
    sh = FineTuneSession(model, 2, HW, lr=LR, trainable="head")
    assert sh.state is s4.state and s4.state.step_count == 2
    o4, oh = s4.opt_begin, sh.opt_begin
    assert o4 < oh
    for k in range(2):
        m, v = s4.state.exp_avg.clone(), s4.state.exp_avg_sq.clone()
        p = s4.flat.param.clone()
        sh.step(xa, T)
        assert torch.equal(s4.state.exp_avg[:oh], m[:oh]) and torch.equal(s4.state.exp_avg_sq[:oh], v[:oh])
        assert torch.equal(s4.flat.param[:oh], p[:oh]) and not torch.equal(s4.state.exp_avg[oh:], m[oh:])
        m, p = s4.state.exp_avg.clone(), s4.flat.param.clone()
        s4.step(xa, T)
        assert not torch.equal(s4.state.exp_avg[o4:oh], m[o4:oh]) and torch.equal(s4.state.exp_avg[:o4], m[:o4])
        assert not torch.equal(s4.flat.param[o4:oh], p[o4:oh]) and torch.equal(s4.flat.param[:o4], p[:o4])
        assert s4.state.step_count == 4 + 2 * k
    # and the folded copies of the layer4 session followed its own steps
    assert torch.equal(s4(xa), InferenceSession(model, 2, HW)(xa))


# ---- CLI --------------------------------------------------------------------------------------------------------
def test_train_freeze_bn_trainable_layer4(cuda, tmp_path):
    """train(cfg) with --init-checkpoint --freeze-bn --trainable layer4: one epoch on tests/test_gpu_train.py's dummy
    dataset (10 training samples at batch 4: a partial last batch, so two layer4 sessions on one optimizer state)."""
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
    torch.save(sd0, ckpt)
    save = tmp_path / "ckpt"
    cfg = TrainConfig(batch_size=4, learning_rate=1e-4, n_epochs=1, device="cuda", max_grad_norm=1.0, random_seed=42,
                      val_epochs=1, print_epochs=1, save_epochs=1, save_dir=str(save),
                      model_config=NCameraCNNConfig(n_cams=2),
                      dataset_config=CameraCubePoseDatasetConfig(dataset_path=data, center_crop=(64, 64)),
                      compile_model=False, wandb_log=False, num_workers=0, init_checkpoint=str(ckpt),
                      freeze_bn=True, trainable="layer4")
    train(cfg)
    (pth,) = list(save.glob("*.pth"))
    sd1 = torch.load(pth, weights_only=True)
    assert set(sd1) == set(sd0)
    trained = ("resnet.layer4.", "resnet.fc.", "output_mlp.")
    for k in sd0:
        moved = k.startswith(trained) and "running_" not in k and "num_batches_tracked" not in k
        assert torch.equal(sd1[k], sd0[k]) != moved, k
