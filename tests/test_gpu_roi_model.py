"""GPU: a model conditioned on the region of interest (NCameraCNNConfig.roi_frame_hw) through every layer that
carries the regions: the training engine (forward, backward, the new weight's gradient), FusedTrainer.step against
stock autograd + torch.optim.Adam (step_roi), and PoseSession (fused tail against the unfused head, against model.eval(), the
region buffer read per replay, the tracked loop). resnet_output_dim = 64, 64 x 64 inputs from 96 x 128 frames."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import roi_embed_reference as ref  # noqa: E402
import track_reference as tref  # noqa: E402
from test_gpu_infer import _randomize_bn  # noqa: E402

from argus_amd import track  # noqa: E402
from argus_amd.models import NCameraCNN, NCameraCNNConfig, roi_features  # noqa: E402
from argus_amd.resident import sample_rois  # noqa: E402

pytestmark = pytest.mark.gpu

HW, FHW = ref.HW, ref.FRAME_HW
PLAIN = NCameraCNNConfig(resnet_output_dim=64)
COND = NCameraCNNConfig(resnet_output_dim=64, roi_frame_hw=FHW)
STAGE_BAR = 2e-5  # the fp32 stage bar of tests/test_gpu_model.py (max error over the reference's maximum)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _rois(batch, seed, cuda=None):
    r = sample_rois(np.random.default_rng(seed), batch * 2, FHW, HW, (16, 32), scale=(0.5, 1.5), shift=0.25)
    t = torch.from_numpy(r).view(batch, 2, 4)
    return t if cuda is None else t.to(cuda)


def _conditioned(cuda, dtype, seed=5, weight=True):
    torch.manual_seed(seed)
    m = NCameraCNN(COND, compute_dtype=dtype)
    _randomize_bn(m)
    if weight:
        with torch.no_grad():
            m.roi_embed.weight.copy_(torch.empty(128, 8).uniform_(-1.0, 1.0, generator=torch.Generator().manual_seed(seed)))
    return m.to(cuda)


def _plain_twin(cond, cuda):
    m = NCameraCNN(PLAIN, compute_dtype=cond.compute_dtype)
    m.load_state_dict({k: v for k, v in cond.state_dict().items() if k != "roi_embed.weight"})
    return m.to(cuda).train(cond.training)


# ---- the engine ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_engine_forward_and_backward_carry_the_term(cuda, dtype):
    B = 3
    m = _conditioned(cuda, dtype).train()
    g = torch.Generator().manual_seed(21)
    x = torch.rand(B, 6, *HW, generator=g).to(cuda)
    roi = _rois(B, 22, cuda)
    dpred = torch.randn(B, 6, generator=g).to(cuda)
    pred = m(x, roi)
    (pred * dpred).sum().backward()
    torch.cuda.synchronize()
    eng = m._engine(cuda)
    P = {k: v.detach().double().cpu() for k, v in m.named_parameters()}
    g0, dh1 = eng.g0.double().cpu(), eng.dh1.double().cpu()
    rho = roi_features(roi.double().cpu(), FHW, HW).reshape(B, 8)
    assert (eng.rho.double().cpu() - rho).abs().max().item() <= 4 * 2.0 ** -23  # the kernel test's 4 ulp
    h1 = g0 @ P["output_mlp.0.weight"].T + P["output_mlp.0.bias"] + rho @ P["roi_embed.weight"].T
    errs = {"h1": _rel(eng.h1, h1), "g1": _rel(eng.g1, F.gelu(h1)),
            "roi_embed.weight.grad": _rel(m.roi_embed.weight.grad, dh1.T @ rho),
            "output_mlp.0.weight.grad": _rel(m.output_mlp[0].weight.grad, dh1.T @ g0)}
    print(f"conditioned engine {dtype}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= STAGE_BAR for v in errs.values()), errs
    assert (rho @ P["roi_embed.weight"].T).abs().max() > 0.05  # the term is visible at this bar
    assert roi.grad is None and not roi.requires_grad


def test_zero_weight_is_the_unconditioned_function(cuda):
    B = 3
    m = _conditioned(cuda, "fp32", weight=False).eval()
    plain = _plain_twin(m, cuda)
    x = torch.rand(B, 6, *HW, generator=torch.Generator().manual_seed(31)).to(cuda)
    ra, rb = _rois(B, 32, cuda), _rois(B, 33, cuda)
    with torch.no_grad():
        want = plain(x)
        ya, yb = m(x, ra), m(x, rb)
        err = _rel(ya, want)
        print(f"zero roi_embed.weight vs the plain model: {err:.2e}")
        assert err <= STAGE_BAR  # epilogue 1 + a separate GELU need not be epilogue 2's bits
        assert torch.equal(ya, yb)  # 0 * rho: the regions cannot matter
        m.roi_embed.weight.copy_(torch.empty(128, 8).uniform_(-1.0, 1.0, generator=torch.Generator().manual_seed(1)))
        za, zb = m(x, ra), m(x, rb)
        assert not torch.equal(za, zb) and not torch.equal(za, ya)
    with pytest.raises(ValueError, match="pass roi"):
        m(x)
    with pytest.raises(ValueError, match="without roi_frame_hw"):
        plain(x, ra)
    with pytest.raises(ValueError, match="is on"):
        m(x, ra.cpu())


# ---- the trainer --------------------------------------------------------------------------------------------------
def test_fused_step_matches_autograd_and_adam(cuda):
    from argus_amd.losses import geometric_loss_fn
    from argus_amd.step import FusedTrainer

    B = 3
    g = torch.Generator().manual_seed(41)
    xs = [torch.rand(B, 6, *HW, generator=g).to(cuda) for _ in range(3)]
    rois = [_rois(B, 42 + i, cuda) for i in range(3)]
    q = F.normalize(torch.randn(B, 4, generator=g), dim=-1)
    T = torch.cat([0.1 * torch.randn(B, 3, generator=g), q], -1).to(cuda)
    fused, stock = [_conditioned(cuda, "fp32", seed=9, weight=False).train() for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(fused.state_dict().values(), stock.state_dict().values()))
    tr = FusedTrainer(fused, lr=1e-4, max_grad_norm=1.0)
    opt = torch.optim.Adam(stock.parameters(), lr=1e-4)
    for i in range(2):
        losses = tr.step_roi(xs[i], T, rois[i]).clone()
        opt.zero_grad()
        per = geometric_loss_fn(stock(xs[i], rois[i]), T)
        per.mean().backward()
        torch.nn.utils.clip_grad_norm_(stock.parameters(), 1.0)
        opt.step()
        print(f"step {i}: fused losses {losses.tolist()} stock {per.reshape(-1).tolist()}")
        assert torch.allclose(losses.cpu(), per.detach().reshape(-1).cpu(), atol=1e-4)
        if i == 0:  # the new parameter trains: it has left zero, in both
            assert int(fused.roi_embed.weight.count_nonzero()) > 0 and int(stock.roi_embed.weight.count_nonzero()) > 0
    with torch.no_grad():
        a, b = fused(xs[2], rois[2]).cpu(), stock(xs[2], rois[2]).cpu()
    print(f"predictions after two steps differ by {(a - b).abs().max().item():.2e}")
    assert torch.allclose(a, b, atol=2e-3)
    with pytest.raises(ValueError, match="pass roi"):
        tr.step(xs[0], T)


# ---- the session --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deployed(cuda):
    return _conditioned(cuda, "bf16", seed=13).eval()


def _frames(batch, seed, cuda):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (batch, 6, *FHW), generator=g, dtype=torch.uint8).to(cuda)


def test_session_fused_tail_against_the_unfused_head_and_the_model(cuda, deployed):
    from argus_amd.pose_session import PoseSession

    B = 2
    frames = _frames(B, 51, cuda)
    ra, rb = _rois(B, 52), _rois(B, 53)
    kw = dict(frame_hw=FHW, roi=True)
    s = PoseSession(deployed, B, HW, **kw)
    un = PoseSession(deployed, B, HW, fused_head=False, **kw)
    assert s.launches_per_forward == 55 and un.launches_per_forward == 60  # 59 + argus_roi_embed
    ya, yu = s(frames, roi=ra), un(frames, roi=ra)
    scale = float(ya.abs().max())
    print(f"fused tail vs unfused head: {(ya - yu).abs().max().item():.2e} (bar {1e-4 * scale:.2e})")
    assert torch.allclose(yu, ya, rtol=0, atol=1e-4 * scale)  # test_gpu_pose_session.py's bar for this pair
    # a new region: another pose from the same graph
    graph = s._graphs["forward", torch.uint8]
    pa = s.pose(frames, roi=ra)
    pb = s.pose(frames, roi=rb)
    assert not torch.equal(pa, pb) and torch.equal(s.pose(frames, roi=ra), pa)
    assert len(s._graphs) == 1 and s._graphs["forward", torch.uint8] is graph
    eager = PoseSession(deployed, B, HW, graph=False, **kw)
    assert torch.equal(eager.pose(frames, roi=ra), pa)

    # against model.eval() on the resampled frames. Both are bf16 networks with different roundings (folded BN,
    # other kernels), so the yardstick is the same pair for the unconditioned twin on the same pixels; a session
    # may be twice as far from the truth as model.eval() (test_gpu_pose_session.py), and the head's own two
    # implementations add that file's 1e-4 of the largest prediction.
    pre = PoseSession(deployed, B, HW, fused_stem=False, graph=False, **kw)
    pre(frames, roi=ra)
    x = pre.x0[..., :3].float().permute(0, 3, 1, 2).reshape(B, 6, *HW).contiguous()  # what the stem resampled
    plain = _plain_twin(deployed, cuda)
    with torch.no_grad():
        y_model = deployed(x, ra.to(cuda))
        d_plain = (PoseSession(plain, B, HW)(x) - plain(x)).abs().max().item()
    d = (ya - y_model).abs().max().item()
    print(f"session vs model.eval(): {d:.3e}; the unconditioned pair: {d_plain:.3e}; max |pred| {scale:.2f}")
    assert d <= 2 * d_plain + 1e-4 * scale
    with torch.no_grad():  # and that bar would see a wrong region: another one moves the model further than it
        assert (deployed(x, rb.to(cuda)) - y_model).abs().max().item() > 2 * d_plain + 1e-4 * scale


def test_tracked_session_reads_the_region_the_stem_used(cuda, deployed):
    from argus_amd.pose_session import PoseSession

    B = 1
    frames = _frames(B, 61, cuda)
    home = [10.0, 20.0, 70.0, 70.0]  # not the centre crop
    kw = dict(frame_hw=FHW)
    open_loop = PoseSession(deployed, B, HW, roi=True, **kw)
    first = open_loop.pose(frames, roi=torch.tensor(home))
    c = first[:, :3].double().mean(0).cpu().numpy()
    off = 0.2 * np.array([0.0, 0.15, 0.13]) / np.hypot(0.15, 0.13)
    words = np.float64([tref.look_at_camera(c + off * [1, s, 1], c, 70.0, FHW) for s in (1.0, -1.0)])
    cams = [track.Camera(w[:9], w[9:12], *w[12:]) for w in words]
    cfg = track.TrackConfig(cams, tref.HALF_EXTENT, margin=tref.MARGIN, z_near=tref.Z_NEAR, smooth=0.5, home=home)
    tracked = PoseSession(deployed, B, HW, track=cfg, **kw)
    assert open_loop.launches_per_forward == 55 and tracked.launches_per_forward == 56
    moved = 0
    for k in range(3):
        before = tracked.roi
        pose = tracked.pose(frames)
        used = tracked.last_roi
        assert torch.equal(used, before)
        moved += int(not torch.equal(tracked.roi, used))
        # the tail read the region the stem used, not the one argus_roi_from_pose wrote behind it
        assert torch.equal(pose, open_loop.pose(frames, roi=used)), k
    assert moved >= 2  # the tracker did move: the two regions were different ones


# ---- train.py / validate.py ---------------------------------------------------------------------------------------
def test_train_and_validate_with_roi_features_end_to_end(cuda, tmp_path, tmp_path_factory, monkeypatch):
    from conftest import make_dummy_dataset

    from argus_amd import _lib
    from argus_amd.data import CameraCubePoseDatasetConfig
    from argus_amd.train import TrainConfig, train
    from argus_amd.validate import ValConfig, validate

    path = make_dummy_dataset(tmp_path_factory.mktemp("roi_features"), hw=FHW)
    calls = []
    L = _lib.lib()
    fn = L.roi_embed
    monkeypatch.setattr(L, "roi_embed", lambda *a: (calls.append(a[:6]), fn(*a))[1])
    save = tmp_path / "m"
    data = CameraCubePoseDatasetConfig(dataset_path=path, center_crop=HW)
    train(TrainConfig(batch_size=5, learning_rate=1e-3, n_epochs=1, device="cuda", max_grad_norm=100.0, random_seed=42,
                      val_epochs=1, print_epochs=1, save_epochs=1, save_dir=str(save), model_config=PLAIN,
                      dataset_config=data, compile_model=False, wandb_log=False, num_workers=0, resident_dataset=True,
                      roi_jitter=(0.7, 1.4, 0.1), roi_features=True))
    # two train steps of five and one validation batch of five, all told about 96 x 128 frames and 64 x 64 inputs
    assert calls == [(5, 2, *FHW, *HW)] * 3
    (pth,) = list(save.glob("*.pth"))
    sd = torch.load(pth, weights_only=True)
    assert tuple(sd["roi_embed.weight"].shape) == (128, 8) and int(sd["roi_embed.weight"].count_nonzero()) > 0
    assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
    losses = validate(ValConfig(str(pth), data, model_config=COND, batch_size=5))
    assert len(losses) == 5 and all(np.isfinite(losses)) and len(calls) == 4
    with pytest.raises(RuntimeError, match="roi_embed.weight"):  # the checkpoint is a conditioned one
        validate(ValConfig(str(pth), data, model_config=PLAIN, batch_size=5))
