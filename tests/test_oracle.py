"""CPU: the oracle is pinned by the golden fixtures (reference models.py run with the oracle ResNet
injected; closed-form loss KATs; the reference tests' literal vectors)."""
import math

import torch

from oracle import se3
from oracle.ncamera import build_reference_model


def test_loss_kats(golden):
    for kat in golden["loss_kats"]:
        p = torch.tensor([kat["pred"]], dtype=torch.float64)
        t = torch.tensor([kat["target"]], dtype=torch.float64)
        assert abs(se3.geometric_loss(p, t).item() - kat["loss"]) < 1e-12


def test_loss_identity_and_shapes():
    # tests/test_train.py:18-36: unbatched -> scalar, batched -> (B,), loss(p, Exp(p)) == 0
    assert se3.geometric_loss(torch.randn(6), se3.se3_exp(torch.randn(6))).shape == torch.Size([])
    p = torch.randn(32, 6, dtype=torch.float64)
    assert se3.geometric_loss(p, se3.random_targets(32).double()).shape == (32,)
    assert se3.geometric_loss(p, se3.se3_exp(p)).abs().max().item() < 1e-12


def test_loss_gradient_matches_finite_differences():
    g = torch.Generator().manual_seed(0)
    p = torch.randn(8, 6, generator=g, dtype=torch.float64) * 0.8
    T = se3.random_targets(8, generator=g).double()
    _, grad = se3.loss_and_grad(p, T, mean=False)
    eps = 1e-6
    for i in range(6):
        e = torch.zeros_like(p)
        e[:, i] = eps
        fd = (se3.geometric_loss(p + e, T) - se3.geometric_loss(p - e, T)) / (2 * eps)
        assert (fd - grad[:, i]).abs().max().item() < 1e-7


def test_near_pi_sign_invariance():
    # rotation by 1.5 pi == rotation by -0.5 pi: the shortest-angle Log gives pi^2/4
    p = torch.tensor([[0, 0, 0, 0, 0, 1.5 * math.pi]], dtype=torch.float64)
    assert abs(se3.geometric_loss(p, torch.tensor([[0, 0, 0, 0, 0, 0, 1.0]], dtype=torch.float64)).item()
               - math.pi**2 / 4) < 1e-12


def test_state_dict_schema_and_forward_match_golden(golden):
    m = build_reference_model(42)
    sd = m.state_dict()
    assert [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()] == golden["state_dict"]
    assert sum(v.numel() for k, v in sd.items()
               if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))) == golden["n_params"] == 25885766
    import tests.golden.make_golden as mg

    x = mg.synthetic_images(2, 256, 256, seed=1234)
    assert mg.state_sha256(sd) == golden["state_sha256"]
    m.train()
    with torch.no_grad():
        pt = m(x)
        m.eval()
        pe = m(x)
    assert torch.allclose(pt, torch.tensor(golden["pred_train"]), atol=1e-6)
    assert torch.allclose(pe, torch.tensor(golden["pred_eval"]), atol=1e-6)


def test_pose_order_kats(golden):
    from argus_amd.utils import xyzwxyz_to_xyzxyzw_SE3, xyzxyzw_to_xyzwxyz_SE3

    a = torch.tensor(golden["pose_order_kats"]["xyzwxyz"])
    b = torch.tensor(golden["pose_order_kats"]["xyzxyzw"])
    assert torch.allclose(xyzwxyz_to_xyzxyzw_SE3(a), b)
    assert torch.allclose(xyzxyzw_to_xyzwxyz_SE3(b), a)
    assert torch.allclose(xyzwxyz_to_xyzxyzw_SE3(a[0]), b[0])
    r = torch.randn(2, 7)
    assert torch.allclose(xyzxyzw_to_xyzwxyz_SE3(xyzwxyz_to_xyzxyzw_SE3(r)), r)


def test_damped_golden_pins_oracle():
    """golden_b8_damped.json (reference models.py at damp_residual(0.1), B=8 at 128x128): the oracle
    reproduces the reference's fp32 and fp64 predictions and its fp32-vs-fp64 gradient error."""
    import json

    import tests.golden.make_golden as mg

    with open(mg.OUT / "golden_b8_damped.json") as f:
        g = json.load(f)
    c = g["config"]
    x = mg.synthetic_images(c["batch"], *c["hw"], seed=c["image_seed"])
    T = mg.synthetic_targets(c["batch"], seed=c["target_seed"])
    assert torch.allclose(T, torch.tensor(g["targets"]))
    grads = {}
    for dt in (torch.float32, torch.float64):
        m = mg.damp_residual(build_reference_model(42), c["damp"]).to(dt).train()
        pred = m(x.to(dt))
        want = torch.tensor(g["pred_train_fp32" if dt == torch.float32 else "pred_train_fp64"], dtype=dt)
        assert (pred.detach() - want).abs().max().item() < (1e-6 if dt == torch.float32 else 1e-12)
        se3.geometric_loss(pred, T.to(dt)).mean().backward()
        grads[dt] = mg.flat_grads(m)
    e, _ = mg.grad_errors(grads[torch.float32], grads[torch.float64])
    assert abs(e - g["ref_fp32_vs_fp64"]["global"]) < 0.2 * g["ref_fp32_vs_fp64"]["global"]
    assert e < 2e-3  # the point is well conditioned (vs 2.2e-2 at seeded init)


def _load(name):
    import json

    import tests.golden.make_golden as mg

    with open(mg.OUT / name) as f:
        return json.load(f)


def test_two_rank_golden_pins_oracle():
    """golden_b8_damped_2rank.json (the reference's DDP step, two ranks of 4 samples at the damped point):
    the oracle reproduces each rank's per-sample losses (per-shard train-mode BN)."""
    import tests.golden.make_golden as mg

    g = _load("golden_b8_damped_2rank.json")
    c = g["config"]
    x = mg.synthetic_images(c["batch"], *c["hw"], seed=c["image_seed"])
    T = mg.synthetic_targets(c["batch"], seed=c["target_seed"])
    assert abs(float(x.double().sum()) - g["images_sum"]) < 1e-3
    m = mg.damp_residual(build_reference_model(42), c["damp"]).train()
    with torch.no_grad():
        for r, (xs, ts) in enumerate(mg.shards(x, T, g["ddp"]["world"])):
            l = se3.geometric_loss(m(xs), ts)
            assert (l - torch.tensor(g["step"]["loss"][r])).abs().max().item() < 1e-5, r
    assert g["ref_fp32_vs_fp64"]["global"] < 2e-3  # well conditioned, as the single-rank point


def test_trajectory_golden_pins_oracle():
    """golden_b8_damped_traj.json: the oracle reproduces the first step's losses, the schedule really
    reduces the learning rate inside the 10 steps, and fp32 stays close to fp64 over the trajectory."""
    import tests.golden.make_golden as mg

    g = _load("golden_b8_damped_traj.json")
    c = g["config"]
    assert c == mg.TRAJ
    (x, T), = mg.trajectory_batches(c)[0][:1]
    m = mg.damp_residual(build_reference_model(42), c["damp"]).train()
    with torch.no_grad():
        l = se3.geometric_loss(m(x), T)
    assert (l - torch.tensor(g["fp32"]["steps"][0]["loss"])).abs().max().item() < 1e-5
    lrs = [s["lr"] for s in g["fp32"]["steps"]]
    assert lrs == [s["lr"] for s in g["fp64"]["steps"]] and min(lrs) < c["lr"]
    for s32, s64 in zip(g["fp32"]["steps"], g["fp64"]["steps"]):
        assert max(abs(a - b) for a, b in zip(s32["loss"], s64["loss"])) < 1e-2


def _regime_properties(name, pred, T, angle):
    """Every sample sits where its regime says; the residual angle is the definition's own."""
    th = pred[:, 3:].double().norm(dim=-1)
    assert (math.pi - angle).min().item() > 5e-4, name  # the principal logarithm jumps at pi
    if name == "generic":
        assert (pred[:, :3].abs().amax(-1) > 0).all() and (th > 1e-2).all() and (angle > 1e-2).all()
        assert (T[:, :3].abs().amax(-1) > 0).all() and (T[:, 3:6].abs().amax(-1) > 0).all()
    elif name == "pred_small_angle":
        assert th.min() == 0 and ((th > 0.9e-4) & (th < 1e-4)).any() and ((th > 1e-4) & (th < 1.1e-4)).any()
    elif name == "residual_small":
        n = torch.sin(angle / 2)
        assert angle.min() < 1e-7 and ((n > 0.98e-4) & (n < 1e-4)).any() and ((n > 1e-4) & (n < 1.02e-4)).any()
    elif name == "residual_near_pi":
        d = math.pi - angle
        assert ((d - 1e-3).abs() < 1e-5).sum() == 4 and ((d - 1e-2).abs() < 1e-5).sum() == 4
        assert (T[:, :3].abs().amax(-1) > 0).all()
    elif name == "pred_beyond_pi":
        assert (th > math.pi).all() and (th > 2 * math.pi).any()
        assert (angle[-4:] < 1.9e-4).all() and (angle[-4:] > 1e-5).all()  # n < 1e-4 with w < 0
    elif name == "large_translation":
        assert (pred[:, :3].double().norm(dim=-1) > 30).all() and (T[:, :3].double().norm(dim=-1) > 30).all()
    elif name == "target_quat_scaled":
        s = T[:, 3:].double().norm(dim=-1)
        n = s * torch.sin(angle / 2)
        assert ((s - 1).abs() > 0.4).sum() >= 10 and (T[:, 6] < 0).any()
        assert ((n < 1e-4) & ((s - 1).abs() > 0.4)).sum() >= 4 and (n > 1e-4).any()


def test_loss_and_grad_match_the_definition_in_every_regime():
    """oracle/se3.py's closed forms (Rodrigues, J_l, atan, their Taylor branches and thresholds) against
    the matrix exponential and the principal matrix logarithm at 40 digits, gradient by central
    differences at that precision (tests/se3_cases.py). Bars: se3_cases.BARS, 4x the measured discrepancy."""
    from tests import se3_cases

    assert list(se3_cases.BARS) == list(se3_cases.regimes())
    for name, (pred, T) in se3_cases.regimes().items():
        d_loss, d_grad, angle = se3_cases.definition_results(name)
        _regime_properties(name, pred, T, angle)
        o_loss, o_grad = se3.loss_and_grad(pred, T, mean=False)
        bar = se3_cases.BARS[name]
        e_loss = (o_loss - d_loss).abs()
        e_grad = (o_grad - d_grad).abs().amax(-1)
        g_inf = d_grad.abs().amax(-1)
        print(name, "loss: rel", (e_loss / d_loss.abs())[d_loss.abs() >= se3_cases.SMALL].tolist(),
              "abs", e_loss[d_loss.abs() < se3_cases.SMALL].tolist())
        print(name, "grad: rel", (e_grad / g_inf)[g_inf >= se3_cases.SMALL].tolist(),
              "abs", e_grad[g_inf < se3_cases.SMALL].tolist())
        assert (e_loss <= bar["r_loss"] * d_loss.abs() + bar["a_loss"]).all(), name
        assert (e_grad <= bar["r_grad"] * g_inf + bar["a_grad"]).all(), name


def test_se3_exp_matches_the_matrix_exponential():
    from tests import se3_cases

    for name in se3_cases.EXP_REGIMES:
        xi = se3_cases.regimes()[name][0]
        want = se3_cases.definition_exp(xi)
        got = se3.se3_exp(xi.double())
        bar = se3_cases.EXP_BARS[name]
        e_t = (got[:, :3] - want[:, :3]).abs().amax(-1)
        e_q = (got[:, 3:] - want[:, 3:]).abs().amax(-1)
        print(name, "t", (e_t / want[:, :3].abs().amax(-1).clamp_min(1.0)).max().item(), "q", e_q.max().item())
        assert (e_t <= bar["r_t"] * want[:, :3].abs().amax(-1).clamp_min(1.0)).all(), name
        assert (e_q <= bar["a_q"]).all(), name
