"""GPU: argus_amd.pose_session.PoseSession (frames in, SE(3) pose out, one replayed graph of 55 launches).

The prediction is held to the fp64 oracle with test_gpu_infer.py's recipe and the existing bars: bf16 within 2x the
distance of the compute_dtype="bf16" model.eval() forward, fp16 within 2x the reference's own fp16 autocast
distance and at most half the bf16 session's. The pose is held to se3_exp of the oracle's fp64 prediction with the
bar those prediction bars propagate to through the exponential's Lipschitz constants (see _pose_bar). With both
ends unfused the session must reproduce InferenceSession bit for bit, which pins the shared 52 convs and places a
failure of the fused session at one end."""
import math

import pytest
import torch

from oracle import se3
from test_gpu_infer import _Count, _images, _product, oracle, oracle_fp64  # noqa: F401

pytestmark = pytest.mark.gpu


def _pose_bar(ref_pred, delta):
    """Per-sample bounds (translation, quaternion) on |pose - se3_exp(ref_pred)|_inf for a prediction within
    ``delta`` (max norm) of ``ref_pred``, from the reference alone. With |d rho|_2, |d phi|_2 <= sqrt(3) delta:
    q = exp(phi / 2) on the unit sphere, whose differential has norm <= 1, so |dq|_2 <= sqrt(3) / 2 delta;
    t = J_l(phi) rho with J_l(phi) = int_0^1 exp(s phi^) ds, so |J_l| <= 1 and |dJ_l| <= |d phi| / 2, hence
    |dt|_2 <= sqrt(3) delta (1 + (|rho|_2 + sqrt(3) delta) / 2) along the segment between the two predictions.
    Added: the fp32 output rounding of test_se3_exp_kernel's bar, 2^-22 max(1, |t|_inf)."""
    r3 = math.sqrt(3.0) * delta
    rho = ref_pred[:, :3].norm(dim=-1)
    t_ref = se3.se3_exp(ref_pred)[:, :3].abs().amax(-1)
    rounding = 2.0 ** -22 * (t_ref + r3 * (1 + rho)).clamp_min(1.0)
    return r3 * (1 + 0.5 * (rho + r3)) + rounding, 0.5 * r3 + rounding


@pytest.mark.parametrize("hw", [(64, 64), (72, 104)], ids=["64x64", "72x104"])
def test_pose_session_matches_the_fp64_oracle(cuda, oracle, oracle_fp64, hw):
    from argus_amd.infer import InferenceSession
    from argus_amd.pose_session import PoseSession

    u8 = _images(hw)
    xc = u8.float() / 255.0
    x = xc.to(cuda)
    ref = oracle_fp64[hw]
    ref_pose = se3.se3_exp(ref)
    m16 = _product(oracle, cuda, "bf16")
    with torch.no_grad():
        d_eval = (m16(x).double().cpu() - ref).abs().max().item()  # the existing bf16 eval path
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.float16):
        d_ref = (oracle(xc).double() - ref).abs().max().item()  # the reference's own fp16 mode, on the CPU
    d_parent = (InferenceSession(m16, 2, hw)(x).double().cpu() - ref).abs().max().item()
    bars = {"bf16": 2 * d_eval, "fp16": min(2 * d_ref, 0.5 * d_parent)}
    for dt, model in (("bf16", m16), ("fp16", _product(oracle, cuda, "fp32"))):
        s = PoseSession(model, 2, hw, compute_dtype=dt)
        pose = s.pose(u8.to(cuda)).double().cpu()
        pred = s(u8.to(cuda)).double().cpu()
        d = (pred - ref).abs().max().item()
        bt, bq = _pose_bar(ref, bars[dt])
        et, eq = (pose[:, :3] - ref_pose[:, :3]).abs().amax(-1), (pose[:, 3:] - ref_pose[:, 3:]).abs().amax(-1)
        print(f"pose session vs fp64 oracle {hw} {dt}: pred {d:.3e} (bar {bars[dt]:.3e}; bf16 model.eval() {d_eval:.3e}, "
              f"reference fp16 autocast {d_ref:.3e}, bf16 InferenceSession {d_parent:.3e}); pose t {et.tolist()} (bar "
              f"{bt.tolist()}), q {eq.tolist()} (bar {bq.tolist()}); max |pred| {ref.abs().max().item():.2f}")
        assert d <= bars[dt]
        assert bool((et <= bt).all()) and bool((eq <= bq).all())


def test_crop_and_layout_give_the_precropped_planar_bits(cuda, oracle):
    from argus_amd.data import center_crop_slices
    from argus_amd.pose_session import PoseSession

    hw, fhw = (72, 104), (80, 120)
    model = _product(oracle, cuda, "bf16")
    g = torch.Generator().manual_seed(5)
    hwc = torch.randint(0, 256, (2, 2, *fhw, 3), generator=g, dtype=torch.uint8)
    ys, xs = center_crop_slices(fhw, hw)
    planar = hwc[:, :, ys, xs, :].permute(0, 1, 4, 2, 3).reshape(2, 6, *hw).contiguous()
    a = PoseSession(model, 2, hw, frame_hw=fhw, layout="hwc")
    b = PoseSession(model, 2, hw)
    c = PoseSession(model, 2, hw, frame_hw=fhw)  # planar frames, cropped by the stem
    pa, pb = a.pose(hwc.to(cuda)), b.pose(planar.to(cuda))
    pc = c.pose(hwc.permute(0, 1, 4, 2, 3).reshape(2, 6, *fhw).contiguous().to(cuda))
    assert torch.equal(pa, pb) and torch.equal(pc, pb) and torch.equal(a.pred, b.pred)
    assert a.launches_per_forward == b.launches_per_forward == 55
    with pytest.raises(ValueError, match="shape"):
        a.pose(planar.to(cuda))


def test_pose_session_semantics(cuda, oracle):
    from argus_amd.infer import InferenceSession
    from argus_amd.pose_session import PoseSession
    from argus_amd.utils import get_pose, se3_exp

    hw = (64, 64)
    model = _product(oracle, cuda, "bf16")
    u8a, u8b = _images(hw, 1), _images(hw, 2)
    xa = (u8a.float() / 255.0).to(cuda)  # the division on the CPU, as the data pipeline does it
    u8a, u8b = u8a.to(cuda), u8b.to(cuda)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    sg, se = PoseSession(model, 2, hw, graph=True), PoseSession(model, 2, hw, graph=False)
    pa = sg.pose(u8a)
    ya = sg(u8a)
    assert pa.shape == (2, 7) and ya.shape == (2, 6) and pa.dtype == ya.dtype == torch.float32
    assert torch.equal(pa, se3_exp(ya))  # the pose of the replay is argus_se3_exp of its prediction
    assert torch.equal(pa, se.pose(u8a)) and torch.equal(ya, se(u8a))  # replayed graph == eager launches
    assert torch.equal(sg.pose(xa), pa) and torch.equal(sg(xa), ya)  # uint8 == its /255 float batch
    assert not torch.equal(sg.pose(u8b), pa)
    assert torch.equal(sg.pose(u8a), pa) and torch.equal(se.pose(u8a), pa)  # no stale state, no ticket residue
    assert pa.data_ptr() != sg.pose(u8a).data_ptr() and ya.data_ptr() != sg(u8a).data_ptr()  # fresh tensors
    assert torch.equal(get_pose(u8a, sg), pa)
    # pose(None) replays on what the caller wrote into the static buffer
    sg.pose(u8b)
    sg.frames[torch.uint8].copy_(u8a)
    assert torch.equal(sg.pose(None), pa)
    sg.frames[torch.float32].copy_(xa)
    assert torch.equal(sg.pose(None, torch.float32), pa)
    # launches: counted as test_gpu_infer.py::test_session_semantics counts them
    se.L = cnt = _Count(se.L)
    se.pose(u8a)
    se.L = cnt._L
    assert cnt.n == se.launches_per_forward == sg.launches_per_forward == 55
    assert not hasattr(sg, "x0") and not hasattr(sg, "amax")  # no NHWC4 copy, no argmax (and no stem output)
    # the session never writes the model; a snapshot until refresh()
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    bias = model.output_mlp[4].bias.data.clone()
    model.output_mlp[4].bias.data += 1
    assert torch.equal(sg(u8a), ya) and torch.equal(se(u8a), ya)
    sg.refresh()
    se.refresh()
    assert torch.equal(sg(u8a), se(u8a))
    assert torch.allclose(sg(u8a), ya + 1, rtol=0, atol=2e-6 * float(ya.abs().max() + 1))  # moved by that bias
    assert torch.equal(sg.pose(u8a), se3_exp(sg(u8a)))
    model.output_mlp[4].bias.data.copy_(bias)
    sg.refresh()
    assert torch.equal(sg(u8a), ya)
    # both ends unfused: InferenceSession's launches, InferenceSession's bits
    parent = InferenceSession(model, 2, hw)
    for graph in (True, False):
        un = PoseSession(model, 2, hw, graph=graph, fused_stem=False, fused_head=False)
        assert un.launches_per_forward == parent.launches_per_forward == 61
        assert torch.equal(un(u8a), parent(u8a)) and torch.equal(un.pose(u8a), parent.pose(u8a))
    # one end at a time: same network, another rounding at that end only. Each of the four head layers is within
    # 1e-5 of fp64 in either implementation (the kernel bar), so two implementations differ by at most 2e-5 a layer
    for kw, launches in ((dict(fused_stem=False), 57), (dict(fused_head=False), 59)):
        half = PoseSession(model, 2, hw, **kw)
        assert half.launches_per_forward == launches
        if "fused_stem" in kw:  # the head alone differs: fp32 sums in another order
            assert torch.allclose(half(u8a), parent(u8a), rtol=0, atol=1e-4 * float(ya.abs().max()))
        else:  # the convs see the fused stem's output: the fused session's prediction up to the head's sums
            assert torch.allclose(half(u8a), ya, rtol=0, atol=1e-4 * float(ya.abs().max()))
    # the fp16 diagnostic probes the pooled stem output in place of the stem output
    s16 = PoseSession(_product(oracle, cuda, "fp32"), 2, hw, compute_dtype="fp16")
    y16 = s16(u8a)
    peak = s16.activation_peak(u8a)
    assert 0 < peak < 65504.0 and torch.equal(s16(u8a), y16)  # the diagnostic disturbs nothing
    assert peak >= float(s16.pool[0][:4 * 16 * 16 * 64].abs().max())


def test_pose_session_refuses_what_it_does_not_serve(cuda, oracle):
    from argus_amd.pose_session import PoseSession

    m32 = _product(oracle, cuda, "fp32")
    with pytest.raises(ValueError, match="InferenceSession"):
        PoseSession(m32, 2, (64, 64))  # the model's dtype is fp32: not a default
    with pytest.raises(ValueError, match="InferenceSession"):
        PoseSession(m32, 2, (64, 64), compute_dtype="fp32")
    with pytest.raises(ValueError, match="InferenceSession"):
        PoseSession(m32, 9, (64, 64), compute_dtype="bf16")  # 18 rows
    with pytest.raises(ValueError, match="fused_stem"):
        PoseSession(m32, 2, (64, 64), compute_dtype="bf16", layout="hwc", fused_stem=False)
    with pytest.raises(ValueError, match="fused_stem"):
        PoseSession(m32, 2, (64, 64), compute_dtype="bf16", frame_hw=(80, 80), fused_stem=False)
    with pytest.raises(ValueError, match="layout"):
        PoseSession(m32, 2, (64, 64), compute_dtype="bf16", layout="nhwc")
    s = PoseSession(m32, 2, (64, 64), compute_dtype="bf16")
    with pytest.raises(ValueError, match="float32 or uint8"):
        s.pose(torch.zeros(2, 6, 64, 64, dtype=torch.float64, device=cuda))
