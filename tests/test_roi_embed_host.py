"""CPU: conditioning the pose head on the region of interest (NCameraCNNConfig.roi_frame_hw). What needs no GPU:
the parameter layout (the new weight is last, every other flat offset stays), zero initialisation that leaves the
generator alone, state-dict compatibility, the ValueErrors in front of any device work, --roi-features' validation,
the two new entry points' refusals, and the reference (tests/roi_embed_reference.py) against itself in float32."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import roi_embed_reference as ref  # noqa: E402

from argus_amd.models import NCameraCNN, NCameraCNNConfig, crop_roi, roi_features  # noqa: E402

PLAIN = NCameraCNNConfig(resnet_output_dim=64)
COND = NCameraCNNConfig(resnet_output_dim=64, roi_frame_hw=ref.FRAME_HW)


@pytest.fixture(scope="module")
def pair():
    """(plain, conditioned, one draw of the generator after each construction), both seeded alike."""
    out = []
    for cfg in (PLAIN, COND):
        torch.manual_seed(7)
        out.append(NCameraCNN(cfg))
        out.append(torch.rand(4))
    return out[0], out[2], out[1], out[3]


# ---- the model ----------------------------------------------------------------------------------------------
def test_default_config_is_todays_model(pair):
    plain = pair[0]
    torch.manual_seed(7)
    default = NCameraCNN(NCameraCNNConfig(resnet_output_dim=64))
    assert NCameraCNNConfig().roi_frame_hw is None and plain.roi_frame_hw is None
    names = [n for n, _ in plain.named_parameters()]
    assert names[-6:] == ["output_mlp.0.weight", "output_mlp.0.bias", "output_mlp.2.weight", "output_mlp.2.bias",
                          "output_mlp.4.weight", "output_mlp.4.bias"]
    assert names[-8:-6] == ["resnet.fc.weight", "resnet.fc.bias"] and names[0] == "resnet.conv1.weight"
    assert not any("roi" in n for n in plain.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), default.state_dict().values()))


def test_conditioned_model_adds_one_zero_parameter_last(pair):
    plain, cond, after_plain, after_cond = pair
    pn, cn = [n for n, _ in plain.named_parameters()], [n for n, _ in cond.named_parameters()]
    assert cn == pn + ["roi_embed.weight"]
    assert list(cond.state_dict()) == list(plain.state_dict()) + ["roi_embed.weight"]
    w = cond.roi_embed.weight
    assert tuple(w.shape) == (128, 8) and w.dtype == torch.float32 and int(w.count_nonzero()) == 0
    assert cond.roi_embed.bias is None and cond.roi_frame_hw == ref.FRAME_HW
    # seeded initialisation: the same values everywhere else, and the generator where the plain model leaves it
    ps, cs = plain.state_dict(), cond.state_dict()
    assert all(torch.equal(ps[k], cs[k]) for k in ps)
    assert torch.equal(after_plain, after_cond)
    with pytest.raises(ValueError, match="n_cams"):
        NCameraCNN(NCameraCNNConfig(n_cams=17, resnet_output_dim=64, roi_frame_hw=ref.FRAME_HW))
    with pytest.raises(ValueError, match="roi_frame_hw"):
        NCameraCNN(NCameraCNNConfig(resnet_output_dim=64, roi_frame_hw=(96,)))


def test_flat_offsets_of_every_other_parameter_are_kept():
    from argus_amd.step import FlatParams

    flats = []
    for cfg in (PLAIN, COND):
        torch.manual_seed(7)
        flats.append(FlatParams(NCameraCNN(cfg)))
    a, b = flats
    assert all(b.offset[n] == o for n, o in a.offset.items())
    assert b.offset["roi_embed.weight"] == a.total and b.total == a.total + 128 * 8
    assert b.offset["roi_embed.weight"] > b.offset["resnet.fc.weight"]  # inside the head's gradient bucket


def test_state_dicts_cross_load_as_documented(pair):
    plain, cond = pair[0], pair[1]
    torch.manual_seed(8)
    target = NCameraCNN(COND)
    with torch.no_grad():
        target.roi_embed.weight.fill_(3.0)
    sd = {"module." + k: v for k, v in plain.state_dict().items()}  # a wrapped, unconditioned checkpoint
    res = target.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    assert int(target.roi_embed.weight.count_nonzero()) == 0  # the unconditioned function
    assert all(torch.equal(v, target.state_dict()[k]) for k, v in plain.state_dict().items())
    torch.manual_seed(9)
    other = NCameraCNN(PLAIN)
    with pytest.raises(RuntimeError, match="roi_embed.weight"):  # strict, as every unexpected key
        other.load_state_dict(cond.state_dict())
    short = dict(plain.state_dict())
    del short["output_mlp.4.bias"]
    with pytest.raises(RuntimeError, match="output_mlp.4.bias"):  # every other mismatch as before
        target.load_state_dict(short)


# ---- ValueErrors before any device work -------------------------------------------------------------------------
def test_forward_and_step_refuse_a_mismatched_roi(pair):
    from argus_amd.step import FusedTrainer

    plain, cond = pair[0], pair[1]
    x, roi = torch.rand(2, 6, 64, 64), crop_roi(2, 2, (16, 32), (64, 64), "cpu")
    assert tuple(roi.shape) == (2, 2, 4) and roi[1, 1].tolist() == [16.0, 32.0, 64.0, 64.0]
    with pytest.raises(ValueError, match="pass roi"):
        cond(x)
    with pytest.raises(ValueError, match="without roi_frame_hw"):
        plain(x, roi)
    with pytest.raises(ValueError, match="shape"):
        cond(x, roi[:1])
    with pytest.raises(ValueError, match="float32"):
        cond(x, roi.double())
    with pytest.raises(RuntimeError, match="HIP"):  # a well-formed call reaches the device check, as before
        cond(x, roi)
    torch.manual_seed(3)
    trainers = [FusedTrainer(NCameraCNN(cfg)) for cfg in (PLAIN, COND)]  # FlatParams only: no device work
    T = torch.zeros(2, 7)
    with pytest.raises(ValueError, match="without roi_frame_hw"):
        trainers[0].step_roi(x, T, roi)
    with pytest.raises(ValueError, match="pass roi"):
        trainers[1].step(x, T)
    with pytest.raises(ValueError, match="pass roi"):
        trainers[1].step_roi(x, T, None)
    with pytest.raises(ValueError, match="shape"):
        trainers[1].step_roi(x, T, roi[:1])


def test_sessions_refuse_what_they_do_not_serve(pair):
    from argus_amd.finetune import FineTuneSession
    from argus_amd.infer import InferenceSession
    from argus_amd.infer_grad import GradientSession
    from argus_amd.pose_session import PoseSession

    cond = pair[1]
    for cls in (InferenceSession, GradientSession, FineTuneSession):
        with pytest.raises(ValueError, match="roi_frame_hw"):
            cls(cond, 1, (64, 64), compute_dtype="bf16")
    with pytest.raises(ValueError, match="roi=True"):
        PoseSession(cond, 1, (64, 64), compute_dtype="bf16", frame_hw=ref.FRAME_HW)
    with pytest.raises(ValueError, match="roi_frame_hw"):
        PoseSession(cond, 1, (64, 64), compute_dtype="bf16", frame_hw=(100, 128), roi=True)
    with pytest.raises(ValueError, match="roi_frame_hw"):
        PoseSession(cond, 1, (64, 64), compute_dtype="bf16", roi=True)  # frame_hw defaults to hw
    with pytest.raises(RuntimeError, match="HIP"):  # the served combination reaches the device check
        PoseSession(cond, 1, (64, 64), compute_dtype="bf16", frame_hw=ref.FRAME_HW, roi=True)


def test_validate_refuses_a_session_for_a_conditioned_model(tmp_path, dummy_data_path):
    from argus_amd.data import CameraCubePoseDatasetConfig
    from argus_amd.validate import ValConfig, validate

    path = tmp_path / "m.pth"
    path.write_bytes(b"")
    cfg = ValConfig(str(path), CameraCubePoseDatasetConfig(dummy_data_path), model_config=COND, session_dtype="bf16")
    with pytest.raises(ValueError, match="InferenceSession"):
        validate(cfg)


# ---- --roi-features -------------------------------------------------------------------------------------------
def test_roi_features_flag_validation(tmp_path, dummy_data_path):
    from argus_amd.data import CameraCubePoseDatasetConfig
    from argus_amd.train import TrainConfig, parse_args

    kw = dict(dataset_config=CameraCubePoseDatasetConfig(dummy_data_path), save_dir=str(tmp_path), wandb_log=False)
    for bad in (dict(), dict(resident_dataset=True), dict(roi_jitter=(0.5, 2.0, 0.1))):
        with pytest.raises(ValueError, match="--roi-features needs"):
            TrainConfig(roi_features=True, **bad, **kw)
    with pytest.raises(ValueError, match="--freeze-bn"):
        TrainConfig(roi_features=True, resident_dataset=True, roi_jitter=(0.5, 2.0, 0.1), freeze_bn=True, **kw)
    assert TrainConfig(roi_features=True, resident_dataset=True, roi_jitter=(0.5, 2.0, 0.1), **kw).roi_features
    assert TrainConfig(roi_features=True, resident_dataset=True, roi_track="calib.json", **kw).roi_features
    assert not TrainConfig(**kw).roi_features
    base = ["--dataset-config.dataset-path", dummy_data_path, "--save-dir", str(tmp_path)]
    for bad in ([], ["--resident-dataset"], ["--roi-jitter", "0.5", "2", "0.1"]):
        with pytest.raises(SystemExit):
            parse_args(base + ["--roi-features"] + bad)
    cfg = parse_args(base + ["--roi-features", "--resident-dataset", "--roi-jitter", "0.5", "2", "0.1"])
    assert cfg.roi_features and cfg.resident_dataset and not parse_args(base).roi_features


# ---- the entry points' refusals (no launch: nothing here needs a device) ----------------------------------------
def _embed(**kw):
    from argus_amd._lib import lib

    a = dict(batch=2, n_cams=2, frame_h=96, frame_w=128, h=64, w=64, rois=16, w_r=16, z=16, g=None, rho=None)
    a.update(kw)
    L = lib().dll
    rc = L.argus_roi_embed(a["batch"], a["n_cams"], a["frame_h"], a["frame_w"], a["h"], a["w"], a["rois"], a["w_r"],
                           a["z"], a["g"], a["rho"], None)
    return rc, L.argus_last_error().decode()


@pytest.mark.parametrize("kw,name", [
    (dict(rois=None), "rois"), (dict(w_r=None), "w_r"), (dict(z=None), "z"), (dict(batch=0), "batch"),
    (dict(n_cams=0), "n_cams"), (dict(frame_h=0), "frame_h"), (dict(frame_w=-1), "frame_w"), (dict(h=7), "h"),
    (dict(w=7), "w"), (dict(h=97), "h > frame_h"), (dict(w=129), "w > frame_w"), (dict(n_cams=17), "n_cams")],
    ids=lambda v: v if isinstance(v, str) else "")
def test_roi_embed_refuses_before_a_launch(kw, name):
    rc, msg = _embed(**kw)
    assert rc == 1 and msg.startswith("roi_embed: ") and name in msg


def test_pose_tail_roi_refuses_before_a_launch():
    from argus_amd._lib import lib

    L = lib().dll
    need, small = L.argus_pose_tail_workspace_bytes(16, 128), L.argus_pose_tail_workspace_bytes(2, 128)

    def call(batch=2, d=128, n_cams=2, fh=96, fw=128, h=64, w=64, rois=16, w_r=16, ws=16, nbytes=need, g0=16):
        rc = L.argus_pose_tail_roi(batch, d, g0, *[16] * 8, 0, n_cams, fh, fw, h, w, rois, w_r, ws, nbytes, None)
        return rc, L.argus_last_error().decode()

    for kw, rc_want, name in ((dict(rois=None), 1, "rois"), (dict(w_r=None), 1, "w_r"), (dict(n_cams=0), 1, "n_cams"),
                              (dict(n_cams=17, batch=1), 1, "n_cams"), (dict(h=7), 1, "at least 8"),
                              (dict(h=97), 1, "h > frame_h"), (dict(batch=9), 1, "batch * n_cams"),
                              (dict(batch=17, n_cams=1), 1, "batch 1..16"), (dict(g0=None), 1, "null"),
                              (dict(d=100), 2, "multiple of 64"), (dict(nbytes=small - 1), 1, "workspace")):
        rc, msg = call(**kw)
        assert rc == rc_want and msg.startswith("pose_tail_roi: ") and name in msg, (kw, rc, msg)


# ---- the reference ---------------------------------------------------------------------------------------------
def test_reference_centre_crop_has_zero_features():
    crop = ref.center_crop_roi()
    assert crop.tolist() == [16.0, 32.0, 64.0, 64.0]
    for dtype in (np.float64, np.float32):
        assert not ref.features(np.tile(crop, (2, 1)), 2, dtype=dtype).any()
    # the model's own statement of the definition agrees with the reference
    rois, _, _ = ref.embed_case(3, 2)
    mine = roi_features(torch.from_numpy(rois).double().view(3, 2, 4), ref.FRAME_HW, ref.HW).reshape(3, 8).numpy()
    assert np.allclose(mine, ref.features(rois, 2), rtol=0, atol=1e-15)
    rho = ref.features(rois, 2)
    assert np.abs(rho[:, 0::4]).max() <= 0.5 and np.abs(rho[:, 1::4]).max() <= 0.5
    assert np.abs(rho[:, 2::4]).max() <= np.log(4.0) and np.abs(rho[:, 3::4]).max() <= np.log(4.0)
    assert np.abs(rho[1:]).min() > 0  # the random regions exercise every feature


@pytest.mark.parametrize("batch,n_cams", ref.EMBED_CASES, ids=lambda v: str(v))
def test_fp32_reference_stays_within_a_quarter_of_the_kernel_bar(batch, n_cams):
    """float32 arithmetic alone (numpy, every step rounded) moves z by at most a quarter of what the kernel is
    allowed: the bar is not slack by more than 4x, and the features by at most a quarter of their 4 ulp."""
    rois, w_r, z = ref.embed_case(batch, n_cams)
    rho64, rho32 = ref.features(rois, n_cams), ref.features(rois, n_cams, dtype=np.float32)
    want = ref.embed(z, rho64, w_r)
    got = ref.embed(z, rho32, w_r, dtype=np.float32)
    S = ref.embed_scale(z, rho64, w_r)
    ratio = (np.abs(got.astype(np.float64) - want) / (ref.embed_bar(n_cams) * S)).max()
    ulps = (np.abs(rho32.astype(np.float64) - rho64).reshape(-1, 4) / ref.RHO_ULP).max()
    print(f"roi_embed fp32 numpy ({batch}, {n_cams}): max |z32 - z64| / bar = {ratio:.3f}; rho {ulps:.2f} ulp")
    assert ratio <= 0.25 and ulps <= 1.0
