"""CPU: aiming the region of interest from the pose (argus_amd/track.py, csrc/track.hip). argus_roi_from_pose
declared, bound, exported and refusing every bad call before a launch; the fp64 restatement's domain and clamp share
on the case set; the MuJoCo camera convention; the calibration file; the jitter's draws; the refusals of
PoseSession / ResidentLoader / the CLIs. Nothing here needs a GPU."""
import ctypes as C
import json
import math
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))

import track_reference as ref  # noqa: E402
from argus_amd import resident, track  # noqa: E402
from argus_amd._lib import LIB_PATH, SIGNATURES, ArgusHipError, TrackCfg, lib  # noqa: E402
from argus_amd.pose_session import check_roi  # noqa: E402

NAME = "argus_roi_from_pose"
ERR_ARG = 1
POSES, INDEX, CAMS, JIT, HOME, ROIS, USED, VALID = (1 << 40) + 4096 * np.arange(8)  # never dereferenced: all refused


# ---- the C ABI --------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported_at_abi_21():
    hdr = (ROOT / "include" / "argus_hip.h").read_text()
    declared = set(re.findall(r"^(?:int|size_t|const char\*)\s+(argus_[a-z0-9_]+)\(", hdr, re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (argus_[a-z0-9_]+)$", out, re.M))
    assert NAME in declared and NAME in SIGNATURES and NAME in exported
    assert "typedef struct argus_track_cfg" in hdr and C.sizeof(TrackCfg) == 32
    assert lib().dll.argus_abi_version() == 21  # no bump: the symbol is the detection


def _cfg(**kw):
    f = dict(half_extent=(0.035, 0.035, 0.035), margin=1.5, scale_lo=0.25, scale_hi=4.0, z_near=0.02, smooth=1.0)
    f.update(kw)
    return TrackCfg((C.c_float * 3)(*f["half_extent"]), f["margin"], f["scale_lo"], f["scale_hi"], f["z_near"],
                    f["smooth"])


def _call(cfg=None, **kw):
    a = dict(batch=2, n_cams=2, frame_h=96, frame_w=160, h=64, w=64, poses=int(POSES), n_poses=5, index=int(INDEX),
             cameras=int(CAMS), jitter=int(JIT), home=int(HOME), rois=int(ROIS), used=int(USED), valid=int(VALID))
    a.update(kw)
    c = _cfg() if cfg is None else cfg
    rc = lib().dll.argus_roi_from_pose(a["batch"], a["n_cams"], a["frame_h"], a["frame_w"], a["h"], a["w"], a["poses"],
                                       a["n_poses"], a["index"], a["cameras"], C.byref(c) if c is not False else None,
                                       a["jitter"], a["home"], a["rois"], a["used"], a["valid"], None)
    return rc, lib().dll.argus_last_error().decode()


@pytest.mark.parametrize("arg", ["poses", "cameras", "home", "rois"])
def test_null_pointers_are_refused_by_name(arg):
    rc, msg = _call(**{arg: None})
    assert rc == ERR_ARG and "roi_from_pose" in msg and arg in msg and "null" in msg


def test_null_cfg_is_refused_by_name():
    rc, msg = _call(cfg=False)
    assert rc == ERR_ARG and "cfg" in msg and "null" in msg


@pytest.mark.parametrize("kw,name", [(dict(batch=0), "batch"), (dict(batch=-1), "batch"), (dict(n_cams=0), "n_cams"),
                                     (dict(frame_h=0), "frame_h"), (dict(frame_w=-5), "frame_w"),
                                     (dict(n_poses=0), "n_poses"), (dict(h=7), "at least 8"), (dict(w=7), "at least 8"),
                                     (dict(h=0), "at least 8"), (dict(w=-3), "at least 8"),
                                     (dict(h=97), "h > frame_h"), (dict(w=161), "w > frame_w"),
                                     (dict(index=None, n_poses=1), "n_poses < batch")])
def test_bad_sizes_are_refused_by_name(kw, name):
    rc, msg = _call(**kw)
    assert rc == ERR_ARG and "roi_from_pose" in msg and name in msg


@pytest.mark.parametrize("kw,name", [
    (dict(half_extent=(0.0, 0.1, 0.1)), "half_extent"), (dict(half_extent=(0.1, -0.1, 0.1)), "half_extent"),
    (dict(half_extent=(0.1, 0.1, float("nan"))), "half_extent"), (dict(half_extent=(float("inf"), 0.1, 0.1)), "half_extent"),
    (dict(margin=0.0), "margin"), (dict(margin=float("nan")), "margin"), (dict(margin=float("inf")), "margin"),
    (dict(z_near=0.0), "z_near"), (dict(z_near=-1.0), "z_near"), (dict(z_near=float("nan")), "z_near"),
    (dict(scale_lo=2.0, scale_hi=1.0), "scale_lo"), (dict(scale_lo=float("nan")), "scale_lo"),
    (dict(smooth=0.0), "smooth"), (dict(smooth=1.5), "smooth"), (dict(smooth=-0.1), "smooth"),
    (dict(smooth=float("nan")), "smooth")], ids=str)
def test_bad_settings_are_refused_by_name(kw, name):
    rc, msg = _call(cfg=_cfg(**kw))
    assert rc == ERR_ARG and "roi_from_pose" in msg and name in msg


def test_optional_pointers_and_the_wrapper():
    """index, jitter, used and valid may be null: the next check (here a null home) is the one that fires."""
    rc, msg = _call(index=None, jitter=None, used=None, valid=None, home=None)
    assert rc == ERR_ARG and "home" in msg
    for arg in ("cameras", "home", "rois", "used"):  # 16-byte accesses
        rc, msg = _call(**{arg: int(ROIS) + 4})
        assert rc == ERR_ARG and arg in msg and "aligned" in msg
    with pytest.raises(ArgusHipError, match="smooth"):
        lib().roi_from_pose(2, 2, 96, 160, 64, 64, int(POSES), 5, None, int(CAMS), C.byref(_cfg(smooth=2.0)), None,
                            int(HOME), int(ROIS), None, None, None)


# ---- the restatement on the case set ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return ref.case_set()


def _ref(cases, **kw):
    poses, cams, _ = cases
    return ref.roi_from_pose(poses, cams, ref.FRAME_HW, ref.HW, ref.HALF_EXTENT, ref.MARGIN, ref.Z_NEAR, **kw)


@pytest.mark.parametrize("smooth", [1.0, 0.3])
@pytest.mark.parametrize("jitter", [False, True], ids=["plain", "jitter"])
def test_restatement_stays_in_check_rois_domain_and_is_mostly_unclamped(cases, smooth, jitter):
    j = cases[2] if jitter else None
    r64 = _ref(cases, smooth=smooth, jitter=j)
    r32 = _ref(cases, smooth=smooth, jitter=j, dtype=np.float32)
    n = 2 * ref.N_POSES
    for r in (r64, r32):
        assert r["rois"].shape == (n, 4) and r["rois"].dtype == np.float32
        check_roi(torch.from_numpy(r["rois"]).reshape(n, 1, 4), ref.FRAME_HW, ref.HW)  # raises on any violation
    share = 1.0 - r64["touched"].mean()
    worst = np.abs(r64["rois"].astype(np.float64) - r32["rois"]).max()
    print(f"valid {r64['valid'].mean():.3f}  unclamped {share:.3f}  |fp32 - fp64| {worst:.2e} px")
    assert np.array_equal(r64["valid"], r32["valid"])
    assert 0.9 < r64["valid"].mean() < 0.96
    assert share >= 0.25  # the parity check of the GPU test is not carried by clamped values
    assert worst <= ref.TOL_PX / 5 * 1.01  # the tolerance is five times the restatement's own error
    home = ref.center_home(n)
    bad = r64["valid"] == 0
    assert bad.sum() >= 2 * 30 and np.array_equal(r64["rois"][bad], home[bad])
    assert bad.reshape(-1, 2)[50:80].all()  # the zero quaternions, the NaN and the infinite translations


def test_case_set_has_no_depth_at_the_threshold(cases):
    """Validity is compared everywhere on the GPU: no corner depth lies within 1e-4 (relative) of z_near."""
    d = _ref(cases)["depth"]
    assert np.nanmin(np.abs(d - np.float32(ref.Z_NEAR)) / ref.Z_NEAR) > 1e-4


def test_restatement_details(cases):
    poses, cams, jit = cases
    base = _ref(cases)
    # an index gathers and clamps
    idx = np.array([5, -3, 4095, 1 << 40, 77])
    r = _ref(cases, index=idx)
    want = base["rois"].reshape(-1, 2, 4)[[5, 0, 4095, 4095, 77]].reshape(-1, 4)
    assert np.array_equal(r["rois"], want)
    # smoothing starts from prev; used is prev
    prev = np.tile(np.float32([10, 20, 48, 48]), (2 * ref.N_POSES, 1))
    s = _ref(cases, smooth=0.5, prev=prev)
    assert np.array_equal(s["used"], prev) and not np.array_equal(s["rois"], base["rois"])
    ok = (base["touched"] | s["touched"]) == 0
    mid = 0.5 * (base["rois"][ok, 2].astype(np.float64) + 48.0)
    assert ok.sum() > 100 and np.abs(s["rois"][ok, 2] - mid).max() < 1e-4
    # a centered cube in front of a camera looking down +z: the box of its projected corners, times the margin
    cam = np.float32([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 100, 100, 80, 48])
    one = ref.roi_from_pose(np.float32([[0, 0, 0.5, 0, 0, 0, 2]]), cam[None], (96, 160), (64, 64), (0.05,) * 3, 1.5, 0.02)
    e = 1.5 * 2 * 100 * 0.05 / 0.45  # the near face
    assert one["valid"][0] == 1 and np.allclose(one["rois"][0], [48 - e / 2, 80 - e / 2, e, e], atol=1e-4)


# ---- cameras ----------------------------------------------------------------------------------------------
def _project(cam: track.Camera, X):
    Y = np.array(cam.R).reshape(3, 3) @ np.asarray(X, dtype=np.float64) + np.array(cam.t)
    return cam.fx * Y[0] / Y[2] + cam.cx, cam.fy * Y[1] / Y[2] + cam.cy, Y[2]


def test_camera_from_mujoco_convention():
    Hs, Ws, fovy = 96, 160, 70.0
    pos = np.array([0.3, -0.2, 0.5])
    q = np.array([0.9, 0.1, -0.3, 0.2])
    q /= np.linalg.norm(q)
    w, x, y, z = q
    Rwc = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    cam = track.camera_from_mujoco(pos, q * 3.0, fovy, (Hs, Ws))  # an unnormalised quaternion is normalised
    assert cam.fx == cam.fy == pytest.approx((Hs / 2) / math.tan(math.radians(fovy) / 2))
    assert (cam.cx, cam.cy) == (Ws / 2, Hs / 2)
    world = lambda p: pos + Rwc @ np.asarray(p, dtype=np.float64)  # noqa: E731  camera frame (MuJoCo's) -> world
    u, v, depth = _project(cam, world([0, 0, -2.0]))  # on the optical axis: the principal point, in front
    assert (u, v) == pytest.approx((Ws / 2, Hs / 2)) and depth == pytest.approx(2.0)
    assert _project(cam, world([0.1, 0, -2.0]))[0] > u and _project(cam, world([0.1, 0, -2.0]))[1] == pytest.approx(v)
    assert _project(cam, world([0, 0.1, -2.0]))[1] < v  # MuJoCo's +y is up: the row decreases
    assert _project(cam, world([0, -0.1, -2.0]))[1] > v
    edge = 2.0 * math.tan(math.radians(fovy) / 2)
    assert _project(cam, world([0, edge, -2.0]))[1] == pytest.approx(0.0, abs=1e-9)   # the top row's upper edge
    assert _project(cam, world([0, -edge, -2.0]))[1] == pytest.approx(Hs, abs=1e-9)  # the bottom row's lower edge
    R = np.array(cam.R).reshape(3, 3)
    assert np.allclose(R @ R.T, np.eye(3)) and np.linalg.det(R) == pytest.approx(1.0)
    assert cam.words().dtype == np.float32 and cam.words().shape == (16,)
    for bad in (dict(fovy_deg=0.0), dict(fovy_deg=180.0), dict(quat_wxyz=(0, 0, 0, 0)), dict(pos=(1, 2))):
        kw = dict(pos=pos, quat_wxyz=q, fovy_deg=fovy, frame_hw=(Hs, Ws))
        kw.update(bad)
        with pytest.raises(ValueError, match="camera_from_mujoco"):
            track.camera_from_mujoco(**kw)


def test_look_at_camera_of_the_reference_agrees_with_the_mujoco_form():
    """A look-at camera through the other door: a MuJoCo camera with the same axes gives the same 16 words (an eye
    off the case set's plane: their rotations are half turns, where this conversion to a quaternion divides by 0)."""
    eye = (0.1, 0.15, 0.13)
    words = ref.look_at_camera(eye, (0, 0, 0), 70.0, ref.FRAME_HW)
    R = words[:9].reshape(3, 3).astype(np.float64)
    Rwc = (np.diag([1.0, -1.0, -1.0]) @ R).T  # MuJoCo's camera axes in the world
    w = math.sqrt(max(0.0, 1 + np.trace(Rwc))) / 2
    q = np.array([w, (Rwc[2, 1] - Rwc[1, 2]) / (4 * w), (Rwc[0, 2] - Rwc[2, 0]) / (4 * w), (Rwc[1, 0] - Rwc[0, 1]) / (4 * w)])
    assert w > 0.1
    cam = track.camera_from_mujoco(eye, q, 70.0, ref.FRAME_HW)
    assert np.allclose(cam.words(), words, atol=1e-6)
    assert _project(cam, (0, 0, 0))[:2] == pytest.approx((80.0, 48.0), abs=1e-4)


# ---- the calibration file ---------------------------------------------------------------------------------
def _calib():
    R = ref.look_at_camera((0.0, 0.15, 0.13), (0, 0, 0), 70.0, ref.FRAME_HW).astype(np.float64)
    return {"cameras": [{"R": R[:9].tolist(), "t": R[9:12].tolist(), "fx": R[12], "fy": R[13], "cx": R[14], "cy": R[15]},
                        {"mujoco": {"pos": [0.0, -0.15, 0.13], "quat": [0.5, 0.5, 0.5, 0.5], "fovy": 70.0}}],
            "frame_hw": [96, 160], "half_extent": 0.035, "z_near": 0.02}


def test_load_calibration_round_trips_both_camera_forms(tmp_path):
    d = _calib()
    p = tmp_path / "calib.json"
    p.write_text(json.dumps(d))
    cfg = track.load_calibration(p)
    assert isinstance(cfg, track.TrackConfig) and len(cfg.cameras) == 2
    assert cfg.half_extent == (0.035,) * 3 and cfg.z_near == 0.02
    assert (cfg.margin, cfg.scale, cfg.smooth, cfg.home) == (1.5, (0.25, 4.0), 1.0, None)  # the defaults
    assert cfg.cameras[0] == track.Camera(**d["cameras"][0])
    m = d["cameras"][1]["mujoco"]
    assert cfg.cameras[1] == track.camera_from_mujoco(m["pos"], m["quat"], m["fovy"], (96, 160))
    assert cfg.camera_words().shape == (2, 16) and cfg.camera_words().dtype == np.float32
    d.update(margin=1.25, scale=[0.5, 2.0], smooth=0.5, home=[16, 48, 64, 64], half_extent=[0.01, 0.02, 0.03])
    p.write_text(json.dumps(d))
    cfg = track.load_calibration(str(p))
    assert (cfg.margin, cfg.scale, cfg.smooth, cfg.home) == (1.25, (0.5, 2.0), 0.5, [16, 48, 64, 64])
    s = cfg.struct()
    assert list(s.half_extent) == [np.float32(v) for v in (0.01, 0.02, 0.03)] and s.smooth == 0.5
    assert cfg.struct(smooth=1.0).smooth == 1.0


@pytest.mark.parametrize("edit,word", [
    (lambda d: d.pop("cameras"), "'cameras'"), (lambda d: d.pop("half_extent"), "'half_extent'"),
    (lambda d: d.pop("z_near"), "'z_near'"), (lambda d: d.pop("frame_hw"), "'frame_hw'"),
    (lambda d: d["cameras"][0].pop("fx"), "cameras[0].'fx'"), (lambda d: d["cameras"][0].update(R=[1, 2, 3]), "cameras[0]"),
    (lambda d: d["cameras"][1]["mujoco"].pop("quat"), "cameras[1].mujoco.'quat'"),
    (lambda d: d["cameras"][1]["mujoco"].update(fovy="wide"), "fovy"),
    (lambda d: d.update(cameras=[]), "'cameras'"), (lambda d: d.update(smooth=0), "smooth"),
    (lambda d: d.update(scale=[2, 1]), "scale"), (lambda d: d.update(margn=2), "'margn'")])
def test_load_calibration_names_the_bad_key(tmp_path, edit, word):
    d = _calib()
    edit(d)
    p = tmp_path / "calib.json"
    p.write_text(json.dumps(d))
    with pytest.raises(ValueError, match="calibration") as e:
        track.load_calibration(p)
    assert word in str(e.value)
    p.write_text("{not json")
    with pytest.raises(ValueError, match="not JSON"):
        track.load_calibration(p)


def test_track_config_validates():
    cam = track.Camera(np.eye(3), (0, 0, 0), 100, 100, 80, 48)
    assert track.TrackConfig([cam], 0.05, z_near=0.02).half_extent == (0.05, 0.05, 0.05)
    for kw in (dict(half_extent=0.0), dict(half_extent=(1, 2)), dict(margin=-1), dict(z_near=0), dict(smooth=0),
               dict(smooth=1.1), dict(scale=(2, 1)), dict(cameras=[]), dict(cameras=[np.zeros(16)])):
        a = dict(cameras=[cam], half_extent=0.05, z_near=0.02)
        a.update(kw)
        with pytest.raises(ValueError):
            track.TrackConfig(**a)
    with pytest.raises(ValueError, match="fx"):
        track.Camera(np.eye(3), (0, 0, 0), 0, 100, 80, 48)


# ---- the jitter -------------------------------------------------------------------------------------------
def test_sample_roi_jitter_consumes_a_generator_as_sample_rois_does():
    r1, r2 = np.random.RandomState(11), np.random.RandomState(11)
    j = track.sample_roi_jitter(r1, 50, scale=(0.5, 2.0), shift=0.3)
    resident.sample_rois(r2, 50, (376, 672), (256, 256), (60, 208), scale=(0.5, 2.0), shift=0.3)
    assert j.shape == (50, 3) and j.dtype == np.float32
    assert np.array_equal(r1.uniform(size=5), r2.uniform(size=5))  # both stand at the same place: 3 draws an image
    # and they are the same draws: sample_rois' unclipped scale is exp of the first
    r3 = np.random.RandomState(11)
    u = r3.uniform([math.log(0.5), -0.3, -0.3], [math.log(2.0), 0.3, 0.3], size=(50, 3))
    assert np.array_equal(j, u.astype(np.float32))
    assert np.abs(j[:, 0]).max() <= math.log(2.0) + 1e-6 and np.abs(j[:, 1:]).max() <= 0.3 + 1e-6
    assert np.array_equal(track.sample_roi_jitter(np.random.RandomState(0), 4), np.zeros((4, 3), dtype=np.float32))
    for kw in (dict(scale=(2, 1)), dict(scale=(0, 1)), dict(shift=-0.1)):
        with pytest.raises(ValueError, match="sample_roi_jitter"):
            track.sample_roi_jitter(np.random.RandomState(0), 4, **kw)


# ---- refusals of the session, the loader and the CLIs -----------------------------------------------------
def _track(n_cams=2):
    cams = [track.Camera(w[:9], w[9:12], *w[12:]) for w in ref.case_set()[1][:n_cams].astype(np.float64)]
    return track.TrackConfig(cams, ref.HALF_EXTENT, margin=ref.MARGIN, z_near=ref.Z_NEAR)


def test_pose_session_refusals():
    from argus_amd.models import NCameraCNN
    from argus_amd.pose_session import PoseSession

    model = NCameraCNN()
    kw = dict(compute_dtype="bf16", frame_hw=(96, 160))
    with pytest.raises(ValueError, match="fused_head"):
        PoseSession(model, 1, (64, 64), track=_track(), fused_head=False, **kw)
    with pytest.raises(ValueError, match="cameras"):
        PoseSession(model, 1, (64, 64), track=_track(1), **kw)
    with pytest.raises(ValueError, match="TrackConfig"):
        PoseSession(model, 1, (64, 64), track={"cameras": []}, **kw)
    with pytest.raises(RuntimeError, match="HIP"):  # a valid request: no CPU fallback
        PoseSession(model, 1, (64, 64), track=_track(), **kw)


class _FakeTensor:
    def __init__(self, shape):
        self.shape = shape


def _fake_dataset(full_frames):
    from argus_amd.data import AugmentationConfig

    ds = resident.ResidentDataset.__new__(resident.ResidentDataset)
    ds.device = torch.device("cuda", 0)
    ds.cfg_aug = AugmentationConfig(num_spaghetti=10)
    ds.n_cams, ds.src_hw, ds.crop_hw, ds.crop_origin = 2, (376, 672), (256, 256), (60, 208)
    ds.full_frames = full_frames
    ds.images = _FakeTensor((10, 6, 376, 672) if full_frames else (10, 6, 256, 256))
    return ds


def test_resident_loader_refusals(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self, *a, **k: self)
    with pytest.raises(ValueError, match="full_frames"):
        resident.ResidentLoader(_fake_dataset(False), batch_size=4, roi_track=_track())
    with pytest.raises(ValueError, match="cameras"):
        resident.ResidentLoader(_fake_dataset(True), batch_size=4, roi_track=_track(1))
    with pytest.raises(ValueError, match="TrackConfig"):
        resident.ResidentLoader(_fake_dataset(True), batch_size=4, roi_track="calib.json")
    ds = _fake_dataset(True)
    ds.device = torch.device("cpu")
    with pytest.raises(RuntimeError, match="HIP"):
        resident.ResidentLoader(ds, batch_size=4, roi_track=_track())


def test_roi_track_flag_parses_and_needs_the_resident_dataset(tmp_path, capsys):
    from conftest import make_dummy_dataset

    from argus_amd.train import TrainConfig, parse_args

    d = make_dummy_dataset(tmp_path)
    base = ["--dataset-config.dataset-path", d, "--save-dir", str(tmp_path / "m")]
    assert parse_args(base).roi_track is None and TrainConfig.__dataclass_fields__["roi_track"].default is None
    cfg = parse_args(base + ["--resident-dataset", "--roi-track", "calib.json"])
    assert cfg.resident_dataset is True and cfg.roi_track == "calib.json" and cfg.roi_jitter is None
    cfg = parse_args(base + ["--resident-dataset", "--roi-track", "c.json", "--roi-jitter", "0.5", "2", "0.1"])
    assert cfg.roi_track == "c.json" and tuple(cfg.roi_jitter) == (0.5, 2, 0.1)
    for argv in (["--roi-track", "calib.json"], ["--no-resident-dataset", "--roi-track", "calib.json"]):
        with pytest.raises(SystemExit):
            parse_args(base + argv)
        assert "--roi-track" in capsys.readouterr().err
    with pytest.raises(ValueError, match="resident"):
        TrainConfig(save_dir=str(tmp_path / "m"), dataset_config=cfg.dataset_config, roi_track="calib.json")


def test_timing_cli_parses_track(monkeypatch, capsys, tmp_path):
    """main() with pose_latency replaced: what the command line hands to the measurement."""
    from argus_amd import timing

    seen = []

    def fake(*args, **kw):
        seen.append(kw)
        return {"mean_s": 0.0}

    monkeypatch.setattr(timing, "pose_latency", fake)
    p = tmp_path / "calib.json"
    p.write_text(json.dumps(_calib()))
    timing.main(["--frozen", "--pose", "--frame-hw", "96", "160", "--hw", "64", "64", "--track", str(p)])
    timing.main(["--frozen", "--pose"])
    assert isinstance(seen[0]["track"], track.TrackConfig) and len(seen[0]["track"].cameras) == 2
    assert seen[1]["track"] is None
    for bad in (["--track", str(p), "--parent"], ["--track", str(tmp_path / "missing.json")]):
        with pytest.raises(SystemExit):
            timing.main(["--frozen", "--pose", *bad])
        assert "--track" in capsys.readouterr().err
    assert len(seen) == 2
