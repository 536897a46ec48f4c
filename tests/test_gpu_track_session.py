"""GPU: the closed loop. PoseSession(track=...) ends every forward with argus_roi_from_pose, so a replay reads the
region the previous replay wrote; ResidentLoader(roi_track=...) aims the training regions at the labelled cube with
the same launch; train --roi-track end to end.

The cameras are built from a first untracked pose, so the predicted cube sits about 0.2 in front of each camera and
projects inside the frame: the tracker has something to follow. Parity with the restatement is at
track_reference.TOL_PX (2^-7 px)."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import track_reference as ref  # noqa: E402
from test_gpu_infer import _randomize_bn  # noqa: E402

from argus_amd import resident, track  # noqa: E402
from argus_amd.pose_session import check_roi  # noqa: E402

pytestmark = pytest.mark.gpu

HW, FHW = (64, 64), (96, 160)
HOME = [16.0, 48.0, 64.0, 64.0]


@pytest.fixture(scope="module")
def model(cuda):
    from argus_amd.models import NCameraCNN

    torch.manual_seed(11)
    m = NCameraCNN(compute_dtype="bf16")
    _randomize_bn(m)
    return m.to(cuda).eval()


def _cameras_around(center, distance=0.2):
    """Two look-at cameras ``distance`` from ``center``, to its sides and above, aimed at it."""
    c = np.asarray(center, dtype=np.float64)
    off = distance * np.array([0.0, 0.15, 0.13]) / np.hypot(0.15, 0.13)
    words = [ref.look_at_camera(c + off * [1, s, 1], c, 70.0, FHW) for s in (1.0, -1.0)]
    return [track.Camera(w[:9], w[9:12], *w[12:]) for w in np.float64(words)]


def _config(cams, smooth=1.0, **kw):
    return track.TrackConfig(cams, ref.HALF_EXTENT, margin=ref.MARGIN, z_near=ref.Z_NEAR, smooth=smooth, **kw)


def _restate(cfg, pose, prev, smooth):
    return ref.roi_from_pose(pose.cpu().numpy(), cfg.camera_words(), FHW, HW, ref.HALF_EXTENT, ref.MARGIN, ref.Z_NEAR,
                             smooth=smooth, prev=prev.reshape(-1, 4).numpy())


@pytest.mark.parametrize("batch,smooth", [(1, 1.0), (2, 0.5)], ids=["b1", "b2-smooth"])
def test_tracked_session_closes_the_loop_on_the_device(cuda, model, batch, smooth):
    from argus_amd.pose_session import PoseSession

    g = torch.Generator().manual_seed(100 + batch)
    frames = [torch.randint(0, 256, (batch, 6, *FHW), generator=g, dtype=torch.uint8).to(cuda) for _ in range(6)]
    kw = dict(compute_dtype="bf16", frame_hw=FHW)
    plain = PoseSession(model, batch, HW, **kw)
    first = plain.pose(frames[0])
    cfg = _config(_cameras_around(first[:, :3].double().mean(0).cpu().numpy()), smooth)
    tracked = PoseSession(model, batch, HW, track=cfg, **kw)
    open_loop = PoseSession(model, batch, HW, roi=True, **kw)
    eager = PoseSession(model, batch, HW, track=cfg, graph=False, **kw)
    home = torch.tensor(HOME).expand(batch, 2, 4)

    # (vii) one more launch, and only with track
    assert plain.launches_per_forward == open_loop.launches_per_forward == 55
    assert tracked.launches_per_forward == eager.launches_per_forward == 56
    assert tracked.has_roi and open_loop.last_roi is None and open_loop.roi_valid is None and plain.roi is None
    assert torch.equal(tracked.roi, home) and torch.equal(tracked.last_roi, home)  # before the first replay
    with pytest.raises(ValueError, match="track"):
        open_loop.reset_roi()

    # (i) the first tracked pose is the untracked one: the warm-up in front of the capture did not move the tracker
    p0 = tracked.pose(frames[0])
    assert torch.equal(p0, first) and torch.equal(tracked.last_roi, home)
    assert bool((tracked.roi_valid == 1).all())  # the cameras were built around this pose
    assert not torch.equal(tracked.roi, home)    # and the tracker did move
    assert torch.equal(eager.pose(frames[0]), first)

    # (ii), (iii), (iv): four more frames
    pose, moved = p0, 0
    for k in range(1, 5):
        region, prev = tracked.roi, tracked.last_roi
        # (iii) the device region is the restatement of the pose the last call returned
        want = _restate(cfg, pose, prev, smooth)
        err = np.abs(region.reshape(-1, 4).numpy().astype(np.float64) - want["rois"])
        print(f"frame {k}: region {region.reshape(-1, 4)[0].tolist()}  |gpu - fp64| {err.max():.3e} px  valid "
              f"{tracked.roi_valid.reshape(-1).tolist()}")
        near = (np.abs(want["depth"] - np.float32(ref.Z_NEAR)) <= 1e-4 * ref.Z_NEAR).any(1)
        assert np.array_equal(tracked.roi_valid.reshape(-1).numpy()[~near], want["valid"][~near])
        assert err[~near].max() <= ref.TOL_PX
        check_roi(region, FHW, HW)
        assert torch.equal(eager.roi, region) and torch.equal(eager.roi_valid, tracked.roi_valid)
        # (ii) the replay reads what the previous replay wrote: the open-loop session handed that region agrees
        pose = tracked.pose(frames[k])
        assert torch.equal(pose, open_loop.pose(frames[k], roi=region))
        assert torch.equal(tracked.last_roi, region)
        assert torch.equal(eager.pose(frames[k]), pose)  # (iv) graph=False, bit for bit
        moved += int(not torch.equal(tracked.roi, region))
    assert moved >= 2  # different frames, different poses, different regions

    # (v) activation_peak is a measurement, not a frame of the sequence
    state = (tracked.roi, tracked.last_roi, tracked.roi_valid)
    assert tracked.activation_peak(frames[5]) > 0
    assert all(torch.equal(a, b) for a, b in zip(state, (tracked.roi, tracked.last_roi, tracked.roi_valid)))

    # (viii) uint8 and fp32 frames have a graph each and one tracker state
    region = tracked.roi
    f32 = frames[5].float() / 255.0
    pose = tracked.pose(f32)  # the first fp32 call: warm-up, capture, replay
    assert torch.equal(pose, open_loop.pose(f32, roi=region)) and torch.equal(tracked.last_roi, region)
    region = tracked.roi
    assert torch.equal(tracked.pose(frames[1]), open_loop.pose(frames[1], roi=region))

    # (vi) reset_roi and set_roi
    tracked.reset_roi()
    assert torch.equal(tracked.roi, home)
    assert torch.equal(tracked.pose(frames[2]), plain.pose(frames[2])) and torch.equal(tracked.last_roi, home)
    mine = torch.tensor([3.5, 70.25, 40.0, 80.0])
    tracked.set_roi(mine)  # an external detector re-acquires the cube
    assert torch.equal(tracked.pose(frames[3]), open_loop.pose(frames[3], roi=mine))
    assert torch.equal(tracked.last_roi, mine.expand(batch, 2, 4)) and not torch.equal(tracked.roi, tracked.last_roi)
    assert torch.equal(tracked.pose(frames[4], roi=mine), open_loop.pose(frames[4], roi=mine))


def test_home_and_the_unfused_stem(cuda, model):
    """TrackConfig.home is validated and used; fused_stem=False tracks through argus_frames_resample (58 launches),
    which reads the same buffer; a pose that puts the cube behind the cameras sends the region home."""
    from argus_amd.pose_session import PoseSession

    g = torch.Generator().manual_seed(7)
    frames = [torch.randint(0, 256, (1, 6, *FHW), generator=g, dtype=torch.uint8).to(cuda) for _ in range(3)]
    kw = dict(compute_dtype="bf16", frame_hw=FHW)
    plain = PoseSession(model, 1, HW, **kw)
    center = plain.pose(frames[0])[0, :3].double().cpu().numpy()
    cams = _cameras_around(center)
    mine = [3.5, 70.25, 40.0, 80.0]
    with pytest.raises(ValueError, match="roi inside the frame"):
        PoseSession(model, 1, HW, track=_config(cams, home=[40.0, 0.0, 64.0, 64.0]), **kw)
    unfused = PoseSession(model, 1, HW, track=_config(cams, home=mine), fused_stem=False, **kw)
    open_loop = PoseSession(model, 1, HW, roi=True, fused_stem=False, **kw)
    assert unfused.launches_per_forward == 58 and open_loop.launches_per_forward == 57
    assert unfused.roi.reshape(-1, 4).tolist() == [mine] * 2
    moved = 0
    for f in frames:
        region = unfused.roi
        assert torch.equal(unfused.pose(f), open_loop.pose(f, roi=region)) and torch.equal(unfused.last_roi, region)
        moved += int(not torch.equal(unfused.roi, region))
    assert moved >= 2
    # cameras that look away from the cube: invalid, home
    turn = np.diag([-1.0, 1.0, -1.0])  # half a turn about the camera's y axis
    away = [track.Camera(turn @ np.array(c.R).reshape(3, 3), turn @ np.array(c.t), c.fx, c.fy, c.cx, c.cy) for c in cams]
    lost = PoseSession(model, 1, HW, track=_config(away, home=mine), **kw)
    lost.set_roi([16.0, 48.0, 64.0, 64.0])
    lost.pose(frames[0])
    assert lost.roi_valid.tolist() == [[0, 0]] and lost.roi.reshape(-1, 4).tolist() == [mine] * 2
    assert lost.last_roi.reshape(-1, 4).tolist() == [HOME] * 2


# ---- the resident loader ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_frames(cuda, tmp_path_factory):
    from conftest import make_dummy_dataset

    from argus_amd.data import AugmentationConfig, CameraCubePoseDatasetConfig

    path = make_dummy_dataset(tmp_path_factory.mktemp("track"), hw=FHW)
    cfg = CameraCubePoseDatasetConfig(dataset_path=path, center_crop=HW)
    ds = resident.ResidentDataset(cfg, AugmentationConfig(num_spaghetti=10), train=True, device=cuda, num_workers=0,
                                  full_frames=True)
    t = ds.poses[:, :3].double().cpu().numpy()
    spread = np.abs(t - t.mean(0)).max()
    cams = _cameras_around(t.mean(0), distance=max(0.2, 3.0 * spread))  # every labelled cube in front of both
    return path, ds, cams


@pytest.mark.parametrize("jitter", [None, (0.5, 2.0, 0.3)], ids=["plain", "jitter"])
def test_loader_aims_the_regions_at_the_labelled_cube(cuda, full_frames, jitter):
    from argus_amd._lib import lib, ptr, stream

    _, ds, cams = full_frames
    cfg = _config(cams, smooth=0.5)  # the loader forces smooth to 1: a batch has no previous frame
    assert tuple(ds.images.shape) == (10, 6, *FHW) and ds.crop_origin == (16, 48)
    kw = dict(batch_size=3, shuffle=True, seed=9, roi_jitter=jitter, roi_seed=123)
    loader = resident.ResidentLoader(ds, roi_track=cfg, **kw)
    off = resident.ResidentLoader(ds, **kw)
    got = [{k: v.clone() for k, v in b.items()} for b in loader]
    assert len(got) == 4 and all(torch.equal(a["images"], b["images"]) for a, b in zip(got, loader))  # reproducible
    order = loader.indices()
    arc_rng, roi_rng = np.random.RandomState(9), np.random.RandomState(123)
    rng_on, rng_off = loader.host_generators(), off.host_generators()
    poses = ds.poses.cpu().numpy()
    valid_seen = 0
    for k, b in enumerate(got):
        idx = order[3 * k:3 * k + 3]
        nb = len(idx)
        assert tuple(b["roi"].shape) == (nb, 2, 4) and tuple(b["roi_valid"].shape) == (nb, 2)
        assert b["roi_valid"].dtype == torch.int32 and torch.equal(b["cube_pose"], ds.poses[idx])
        jit = None if jitter is None else track.sample_roi_jitter(roi_rng, 2 * nb, jitter[:2], jitter[2])
        want = ref.roi_from_pose(poses, cfg.camera_words(), FHW, HW, ref.HALF_EXTENT, ref.MARGIN, ref.Z_NEAR, index=idx,
                                 jitter=jit, smooth=1.0)
        roi = b["roi"].reshape(-1, 4).cpu()
        err = np.abs(roi.numpy().astype(np.float64) - want["rois"])
        print(f"batch {k}: largest |gpu - fp64| {err.max():.3e} px, valid {b['roi_valid'].reshape(-1).tolist()}")
        assert err.max() <= ref.TOL_PX and np.array_equal(b["roi_valid"].reshape(-1).cpu().numpy(), want["valid"])
        check_roi(roi.reshape(-1, 1, 4), FHW, HW)
        valid_seen += int(want["valid"].sum())
        # the images are argus_batch_gather_resample's on that region and the epoch's arcs
        recs = resident.arc_records(resident.sample_arcs(arc_rng, 2 * nb, 10, ds.src_hw))
        arcs = torch.from_numpy(recs.reshape(-1)).to(cuda)
        index = torch.tensor(idx, dtype=torch.int64, device=cuda)
        out = torch.full((nb, 6, *HW), 0xA5, dtype=torch.uint8, device=cuda)
        lib().batch_gather_resample(nb, 2, *FHW, *HW, ptr(ds.images), len(ds), ptr(index), ptr(b["roi"]), ptr(arcs), 10,
                                    ptr(out), stream())
        torch.cuda.synchronize()
        assert torch.equal(out, b["images"]) and (out == 0).any()
        # the arc records of the pinned slot are the same bytes with roi_track on and off
        words = nb * (2 + loader._roi_words + 2 * 10 * resident.ARC_WORDS)
        hv_on, hv_off = np.zeros(words, dtype=np.int32), np.zeros(words, dtype=np.int32)
        a_on, a_off = loader.fill_slot(hv_on, idx, *rng_on), off.fill_slot(hv_off, idx, *rng_off)
        assert a_on == a_off and np.array_equal(hv_on[a_on:], hv_off[a_off:]) and hv_on[a_on:].any()
        assert np.array_equal(hv_on[a_on:], recs.reshape(-1))
        if jitter is not None:  # three floats an image in the regions' slot, its stride kept
            assert np.array_equal(hv_on[2 * nb:2 * nb + 6 * nb].view(np.float32).reshape(-1, 3), jit)
    assert valid_seen >= 10  # the cameras were placed to see the cubes
    assert not any(torch.equal(a["roi"], b["roi"]) for a, b in zip(got, off))  # and the regions did move


def test_train_with_roi_track_end_to_end(cuda, full_frames, tmp_path, monkeypatch):
    from argus_amd import _lib
    from argus_amd.train import parse_args, train

    path, _, cams = full_frames
    calib = tmp_path / "calib.json"
    calib.write_text(json.dumps({
        "cameras": [{"R": list(c.R), "t": list(c.t), "fx": c.fx, "fy": c.fy, "cx": c.cx, "cy": c.cy} for c in cams],
        "half_extent": 0.035, "z_near": 0.02}))
    calls = []
    L = _lib.lib()
    for name in ("roi_from_pose", "batch_gather_resample", "batch_gather_occlude"):
        fn = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _fn=fn, _name=name: (calls.append(_name), _fn(*a))[1])
    save = tmp_path / "m"
    train(parse_args(["--dataset-config.dataset-path", path, "--dataset-config.center-crop", "64", "64", "--save-dir",
                      str(save), "--batch-size", "5", "--learning-rate", "1e-3", "--n-epochs", "1", "--device", "cuda",
                      "--max-grad-norm", "100.0", "--random-seed", "42", "--val-epochs", "1", "--print-epochs", "1",
                      "--save-epochs", "1", "--no-compile-model", "--no-wandb-log", "--num-workers", "0",
                      "--resident-dataset", "--roi-track", str(calib), "--roi-jitter", "0.7", "1.4", "0.1"]))
    # one epoch of two steps: the train split through both launches, the validation split through the cropped store's
    assert calls.count("roi_from_pose") == 2 and calls.count("batch_gather_resample") == 2
    assert calls.count("batch_gather_occlude") >= 1
    (pth,) = list(save.glob("*.pth"))
    sd = torch.load(pth, weights_only=True)
    assert int(sd["resnet.bn1.num_batches_tracked"]) == 2
    assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
