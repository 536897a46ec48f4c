"""GPU: the resident loader's region of interest (argus_batch_gather_resample, csrc/resident.hip;
ResidentDataset(full_frames=True), ResidentLoader(roi_jitter=...), train --roi-jitter): bit-equal to the cropped
store's launch at unit scale, exact on the integer construction, within half a step of the fp64 restatement
(arc_reference.occlude on the full frame, then roi_reference.resample) on general regions, within the number
formats of what argus_frames_resample deploys, and the loader and the CLI end to end.

Every kernel launch here runs twice, on outputs pre-filled with two different sentinels: equal results mean every
byte was written (and that two calls agree)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arc_reference as ref  # noqa: E402
import roi_reference as roi  # noqa: E402

from argus_amd import resident  # noqa: E402

pytestmark = pytest.mark.gpu

# |out - 255 ref| <= 0.5 + 2^-9: rintf's half step plus the fp32 chain (about 44 roundings on values <= 1: at most
# 7e-4 of a step; 2^-9 is three times that)
BAR = 0.5 + 2.0 ** -9


def _launch(store, index, rois, arcs, n_arcs, hw, n_samples=None):
    """out (B, C, h, w) uint8 of argus_batch_gather_resample; two launches on different sentinels must agree."""
    from argus_amd._lib import lib, ptr, stream

    n, c, Hs, Ws = store.shape
    outs = []
    for sentinel in (0xA5, 0x5A):
        out = torch.full((index.numel(), c, *hw), sentinel, dtype=torch.uint8, device=store.device)
        lib().batch_gather_resample(index.numel(), c // 3, Hs, Ws, hw[0], hw[1], ptr(store),
                                    n if n_samples is None else n_samples, ptr(index), ptr(rois), ptr(arcs), n_arcs,
                                    ptr(out), stream())
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])  # every byte written, and deterministic
    return outs[0]


def _occlude_launch(store, index, arcs, n_arcs, crop):
    from argus_amd._lib import lib, ptr, stream

    n, c, h, w = store.shape
    out = torch.full((index.numel(), c, h, w), 0xA5, dtype=torch.uint8, device=store.device)
    lib().batch_gather_occlude(index.numel(), c // 3, h, w, ptr(store), n, ptr(index), ptr(arcs), n_arcs, crop[0],
                               crop[1], ptr(out), stream())
    torch.cuda.synchronize()
    return out


def _dev(a, cuda, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(cuda)


def _reference(store, idx, rois, recs, hw):
    """255 * (the fp64 restatement): occlude the full frames of the gathered images, then resample. store
    (n, 3*n_cams, Hs, Ws) uint8 numpy; rois (n_img, 4); recs (n_img, n_arcs, 12) or None -> (n_img, 3, h, w) fp64."""
    n, c, Hs, Ws = store.shape
    frames = store[idx].reshape(len(idx) * (c // 3), 3, Hs, Ws)
    if recs is not None and recs.shape[1] > 0:
        frames = ref.occlude(frames, recs)
    return 255.0 * roi.resample(torch.from_numpy(frames).double() / 255.0, np.asarray(rois, dtype=np.float32).tolist(),
                                hw).numpy()


# ---- 1. identity: unit scale at an integer origin is the cropped store's launch, bit for bit -------------------
@pytest.mark.parametrize("n_cams,batch,n_arcs", [(1, 3, 74), (2, 2, 56), (2, 2, 0)])  # 74: two chunks of records
def test_unit_scale_is_gather_occlude_bitwise(cuda, n_cams, batch, n_arcs):
    from test_gpu_resident import SRC_HW, _arc_pool

    g = torch.Generator().manual_seed(10 * n_cams + n_arcs)
    store = torch.randint(1, 256, (5, 3 * n_cams, *SRC_HW), dtype=torch.uint8, generator=g)
    n_img = batch * n_cams
    recs = None
    if n_arcs:
        pool = resident.arc_records(_arc_pool())
        assert len(pool) <= n_img * n_arcs
        recs = np.zeros((n_img * n_arcs, ref.ARC_WORDS), dtype=np.int32)
        recs[:len(pool)] = pool
        recs = _dev(recs.reshape(n_img, n_arcs, ref.ARC_WORDS), cuda)
    index = torch.tensor([(3 * i + 1) % 5 for i in range(batch)], dtype=torch.int64, device=cuda)
    dstore = store.to(cuda)
    covered = 0
    # the center crop of test_gpu_resident.py, then odd sizes at other origins (the last flush with the far edges)
    for hw, origin in (((40, 56), (5, 8)), ((31, 45), (0, 0)), ((31, 45), (7, 11)), ((31, 45), (19, 27)),
                       ((9, 72), (20, 0))):
        rois = _dev(np.tile(np.float32([*origin, *hw]), (n_img, 1)), cuda)
        got = _launch(dstore, index, rois, recs, n_arcs, hw)
        cropped = dstore[:, :, origin[0]:origin[0] + hw[0], origin[1]:origin[1] + hw[1]].contiguous()
        want = _occlude_launch(cropped, index, recs, n_arcs, origin)
        assert torch.equal(got, want), (hw, origin)
        covered += int((got == 0).sum())
    assert (covered > 0) == (n_arcs > 0)
    assert torch.equal(dstore.cpu(), store)  # the store is read only


# ---- 2. exact cases: zero tolerance -------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,origin", [((24, 136), (4, 6)),    # 3 x 3 tiles, the last column tile 8 wide
                                       ((20, 70), (2, 2)),     # ragged in both axes
                                       ((8, 64), (40, 150)),   # one whole tile
                                       ((11, 9), (36, 260))])  # smaller than a tile; ends at S - 2 in both axes
def test_exact_regions_are_exact(cuda, hw, origin):
    """uint8 frames of {0, 64, 128, 192}, even integer origin >= 2, extent 2n, end <= S - 2: no tap is truncated,
    every weight is 1/8 or 3/8 per axis and the pixel is the integer (Wy v Wx^T) / 64 (255 px is within 1.2e-5 of it
    in fp32: test_resident_roi_host.py)."""
    Hs, Ws = 60, 280
    assert origin[0] % 2 == 0 and origin[1] % 2 == 0 and min(origin) >= 2
    assert origin[0] + 2 * hw[0] <= Hs - 2 and origin[1] + 2 * hw[1] <= Ws - 2
    g = torch.Generator().manual_seed(hw[0])
    store = torch.randint(0, 4, (3, 6, Hs, Ws), generator=g).to(torch.uint8) * 64
    index = torch.tensor([2, 0], dtype=torch.int64, device=cuda)
    rois = np.tile(np.float32([*origin, 2 * hw[0], 2 * hw[1]]), (4, 1))
    got = _launch(store.to(cuda), index, _dev(rois, cuda), None, 0, hw).cpu().numpy()
    wy = 8 * roi.axis_matrix(Hs, hw[0], float(origin[0]), 2.0 * hw[0]).numpy()
    wx = 8 * roi.axis_matrix(Ws, hw[1], float(origin[1]), 2.0 * hw[1]).numpy()
    assert set(np.unique(wy)) == {0.0, 1.0, 3.0} and set(np.unique(wx)) == {0.0, 1.0, 3.0}
    want = wy @ store[[2, 0]].numpy().astype(np.float64) @ wx.T / 64.0
    assert np.array_equal(want, np.rint(want)) and want.max() <= 192
    assert np.array_equal(got.astype(np.float64), want)


# ---- 3. general regions against the fp64 restatement ----------------------------------------------------------------
FRAME, HW = (170, 560), (40, 136)
# (y0, x0, height, width); the two cameras of a sample get different regions
REGIONS = [
    (65.0, 212.0, 40.0, 136.0),     # unit scale: the center crop
    (3.3, 7.7, 51.9, 200.3),        # fractional origin and extents, scales 1.30 and 1.47
    (20.0, 30.0, 16.0, 54.4),       # scale 0.4
    (80.5, 100.25, 10.0, 34.0),     # scale 0.25
    (10.5, 11.25, 40.0, 136.0),     # unit scale at a fractional origin
    (1.5, 2.5, 116.0, 394.4),       # scale 2.9
    (5.0, 8.0, 160.0, 544.0),       # scale 4
    (0.0, 0.0, 60.0, 204.0),        # flush with the top and left edges
    (110.0, 356.0, 60.0, 204.0),    # flush with the bottom and right edges
    (10.0, 0.0, 160.0, 544.0),      # scale 4, flush with the bottom and left edges
]


def _general_arcs(n_img, n_arcs):
    if n_arcs == 0:
        return None
    rng = np.random.RandomState(4)
    p = resident.sample_arcs(rng, n_img, n_arcs, FRAME)
    # the frame's inscribed ellipse without a hole: covers the whole footprint of every tile of image 0 (its region
    # lies at the center: (68 / 280)^2 + (20 / 85)^2 < 1 at its corners)
    p[0, 0] = (0, 0, FRAME[1] - 1, FRAME[0] - 1, 0, 360, 400)
    p[1, 0] = (10, 10, 300, 100, 40, 40, 3)   # a0 == a1: covers nothing
    p[2, 0] = (40, 30, 75, 60, 0, 360, 30)    # a filled disc that overlaps region 2 in part
    return resident.arc_records(p)


@pytest.fixture(scope="module")
def general_case():
    """10 camera images (5 two-camera samples out of a store of 6) without zero bytes, their regions, and the
    reference per arc count, computed once."""
    g = torch.Generator().manual_seed(21)
    store = torch.randint(1, 256, (6, 6, *FRAME), dtype=torch.uint8, generator=g)
    idx = [4, 0, 5, 2, 2]
    rois = np.float32(REGIONS)
    from argus_amd.pose_session import check_roi

    check_roi(torch.from_numpy(rois).reshape(5, 2, 4), FRAME, HW)
    cases = {}
    for n_arcs in (0, 1, 10):
        recs = _general_arcs(10, n_arcs)
        cases[n_arcs] = (recs, _reference(store.numpy(), idx, rois, recs, HW))
    return store, idx, rois, cases


@pytest.mark.parametrize("n_arcs", [0, 1, 10])
def test_general_regions_match_the_fp64_restatement(cuda, general_case, n_arcs):
    store, idx, rois, cases = general_case
    recs, want = cases[n_arcs]
    index = torch.tensor(idx, dtype=torch.int64, device=cuda)
    got = _launch(store.to(cuda), index, _dev(rois, cuda), None if recs is None else _dev(recs, cuda), n_arcs, HW)
    got = got.cpu().numpy().reshape(want.shape).astype(np.float64)
    err = np.abs(got - want)
    print(f"n_arcs {n_arcs}: largest |out - 255 ref| per image", err.reshape(10, -1).max(1).round(4))
    assert err.max() <= BAR  # every pixel
    if n_arcs:
        assert (got[0] == 0).all()  # the arc that covers every footprint
        plain = cases[0][1]
        if n_arcs == 1:
            assert np.array_equal(want[1], plain[1])  # the arc that covers nothing
        assert (np.abs(want - plain) > 1).any(axis=(1, 2, 3)).sum() >= (2 if n_arcs == 1 else 5)
        dimmed = want[2] < plain[2] - 1
        assert dimmed.any() and not dimmed.all()  # covered source pixels weigh in as 0 where the disc reaches


# ---- 4. determinism and hygiene ---------------------------------------------------------------------------------------
def test_arc_order_invalid_records_bad_indices_and_the_store(cuda, general_case):
    store, idx, rois, cases = general_case
    recs, want = cases[10]
    dstore, drois = store.to(cuda), _dev(rois, cuda)
    index = torch.tensor(idx, dtype=torch.int64, device=cuda)
    base = _launch(dstore, index, drois, _dev(recs, cuda), 10, HW)
    perm = np.random.RandomState(0).permutation(10)
    assert torch.equal(_launch(dstore, index, drois, _dev(recs[:, perm], cuda), 10, HW), base)
    bad = np.array([[5, 5, 4, 9, 1, 1, 0, 0, 0, 0, 0, 0], [-1, 5, 9, 9, 1, 1, 0, 0, 0, 0, 0, 0],
                    [0, 0, 9000, 9, 1, 1, 0, 0, 0, 0, 0, 0], [0, 0, 9, 9, 1, 7, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    withbad = np.concatenate([np.broadcast_to(bad[:2], (10, 2, 12)), recs, np.broadcast_to(bad[2:], (10, 2, 12))], 1)
    assert torch.equal(_launch(dstore, index, drois, _dev(withbad, cuda), 14, HW), base)
    # an index outside [0, n_samples) is clamped
    wild = torch.tensor([-3, 99, 2, 1 << 40, -(1 << 40)], dtype=torch.int64, device=cuda)
    tame = torch.tensor([0, 5, 2, 5, 0], dtype=torch.int64, device=cuda)
    assert torch.equal(_launch(dstore, wild, drois, None, 0, HW), _launch(dstore, tame, drois, None, 0, HW))
    # n_samples below the store's: the clamp follows the argument
    assert torch.equal(_launch(dstore, wild, drois, None, 0, HW, n_samples=3),
                       _launch(dstore, torch.tensor([0, 2, 2, 2, 0], device=cuda), drois, None, 0, HW))
    assert torch.equal(dstore.cpu(), store)


# ---- 5. train sees what deploy sees --------------------------------------------------------------------------------------
def test_bytes_are_what_frames_resample_deploys(cuda, general_case):
    """|out / 255 - bf16| <= 0.5 / 255 (uint8 half step) + 2^-9 (bf16 half ulp below 1) + 1e-5 (fp32 slack)."""
    from argus_amd._lib import BF16, FrameSrc, lib, ptr, stream

    store, idx, rois, _ = general_case
    Hs, Ws = FRAME
    dstore, drois = store.to(cuda), _dev(rois, cuda)
    index = torch.tensor(idx, dtype=torch.int64, device=cuda)
    got = _launch(dstore, index, drois, None, 0, HW).view(10, 3, *HW).float() / 255.0
    frames = dstore[index].view(10, 3, Hs, Ws).contiguous()
    x0 = torch.full((10, *HW, 4), float("nan"), dtype=torch.bfloat16, device=cuda)
    src = FrameSrc(ptr(frames), 0, 3 * Hs * Ws, Hs * Ws, Ws, 1, Hs, Ws, 0, 0)
    lib().frames_resample(BF16, 10, HW[0], HW[1], C.byref(src), ptr(drois), ptr(x0), stream())
    torch.cuda.synchronize()
    deployed = x0[..., :3].permute(0, 3, 1, 2).float()
    err = (got - deployed).abs()
    print("largest |out / 255 - bf16|:", err.max().item())
    assert bool(torch.isfinite(deployed).all()) and err.max().item() <= 0.5 / 255 + 2.0 ** -9 + 1e-5


# ---- loader and CLI ---------------------------------------------------------------------------------------------------
CROP = (40, 136)  # of the fixture's 256 x 256 frames: origin (108, 60)


@pytest.fixture(scope="module")
def stores(cuda, dummy_data_path):
    """The fixture's training split twice: the cropped store and the full frames, ten arcs an image."""
    from argus_amd.data import AugmentationConfig, CameraCubePoseDatasetConfig

    cfg = CameraCubePoseDatasetConfig(dataset_path=dummy_data_path, center_crop=CROP)
    aug = AugmentationConfig(num_spaghetti=10)
    cropped = resident.ResidentDataset(cfg, aug, train=True, device=cuda, num_workers=0)
    full = resident.ResidentDataset(cfg, aug, train=True, device=cuda, num_workers=0, full_frames=True)
    return cropped, full


def test_full_frames_without_jitter_equal_the_cropped_loader(cuda, stores):
    cropped, full = stores
    assert tuple(full.images.shape) == (10, 6, 256, 256) and tuple(cropped.images.shape) == (10, 6, *CROP)
    assert full.crop_hw == cropped.crop_hw == CROP and full.crop_origin == cropped.crop_origin == (108, 60)
    assert full.full_frames and not cropped.full_frames and torch.equal(full.poses, cropped.poses)
    assert torch.equal(full.images[:, :, 108:148, 60:196], cropped.images)
    kw = dict(batch_size=4, shuffle=True, seed=9)
    a, b = resident.ResidentLoader(cropped, **kw), resident.ResidentLoader(full, **kw)
    for epoch in (0, 3):
        a.set_epoch(epoch), b.set_epoch(epoch)
        ba, bb = list(a), list(b)
        assert len(ba) == len(bb) == 3
        for x, y in zip(ba, bb):
            assert "roi" not in x and tuple(y["roi"].shape) == (x["images"].shape[0], 2, 4)
            assert y["roi"].dtype == torch.float32 and y["roi"].device.type == "cuda"
            assert torch.equal(y["roi"].cpu(), torch.tensor([108.0, 60.0, 40.0, 136.0]).expand_as(y["roi"]))
            assert torch.equal(x["images"], y["images"]) and torch.equal(x["cube_pose"], y["cube_pose"])
            assert (x["images"] == 0).any()  # arcs included
    with pytest.raises(ValueError, match="full_frames"):
        resident.ResidentLoader(cropped, batch_size=4, roi_jitter=(0.5, 2.0, 0.1))


def test_jittered_loader_matches_sample_rois_and_the_reference(cuda, stores):
    _, full = stores
    jitter = (0.4, 3.0, 0.3)
    loader = resident.ResidentLoader(full, batch_size=5, shuffle=True, seed=9, roi_jitter=jitter, roi_seed=123)
    loader.set_epoch(0)
    e0 = [{k: v.cpu() for k, v in b.items()} for b in loader]
    again = [b["images"].cpu() for b in loader]
    loader.set_epoch(1)
    e1 = [{k: v.cpu() for k, v in b.items()} for b in loader]
    loader.set_epoch(0)
    back = [b["images"].cpu() for b in loader]
    assert all(torch.equal(a["images"], b) for a, b in zip(e0, again))
    assert all(torch.equal(a["images"], b) for a, b in zip(e0, back))       # repeat under set_epoch
    assert not any(torch.equal(a["images"], b["images"]) for a, b in zip(e0, e1))   # epochs differ
    assert not any(torch.equal(a["roi"], b["roi"]) for a, b in zip(e0, e1))
    order = loader.indices()
    arc_rng = np.random.RandomState(9)          # arc_seed + 1000003 * epoch + rank
    roi_rng = np.random.RandomState(123)        # roi_seed + 1000003 * epoch + rank
    store = full.images.cpu().numpy()
    scales = []
    for k, got in enumerate(e0):
        idx = order[5 * k:5 * k + 5]
        rois = resident.sample_rois(roi_rng, 10, full.src_hw, CROP, full.crop_origin, scale=jitter[:2], shift=jitter[2])
        assert torch.equal(got["roi"], torch.from_numpy(rois).view(5, 2, 4))
        recs = resident.arc_records(resident.sample_arcs(arc_rng, 10, 10, full.src_hw))
        want = _reference(store, idx, rois, recs, CROP)
        err = np.abs(got["images"].numpy().reshape(want.shape).astype(np.float64) - want)
        print("batch", k, "largest |out - 255 ref|", err.max())
        assert err.max() <= BAR
        scales += (rois[:, 2] / CROP[0]).tolist()
    assert min(scales) < 0.8 and max(scales) > 1.5  # 256 / 136 = 1.88 caps the scale


def _train_argv(data, save, *extra):
    return ["--dataset-config.dataset-path", data, "--save-dir", str(save), "--batch-size", "5", "--learning-rate", "1e-3",
            "--n-epochs", "2", "--device", "cuda", "--max-grad-norm", "100.0", "--random-seed", "42", "--val-epochs", "1",
            "--print-epochs", "1", "--save-epochs", "1", "--no-compile-model", "--no-wandb-log", "--num-workers", "0",
            "--resident-dataset", *extra]


def test_train_with_roi_jitter_end_to_end_and_reproducible(cuda, dummy_data_path, tmp_path, monkeypatch):
    """``python -m argus_amd.train --resident-dataset --roi-jitter 0.5 2 0.1`` (main()'s two calls, in this
    process): two epochs of two steps, the train split through argus_batch_gather_resample and the validation split
    through the cropped store's launch; reruns are bit-identical. Without the flag no launch is the new one."""
    from argus_amd import _lib
    from argus_amd.train import parse_args, train

    calls = []
    L = _lib.lib()
    for name in ("batch_gather_resample", "batch_gather_occlude"):
        fn = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _fn=fn, _name=name: (calls.append(_name), _fn(*a))[1])

    def run(tag, *extra):
        save = tmp_path / tag
        del calls[:]
        train(parse_args(_train_argv(dummy_data_path, save, *extra)))
        pths = list(save.glob("*.pth"))
        assert len(pths) == 1
        return torch.load(pths[0], weights_only=True), list(calls)

    sd1, c1 = run("a", "--roi-jitter", "0.5", "2", "0.1")
    assert c1.count("batch_gather_resample") == 4 and c1.count("batch_gather_occlude") >= 1  # 2 epochs x 2 steps; val
    assert int(sd1["resnet.bn1.num_batches_tracked"]) == 4
    assert all(bool(torch.isfinite(v).all()) for v in sd1.values() if v.is_floating_point())
    sd2, _ = run("b", "--roi-jitter", "0.5", "2", "0.1")
    assert all(torch.equal(sd1[k], sd2[k]) for k in sd1)  # one seed: bit-identical reruns
    sd3, c3 = run("c")
    assert "batch_gather_resample" not in c3 and c3.count("batch_gather_occlude") >= 4  # the existing path and launch
    assert any(not torch.equal(sd1[k], sd3[k]) for k in sd1)  # the jitter did change what the model saw
