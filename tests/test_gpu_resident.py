"""GPU: the device-resident dataset (argus_amd/resident.py, csrc/resident.hip): the gather, the arc
rasteriser bit for bit against tests/arc_reference.py, the loader against the DataLoader path and
``train(resident_dataset=True)`` end to end."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arc_reference as ref  # noqa: E402

from argus_amd import resident  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _launch(store, index, arcs, n_arcs, crop=(0, 0), n_samples=None):
    """out (B, C, h, w) uint8 of one argus_batch_gather_occlude launch; out is pre-filled with a sentinel."""
    from argus_amd._lib import lib, ptr, stream

    n, c, h, w = store.shape
    out = torch.full((index.numel(), c, h, w), SENTINEL, dtype=torch.uint8, device=store.device)
    lib().batch_gather_occlude(index.numel(), c // 3, h, w, ptr(store), n if n_samples is None else n_samples,
                               ptr(index), ptr(arcs), n_arcs, crop[0], crop[1], ptr(out), stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n_cams", [1, 2, 3])
@pytest.mark.parametrize("hw", [(5, 7), (8, 16), (40, 56), (33, 130)])
def test_gather_only_is_bit_equal(cuda, n_cams, hw):
    g = torch.Generator().manual_seed(n_cams * 1000 + hw[1])
    store = torch.randint(0, 256, (7, 3 * n_cams, *hw), dtype=torch.uint8, generator=g).to(cuda)
    for idx in ([3], [6, 5, 4, 3, 2, 1, 0, 0, 6], [2, 2, 2, 5], [0, 6]):
        index = torch.tensor(idx, dtype=torch.int64, device=cuda)
        out = _launch(store, index, None, 0)
        assert torch.equal(out, store[index]), idx
    # a store that does not start on a 16-byte boundary: rows that cannot move as 16-byte runs still copy
    flat = torch.zeros(store.numel() + 3, dtype=torch.uint8, device=cuda)
    off = flat[3:].view(store.shape)
    off.copy_(store)
    index = torch.tensor([6, 0, 3], dtype=torch.int64, device=cuda)
    assert torch.equal(_launch(off, index, None, 0), store[index])


# ---------------------------------------------------------------------------- arcs, bit for bit
SRC_HW, CROP_HW, CROP_AT = (50, 72), (40, 56), (5, 8)
# (x0, y0, x1, y1, a0, a1, width) in SOURCE coordinates; the crop window is x 8..63, y 5..44
HAND = [
    (20, 12, 44, 30, 0, 360, 2),      # inside the crop, full ellipse
    (20, 12, 44, 30, 40, 40, 3),      # a0 == a1: nothing
    (0, 0, 30, 20, 10, 300, 1),       # straddles the crop's corner
    (50, 30, 71, 49, 200, 100, 4),    # straddles the far corner, span > 180
    (0, 0, 6, 4, 0, 360, 2),          # entirely outside (above / left)
    (64, 0, 71, 49, 0, 360, 1),       # entirely outside (right)
    (0, 45, 71, 49, 0, 360, 1),       # entirely outside (below)
    (30, 8, 30, 40, 45, 200, 2),      # x0 == x1
    (12, 25, 60, 25, 300, 20, 3),     # y0 == y1
    (33, 21, 33, 21, 10, 20, 1),      # one-pixel box
    (8, 5, 8, 5, 0, 360, 4),          # one-pixel box on the crop's first pixel
    (10, 10, 16, 30, 0, 360, 4),      # width >= semi-axis: no hole
    (10, 10, 18, 18, 0, 360, 4),      # width == semi-axis (inner diameter 1)
    (14, 8, 50, 40, 350, 10, 1),      # wrapped span
    (14, 8, 50, 40, 30, 209, 2),      # span just under 180
    (14, 8, 50, 40, 30, 211, 2),      # span just over 180
    (14, 8, 50, 40, 30, 210, 3),      # span exactly 180
    (0, 0, 71, 49, 0, 360, 1),        # the whole frame's ellipse
    (8, 5, 63, 44, 90, 270, 4),       # the crop window's own box
    (22, 11, 23, 12, 0, 360, 1),      # 2 x 2 box
    (40, 20, 45, 22, 100, 80, 2),     # thin box, long wrapped span
]


def _arc_pool():
    sampled = resident.sample_arcs(np.random.RandomState(77), 1, 200, SRC_HW)[0]
    assert {1, 2, 3, 4} <= set(sampled[:, 6].tolist())  # widths 1 to 4 all occur
    return np.concatenate([np.array(HAND, dtype=np.int32), sampled])


@pytest.fixture(scope="module")
def arc_case():
    """A store of 7 two-camera samples without zeros (so a zero is a covered pixel) and the record pool."""
    g = torch.Generator().manual_seed(5)
    store = torch.randint(1, 256, (7, 6, *CROP_HW), dtype=torch.uint8, generator=g)
    return store, resident.arc_records(_arc_pool())


@pytest.mark.parametrize("n_arcs", [1, 10, 33, 70])  # 70: more than the 64 records staged in LDS at a time
def test_arcs_bit_equal_to_the_reference(cuda, arc_case, n_arcs):
    store, pool = arc_case
    n_img = -(-len(pool) // n_arcs)
    n_img += n_img % 2
    recs = np.zeros((n_img * n_arcs, ref.ARC_WORDS), dtype=np.int32)  # the padding: mode 0, covers nothing
    recs[:len(pool)] = pool
    recs = recs.reshape(n_img, n_arcs, ref.ARC_WORDS)
    b = n_img // 2
    idx = [(3 * i + 1) % 7 for i in range(b)]
    index = torch.tensor(idx, dtype=torch.int64, device=cuda)
    out = _launch(store.to(cuda), index, torch.from_numpy(recs).to(cuda), n_arcs, CROP_AT).cpu().numpy()
    gathered = store[idx].numpy().reshape(n_img, 3, *CROP_HW)
    want = ref.occlude(gathered, recs, *CROP_AT)
    assert np.array_equal(out.reshape(want.shape), want)
    covered = want[:, 0] == 0
    assert covered.any() and not covered.all()
    assert np.array_equal(out.reshape(want.shape)[:, :, ~covered.any(0)], gathered[:, :, ~covered.any(0)])
    # the two images of one sample carry different arcs (records are per image, not per sample)
    assert any(not np.array_equal(covered[2 * i], covered[2 * i + 1]) for i in range(b))


def test_arc_order_does_not_matter_and_invalid_records_cover_nothing(cuda, arc_case):
    store, pool = arc_case
    recs = pool[:20].copy()
    bad = np.array([[5, 5, 4, 9, 1, 1, 0, 0, 0, 0, 0, 0], [-1, 5, 9, 9, 1, 1, 0, 0, 0, 0, 0, 0],
                    [0, 0, 9000, 9, 1, 1, 0, 0, 0, 0, 0, 0], [0, 0, 9, 9, 1, 7, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    index = torch.tensor([4], dtype=torch.int64, device=cuda)
    a = np.stack([recs, recs[::-1]])  # camera a: in order; camera b: reversed
    out = _launch(store[:, :6].to(cuda), index, torch.from_numpy(np.ascontiguousarray(a)).to(cuda), 20, CROP_AT)
    m = (out[0].cpu().numpy() == 0)
    assert np.array_equal(m[0], m[3]) and m[0].any()
    withbad = np.stack([np.concatenate([recs, bad]), np.concatenate([bad, recs])])
    out2 = _launch(store.to(cuda), index, torch.from_numpy(np.ascontiguousarray(withbad)).to(cuda), 24, CROP_AT)
    assert torch.equal(out2, out)


def test_bad_index_is_clamped_and_bad_arguments_are_reported(cuda):
    """Documented behaviour (include/argus_hip.h): an index entry outside [0, n_samples) is clamped, bad
    arguments come back through the error channel before anything is launched."""
    from argus_amd._lib import ArgusHipError

    store = torch.randint(0, 256, (7, 6, 8, 16), dtype=torch.uint8).to(cuda)
    index = torch.tensor([-3, 99, 2, 7, -(1 << 40), 1 << 40], dtype=torch.int64, device=cuda)
    out = _launch(store, index, None, 0)
    assert torch.equal(out, store[torch.tensor([0, 6, 2, 6, 0, 6], device=cuda)])
    good = torch.tensor([1], dtype=torch.int64, device=cuda)
    with pytest.raises(ArgusHipError, match="bad arguments"):
        _launch(store, good, None, -1)
    with pytest.raises(ArgusHipError, match="bad arguments"):
        _launch(store, good, None, 2)  # arcs promised, none given
    with pytest.raises(ArgusHipError, match="bad arguments"):
        _launch(store, good, None, 0, n_samples=0)
    with pytest.raises(ArgusHipError, match="8192"):
        _launch(store, good, None, 0, crop=(0, 8190))


# ---------------------------------------------------------------------------- dataset + loader
def _cfgs(path, crop, n_spaghetti):
    from argus_amd.data import AugmentationConfig, CameraCubePoseDatasetConfig

    return (CameraCubePoseDatasetConfig(dataset_path=path, center_crop=crop),
            AugmentationConfig(num_spaghetti=n_spaghetti))


@pytest.fixture(scope="module")
def resident_sets(cuda, dummy_data_path):
    """ResidentDatasets of the fixture's training split, decoded once per crop."""
    out = {}
    for crop in ((256, 256), (128, 128)):
        for k in (0, 10):
            cfg, aug = _cfgs(dummy_data_path, crop, k)
            if k == 0:
                out[crop, k] = resident.ResidentDataset(cfg, aug, train=True, device=cuda, num_workers=0)
            else:  # the same store under another augmentation config
                ds = resident.ResidentDataset.__new__(resident.ResidentDataset)
                ds.__dict__.update(out[crop, 0].__dict__)
                ds.cfg_aug = aug
                out[crop, k] = ds
    return out


@pytest.mark.parametrize("crop", [(256, 256), (128, 128)])
def test_loader_batches_equal_the_dataloader_path(cuda, dummy_data_path, resident_sets, crop):
    from torch.utils.data import DataLoader

    from argus_amd.data import CameraCubePoseDataset

    ds = resident_sets[crop, 0]
    assert ds.src_hw == (256, 256) and ds.crop_hw == crop and ds.n_cams == 2 and len(ds) == 10
    assert ds.crop_origin == ((0, 0) if crop == (256, 256) else (64, 64)) and ds.ingest_seconds > 0
    cfg, aug = _cfgs(dummy_data_path, crop, 0)
    want = list(DataLoader(CameraCubePoseDataset(cfg, aug, train=True, uint8=True, device_augmentation=True),
                           batch_size=4, shuffle=False))
    loader = resident.ResidentLoader(ds, batch_size=4, shuffle=False, seed=0)
    got = list(loader)
    assert len(loader) == len(got) == len(want) == 3 and got[-1]["images"].shape[0] == 2
    for a, b in zip(got, want):
        assert a["images"].dtype == torch.uint8 and a["images"].device.type == "cuda"
        assert a["cube_pose"].dtype == torch.float32 and a["cube_pose"].device.type == "cuda"
        assert torch.equal(a["images"].cpu(), b["images"]) and torch.equal(a["cube_pose"].cpu(), b["cube_pose"])
    # cfg_aug None is the same launch with no arcs
    none = resident.ResidentDataset.__new__(resident.ResidentDataset)
    none.__dict__.update(ds.__dict__)
    none.cfg_aug = None
    first = next(iter(resident.ResidentLoader(none, batch_size=4)))
    assert torch.equal(first["images"].cpu(), want[0]["images"])
    # sharded and shuffled: the rank's DistributedSampler order
    sh = resident.ResidentLoader(ds, batch_size=3, shuffle=True, seed=3, rank=1, world=2)
    sh.set_epoch(2)
    order = resident.epoch_indices(10, 2, True, 3, 1, 2)
    poses = torch.cat([b["cube_pose"] for b in sh])
    assert torch.equal(poses, ds.poses[torch.tensor(order, device=cuda)])


def test_store_limit_is_checked_before_allocating(cuda, dummy_data_path):
    cfg, aug = _cfgs(dummy_data_path, (256, 256), 0)
    with pytest.raises(MemoryError, match="DataLoader"):
        resident.ResidentDataset(cfg, aug, train=True, device=cuda, max_bytes=10 * 6 * 256 * 256 - 1, num_workers=0)


@pytest.mark.parametrize("crop", [(256, 256), (128, 128)])
def test_loader_arcs_are_reproducible_and_match_the_reference(cuda, resident_sets, crop):
    ds = resident_sets[crop, 10]
    loader = resident.ResidentLoader(ds, batch_size=5, shuffle=True, seed=9)
    loader.set_epoch(0)
    e0 = [b["images"].cpu() for b in loader]
    again = [b["images"].cpu() for b in loader]
    loader.set_epoch(1)
    e1 = [b["images"].cpu() for b in loader]
    assert all(torch.equal(a, b) for a, b in zip(e0, again))  # one seed, one epoch: bit-reproducible
    assert not all(torch.equal(a, b) for a, b in zip(e0, e1))  # epochs differ
    # the same records on the CPU reference: the same pixels, so the same share of zeroed pixels per image
    loader.set_epoch(0)
    order = loader.indices()
    rng = np.random.RandomState(9)  # arc_seed + 1000003 * epoch + rank
    store = ds.images.cpu().numpy()
    for k, got in enumerate(e0):
        idx = order[5 * k:5 * k + 5]
        recs = resident.arc_records(resident.sample_arcs(rng, 2 * len(idx), 10, ds.src_hw))
        want = ref.occlude(store[idx].reshape(2 * len(idx), 3, *crop), recs, *ds.crop_origin)
        got = got.numpy().reshape(want.shape)
        share_got, share_want = (got == 0).mean(axis=(1, 2, 3)), (want == 0).mean(axis=(1, 2, 3))
        print("zeroed share per image: kernel", share_got.round(4), "reference", share_want.round(4))
        assert share_want.min() <= share_got.min() and share_got.max() <= share_want.max()
        assert np.array_equal(got, want)
    assert max((g == 0).float().mean().item() for g in e0) > 0.005  # ten arcs do cover something


def test_train_with_resident_dataset_end_to_end_and_reproducible(cuda, dummy_data_path, tmp_path):
    """Mirrors test_train_loop_end_to_end_and_reproducible on the resident path (B = 5, fp32, augmentation on)."""
    from argus_amd.data import CameraCubePoseDatasetConfig
    from argus_amd.models import NCameraCNN, NCameraCNNConfig
    from argus_amd.train import TrainConfig, train

    save = tmp_path / "ckpt"
    cfg = TrainConfig(batch_size=5, learning_rate=1e-3, n_epochs=1, device="cuda", max_grad_norm=100.0,
                      random_seed=42, val_epochs=1, print_epochs=1, save_epochs=1, save_dir=str(save),
                      model_config=NCameraCNNConfig(n_cams=2),
                      dataset_config=CameraCubePoseDatasetConfig(dataset_path=dummy_data_path),
                      compile_model=False, wandb_log=False, num_workers=0, resident_dataset=True)
    train(cfg)
    pths = list(save.glob("*.pth"))
    assert len(pths) == 1
    sd1 = torch.load(pths[0], weights_only=True)
    model = NCameraCNN().to(cuda).eval()
    model.load_state_dict(sd1)
    with torch.no_grad():
        out1 = model(torch.ones(1, 6, 256, 256, device=cuda))
    assert torch.isfinite(out1).all()
    assert int(sd1["resnet.bn1.num_batches_tracked"]) == 2  # 10 samples, B = 5
    for p in pths:
        p.unlink()
    train(cfg)
    sd2 = torch.load(next(save.glob("*.pth")), weights_only=True)
    assert all(torch.equal(sd1[k], sd2[k]) for k in sd1)  # one seed: bit-identical reruns
