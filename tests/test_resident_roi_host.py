"""CPU: the resident loader's random region of interest (argus_amd/resident.py, csrc/resident.hip):
argus_batch_gather_resample declared, bound, exported and refusing every bad call before a launch; sample_rois'
draws, domain and reproducibility; the arc stream unchanged by the jitter; the CLI flag; the exact-arithmetic
construction the GPU test relies on. Nothing here needs a GPU."""
import ctypes as C
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

from argus_amd import resident  # noqa: E402
from argus_amd._lib import LIB_PATH, SIGNATURES, ArgusHipError, lib  # noqa: E402
from argus_amd.pose_session import check_roi  # noqa: E402

NAME = "argus_batch_gather_resample"
ERR_ARG, ERR_SHAPE = 1, 2
STORE, OUT, IDX, ROIS, ARCS = 1 << 40, 1 << 41, 1 << 42, 1 << 43, 1 << 44  # never dereferenced: all calls are refused


# ---- the C ABI --------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported_at_abi_21():
    hdr = (ROOT / "include" / "argus_hip.h").read_text()
    declared = set(re.findall(r"^(?:int|size_t|const char\*)\s+(argus_[a-z0-9_]+)\(", hdr, re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (argus_[a-z0-9_]+)$", out, re.M))
    assert NAME in declared and NAME in SIGNATURES and NAME in exported
    assert lib().dll.argus_abi_version() == 21  # no bump: the symbol is the detection


def _call(**kw):
    a = dict(batch=2, n_cams=2, src_h=40, src_w=48, h=16, w=24, store=STORE, n=3, index=IDX, rois=ROIS, arcs=ARCS,
             n_arcs=1, out=OUT)
    a.update(kw)
    rc = lib().dll.argus_batch_gather_resample(a["batch"], a["n_cams"], a["src_h"], a["src_w"], a["h"], a["w"],
                                               a["store"], a["n"], a["index"], a["rois"], a["arcs"], a["n_arcs"],
                                               a["out"], None)
    return rc, lib().dll.argus_last_error().decode()


@pytest.mark.parametrize("arg", ["store", "index", "rois", "out", "arcs"])
def test_null_pointers_are_refused_by_name(arg):
    rc, msg = _call(**{arg: None})
    assert rc == ERR_ARG and "batch_gather_resample" in msg and arg in msg and "null" in msg


def test_arcs_may_be_null_only_without_arcs():
    # n_arcs == 0 ignores arcs: the next check (here the overlap) is the one that fires
    rc, msg = _call(arcs=None, n_arcs=0, out=STORE)
    assert rc == ERR_ARG and "overlaps" in msg


@pytest.mark.parametrize("kw,name", [(dict(batch=0), "batch"), (dict(batch=-4), "batch"), (dict(n_cams=0), "n_cams"),
                                     (dict(n=0), "n_samples"), (dict(n_arcs=-1), "n_arcs"), (dict(src_h=0), "src_h"),
                                     (dict(src_w=-2), "src_w")])
def test_non_positive_sizes_are_refused_by_name(kw, name):
    rc, msg = _call(**kw)
    assert rc == ERR_ARG and "batch_gather_resample" in msg and name in msg


@pytest.mark.parametrize("kw,word", [(dict(h=7), "at least 8"), (dict(w=7), "at least 8"), (dict(h=0), "at least 8"),
                                     (dict(w=-1), "at least 8"),
                                     (dict(src_h=8193), "8192"), (dict(src_w=8193), "8192"),
                                     (dict(h=41), "h > src_h"), (dict(w=49), "w > src_w")])
def test_shapes_outside_the_served_range_are_refused(kw, word):
    rc, msg = _call(**kw)
    assert rc == ERR_SHAPE and "batch_gather_resample" in msg and word in msg


def test_largest_frame_fits_31_bits():
    """One image's offsets (3 planes of src_h x src_w) fit 31 bits for every frame side the entry point accepts
    (<= 8192), so that refusal cannot be reached alone; the largest served frame passes it and reaches the next
    check (the overlap)."""
    assert 3 * 8192 * 8192 < 1 << 31
    rc, msg = _call(src_h=8192, src_w=8192, out=STORE + 5)
    assert rc == ERR_ARG and "overlaps" in msg


def test_out_overlapping_store_is_refused():
    store_bytes = 3 * 2 * 3 * 40 * 48
    out_bytes = 2 * 2 * 3 * 16 * 24
    for out in (STORE, STORE + store_bytes - 1, STORE - out_bytes + 1):
        rc, msg = _call(out=out)
        assert rc == ERR_ARG and "out overlaps store" in msg, out
    # the wrapper raises with the message
    with pytest.raises(ArgusHipError, match="out overlaps store"):
        lib().batch_gather_resample(2, 2, 40, 48, 16, 24, STORE, 3, IDX, ROIS, ARCS, 1, STORE, None)


# ---- sample_rois --------------------------------------------------------------------------------------------
def _draws_one_by_one(rng, n, frame_hw, hw, origin, scale, shift):
    """The documented draw order, one rng.uniform call per draw, in float64 (before the float32 rounding)."""
    out = []
    for _ in range(n):
        s = math.exp(rng.uniform(math.log(scale[0]), math.log(scale[1])))
        dy = rng.uniform(-shift, shift) * hw[0]
        dx = rng.uniform(-shift, shift) * hw[1]
        s = min(max(s, 0.25), 4.0, frame_hw[0] / hw[0], frame_hw[1] / hw[1])
        eh, ew = min(s * hw[0], frame_hw[0]), min(s * hw[1], frame_hw[1])
        y0 = min(max(origin[0] + hw[0] / 2 + dy - eh / 2, 0.0), frame_hw[0] - eh)
        x0 = min(max(origin[1] + hw[1] / 2 + dx - ew / 2, 0.0), frame_hw[1] - ew)
        out.append((y0, x0, eh, ew))
    return np.array(out)


def test_sample_rois_is_reproducible_and_draws_in_the_stated_order():
    args = ((376, 672), (256, 256), (60, 208))
    a = resident.sample_rois(np.random.RandomState(11), 50, *args, scale=(0.25, 4.0), shift=0.5)
    b = resident.sample_rois(np.random.RandomState(11), 50, *args, scale=(0.25, 4.0), shift=0.5)
    assert a.dtype == np.float32 and a.shape == (50, 4) and np.array_equal(a, b)
    assert not np.array_equal(a, resident.sample_rois(np.random.RandomState(12), 50, *args, scale=(0.25, 4.0), shift=0.5))
    r1, r2 = np.random.RandomState(11), np.random.RandomState(11)
    want = _draws_one_by_one(r1, 50, *args, (0.25, 4.0), 0.5)
    got = resident.sample_rois(r2, 50, *args, scale=(0.25, 4.0), shift=0.5)
    assert np.abs(got - want).max() <= 2.0 ** -14  # float32 rounding of values below 1024 (+ one step of the clip)
    assert r1.uniform() == r2.uniform()  # both generators stand at the same place: 3 draws an image
    # the aspect ratio is the network's, the scale is shared by the axes
    assert np.allclose(a[:, 2] / 256, a[:, 3] / 256, rtol=1e-6)
    s = a[:, 2] / 256
    assert s.min() >= 0.25 and s.max() <= 376 / 256 + 1e-6 and s.min() < 0.5 and s.max() > 1.3
    assert len({tuple(r) for r in a}) == 50


@pytest.mark.parametrize("frame_hw,hw,origin", [((376, 672), (256, 256), (60, 208)),
                                                ((258, 257), (256, 256), (1, 0)),
                                                ((170, 560), (40, 136), (65, 212))])
def test_ten_thousand_draws_pass_check_roi(frame_hw, hw, origin):
    rois = resident.sample_rois(np.random.RandomState(3), 10000, frame_hw, hw, origin, scale=(0.25, 4.0), shift=0.5)
    t = check_roi(torch.from_numpy(rois).reshape(10000, 1, 4), frame_hw, hw)  # raises on any violation
    assert t.dtype == torch.float32 and torch.equal(t.reshape(-1, 4), torch.from_numpy(rois))
    assert (rois[:, :2] >= 0).all()
    if frame_hw == (376, 672):  # the clips do bind: some regions touch the frame's edges
        assert (rois[:, 0] == 0).any() and (rois[:, 0].astype(np.float64) + rois[:, 2] == 376).any()


def test_unit_scale_and_no_shift_is_the_center_crop_exactly():
    from argus_amd.data import center_crop_slices

    for frame_hw, hw in (((376, 672), (256, 256)), ((50, 73), (31, 45)), ((256, 256), (256, 256))):
        ys, xs = center_crop_slices(frame_hw, hw)
        rois = resident.sample_rois(np.random.RandomState(0), 7, frame_hw, hw, (ys.start, xs.start), scale=(1, 1),
                                    shift=0)
        assert np.array_equal(rois, np.tile(np.float32([ys.start, xs.start, hw[0], hw[1]]), (7, 1)))
    assert np.array_equal(resident.sample_rois(np.random.RandomState(0), 3, (64, 64), (32, 32), (16, 16)),
                          np.tile(np.float32([16, 16, 32, 32]), (3, 1)))  # the defaults
    with pytest.raises(ValueError):
        resident.sample_rois(np.random.RandomState(0), 3, (64, 64), (32, 32), (16, 16), scale=(2, 1))
    with pytest.raises(ValueError):
        resident.sample_rois(np.random.RandomState(0), 3, (30, 64), (32, 32), (0, 16))


# ---- loader ---------------------------------------------------------------------------------------------------
class _FakeTensor:
    """What ResidentLoader touches of a device tensor before the first launch."""

    def __init__(self, shape):
        self.shape = shape


def _fake_dataset(full_frames, n_arcs=10):
    from argus_amd.data import AugmentationConfig

    ds = resident.ResidentDataset.__new__(resident.ResidentDataset)
    ds.device = torch.device("cuda", 0)
    ds.cfg_aug = AugmentationConfig(num_spaghetti=n_arcs)
    ds.n_cams, ds.src_hw, ds.crop_hw, ds.crop_origin = 2, (376, 672), (256, 256), (60, 208)
    ds.full_frames = full_frames
    ds.images = _FakeTensor((10, 6, 376, 672) if full_frames else (10, 6, 256, 256))
    return ds


@pytest.fixture
def no_pinning(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self, *a, **k: self)


def test_roi_jitter_on_a_cropped_store_raises(no_pinning):
    with pytest.raises(ValueError, match="full_frames"):
        resident.ResidentLoader(_fake_dataset(False), batch_size=4, roi_jitter=(0.5, 2.0, 0.1))
    for bad in ((0.5, 2.0), (2.0, 0.5, 0.1), (0.0, 1.0, 0.1), (0.5, 2.0, -0.1)):
        with pytest.raises(ValueError, match="roi_jitter"):
            resident.ResidentLoader(_fake_dataset(True), batch_size=4, roi_jitter=bad)
    ok = resident.ResidentLoader(_fake_dataset(True), batch_size=4, roi_jitter=(0.5, 2, 0.1), roi_seed=5)
    assert ok.roi_jitter == (0.5, 2.0, 0.1) and ok.roi_seed == 5 and ok.full_frames
    assert resident.ResidentLoader(_fake_dataset(False), batch_size=4).roi_jitter is None


def test_arc_draws_of_an_epoch_do_not_depend_on_the_jitter(no_pinning):
    """The loader's host side (the words of the pinned slot, batch after batch of one epoch): the arc records are
    the same with the jitter on and off and with a cropped store, because the regions have a generator of their
    own; the regions are the center crop without jitter and sample_rois from the documented seed with it."""
    def epoch_words(ds, **kw):
        loader = resident.ResidentLoader(ds, batch_size=4, shuffle=True, seed=3, rank=1, world=2, **kw)
        loader.set_epoch(2)
        rng, roi_rng = loader.host_generators()
        assert (roi_rng is None) == (loader.roi_jitter is None)
        out = []
        for idx in ([7, 2, 9, 4], [1, 1, 0, 3], [5]):  # the last batch is partial
            hv = np.zeros(len(idx) * (2 + loader._roi_words + 2 * 10 * resident.ARC_WORDS), dtype=np.int32)
            a_at = loader.fill_slot(hv, idx, rng, roi_rng)
            assert np.array_equal(hv[:2 * len(idx)].view(np.int64), idx)
            out.append((hv[2 * len(idx):a_at].view(np.float32).reshape(-1, 4).copy(), hv[a_at:].copy()))
        return out

    crop = epoch_words(_fake_dataset(False))
    full = epoch_words(_fake_dataset(True))
    jit = epoch_words(_fake_dataset(True), roi_jitter=(0.25, 4.0, 0.5), roi_seed=99)
    other = epoch_words(_fake_dataset(True), roi_jitter=(0.5, 2.0, 0.1))
    roi_rng = np.random.RandomState(99 + 1000003 * 2 + 1)  # roi_seed + 1000003 * epoch + rank
    for (r0, a0), (r1, a1), (r2, a2), (r3, a3) in zip(crop, full, jit, other):
        assert a0.size == r1.shape[0] * 10 * resident.ARC_WORDS and a0.any()
        assert np.array_equal(a0, a1) and np.array_equal(a0, a2) and np.array_equal(a0, a3)
        assert r0.size == 0 and np.array_equal(r1, np.tile(np.float32([60, 208, 256, 256]), (len(r1), 1)))
        want = resident.sample_rois(roi_rng, len(r2), (376, 672), (256, 256), (60, 208), scale=(0.25, 4.0), shift=0.5)
        assert np.array_equal(r2, want) and not np.array_equal(r2, r1) and not np.array_equal(r3, r1)
    assert not np.array_equal(crop[0][1], crop[1][1])  # batches differ


def test_no_cpu_fallback(tmp_path):
    from conftest import make_dummy_dataset

    from argus_amd.data import CameraCubePoseDatasetConfig

    cfg = CameraCubePoseDatasetConfig(dataset_path=make_dummy_dataset(tmp_path), center_crop=(128, 128))
    with pytest.raises(RuntimeError, match="HIP"):
        resident.ResidentDataset(cfg, None, train=True, device="cpu", full_frames=True)
    ds = _fake_dataset(True)
    ds.device = torch.device("cpu")
    with pytest.raises(RuntimeError, match="HIP"):
        resident.ResidentLoader(ds, batch_size=4, roi_jitter=(0.5, 2.0, 0.1))


# ---- CLI ------------------------------------------------------------------------------------------------------
def test_roi_jitter_flag_parses_and_needs_the_resident_dataset(tmp_path, capsys):
    from conftest import make_dummy_dataset

    from argus_amd.train import TrainConfig, parse_args

    d = make_dummy_dataset(tmp_path)
    base = ["--dataset-config.dataset-path", d, "--save-dir", str(tmp_path / "m")]
    assert parse_args(base).roi_jitter is None and TrainConfig.__dataclass_fields__["roi_jitter"].default is None
    assert parse_args(base + ["--resident-dataset"]).roi_jitter is None
    cfg = parse_args(base + ["--resident-dataset", "--roi-jitter", "0.5", "2", "0.1"])
    assert cfg.resident_dataset is True and tuple(cfg.roi_jitter) == (0.5, 2, 0.1)
    for argv in (["--roi-jitter", "0.5", "2", "0.1"], ["--no-resident-dataset", "--roi-jitter", "0.5", "2", "0.1"],
                 ["--resident-dataset", "--roi-jitter", "0.5", "2"]):
        with pytest.raises(SystemExit):
            parse_args(base + argv)
        assert "--roi-jitter" in capsys.readouterr().err
    with pytest.raises(ValueError, match="resident"):
        TrainConfig(save_dir=str(tmp_path / "m"), dataset_config=cfg.dataset_config, roi_jitter=(0.5, 2.0, 0.1))


# ---- the exact construction the GPU test relies on ------------------------------------------------------------
def _f32_fma(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64, one rounding of the sum."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def test_exact_regions_give_integers_in_emulated_fp32():
    """Even integer origin >= 2, extent 2n, end <= S - 2: every weight is 1/8 or 3/8 per axis (4 taps, none
    truncated), so the pixel is (Wy v Wx^T) / 64 of bytes; for v in {0, 64, 128, 192} that is an integer, and the
    kernel's fp32 chain (v / 255 first, fmaf chains, 255 * px) lands within 1.2e-5 of it: rintf recovers it."""
    import roi_reference as roi

    S, n, o = 24, 8, 4
    m = roi.axis_matrix(S, n, float(o), 2.0 * n)
    assert set(np.unique(m.numpy())) == {0.0, 0.125, 0.375}
    assert all(int((m[i] > 0).sum()) == 4 for i in range(n))
    m0 = roi.axis_matrix(S, n, 0.0, 2.0 * n)
    assert int((m0[0] > 0).sum()) == 3 and not set(np.unique(m0[0].numpy())) <= {0.0, 0.125, 0.375}  # origin 0 truncates
    w = np.float32([0.125, 0.375, 0.375, 0.125])
    vals = np.float32([0, 64, 128, 192])
    grid = np.stack(np.meshgrid(*([vals] * 4), indexing="ij"), -1).reshape(-1, 4)  # every row of 4 taps
    p = grid / np.float32(255.0)
    rows = np.zeros(len(grid), dtype=np.float32)
    for k in range(4):
        rows = _f32_fma(np.full_like(rows, w[k]), p[:, k], rows)
    worst = 0.0
    ridx = np.random.RandomState(0).randint(0, len(grid), (20000, 4))
    px = np.zeros(20000, dtype=np.float32)
    for k in range(4):
        px = _f32_fma(np.full_like(px, w[k]), rows[ridx[:, k]], px)
    got = (np.float32(255.0) * px).astype(np.float64)
    exact = sum(w[k].astype(np.float64) * (grid[ridx[:, k]].astype(np.float64) @ w.astype(np.float64)) for k in range(4))
    assert np.array_equal(exact, np.rint(exact))  # multiples of 64 / 64
    worst = np.abs(got - exact).max()
    print("largest |255 px - integer| in emulated fp32:", worst)
    assert worst <= 1.2e-5  # against rintf's 0.5
    assert np.array_equal(np.rint(got), exact)
