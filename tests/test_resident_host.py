"""CPU: the host side of the device-resident dataset (argus_amd/resident.py): the arc sampler against
``draw_spaghetti``'s np.random draws, the epoch order against DistributedSampler, the arc definition
(tests/arc_reference.py) against PIL itself, the CLI flag and the no-CPU-fallback errors."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arc_reference as ref  # noqa: E402

from argus_amd import resident  # noqa: E402


def _spaghetti_calls(seed, n_arcs, hw, monkeypatch):
    """The (x0, y0, x1, y1, a0, a1, width) ``draw_spaghetti`` hands to ``ImageDraw.arc`` after np.random.seed."""
    from PIL import Image, ImageDraw

    from argus_amd.utils import draw_spaghetti

    calls = []

    class Recorder:
        def __init__(self, img):
            pass

        def arc(self, box, a0, a1, fill, width):
            calls.append((*box, a0, a1, width))

    monkeypatch.setattr(ImageDraw, "Draw", Recorder)
    np.random.seed(seed)
    draw_spaghetti(Image.new("RGB", hw[::-1]), n_arcs)
    follow = np.random.randint(0, 1 << 30)
    return np.array(calls, dtype=np.int64), follow


@pytest.mark.parametrize("seed,hw", [(0, (376, 672)), (7, (256, 256)), (3, (2, 3)), (11, (1, 1))])
def test_sample_arcs_reproduces_draw_spaghetti(seed, hw, monkeypatch):
    want, follow = _spaghetti_calls(seed, 40, hw, monkeypatch)
    rng = np.random.RandomState(seed)
    got = resident.sample_arcs(rng, 4, 10, hw)  # 4 images of 10 arcs: the same stream, image after image
    assert got.shape == (4, 10, 7) and got.dtype == np.int32
    assert np.array_equal(got.reshape(40, 7), want)
    assert (got[..., 2] >= got[..., 0]).all() and (got[..., 3] >= got[..., 1]).all()
    assert (got[..., 2] < hw[1]).all() and (got[..., 3] < hw[0]).all() and (got[..., 6] >= 1).all()
    assert rng.randint(0, 1 << 30) == follow  # the RandomState goes on where draw_spaghetti's calls leave it
    # the draw-by-draw path (any rng with randint / uniform) is the same stream
    slow = resident._sample_arcs_py(np.random.RandomState(seed), 40, hw, (1.0, 5.0))
    assert np.array_equal(slow, want)


def test_arc_records_match_the_reference_encoding():
    p = resident.sample_arcs(np.random.RandomState(3), 1, 200, (50, 72))[0]
    odd = [(1, 2, 9, 9, 370, 10, 2), (1, 2, 9, 9, 10, 370, 2), (1, 2, 9, 9, -20, 30, 0), (1, 2, 9, 9, 10.5, 10.5, 3),
           (1, 2, 9, 9, 0, 720, 3), (1, 2, 9, 9, 350, 10, 1), (1, 2, 9, 9, 0, 180, 1), (1, 2, 9, 9, 0, 181, 1)]
    for q in [tuple(r) for r in p] + odd:
        rec = resident.arc_records(np.array(q))
        assert rec.dtype == np.int32 and np.array_equal(rec, ref.make_record(*q)), q
    modes = [int(resident.arc_records(np.array(q))[5]) for q in odd]
    assert modes == [0, 1, 2, 0, 1, 2, 2, 3]  # 370 -> 10 is 10 -> 10: nothing, as in PIL
    assert resident.ARC_WORDS == ref.ARC_WORDS and resident.MAX_FRAME == ref.FRAME


@pytest.mark.parametrize("n", [10, 11])
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("drop_last", [False, True])
def test_epoch_indices_equal_distributed_sampler(n, world, shuffle, drop_last):
    from torch.utils.data.distributed import DistributedSampler

    for seed in (0, 5):
        for rank in range(world):
            s = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=shuffle, seed=seed,
                                   drop_last=drop_last)
            for epoch in (0, 1):
                s.set_epoch(epoch)
                assert resident.epoch_indices(n, epoch, shuffle, seed, rank, world, drop_last) == list(s)


# ---------------------------------------------------------------------------- the definition against PIL
def _pil_mask(p, hw):
    from PIL import Image, ImageDraw

    im = Image.new("L", hw[::-1], 255)
    ImageDraw.Draw(im).arc(tuple(int(v) for v in p[:4]), p[4], p[5], fill=0, width=int(p[6]))
    return np.asarray(im) == 0


def _ref_mask(p, hw):
    return ref.arc_mask(ref.make_record(*p), hw[0], hw[1])


def _dilate(m):
    p = np.pad(m, 1)
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


# The shipped definition's distances from PIL 12.2.0 (2,000 arcs drawn as draw_spaghetti draws them on a
# 256 x 256 frame, seed 1234, nothing excluded): area ratio 0.98489, IoU 0.93790, PIL pixels farther than
# one pixel (Chebyshev) from a reference pixel of the same arc 0.651 %, reference pixels farther than one
# pixel from a PIL pixel 0.473 %. (A 20-line centre-sampled float model scored 0.983 / 0.929 / 1.05 % /
# 0.71 %: the definition is closer on all four.) Each bar is the measured distance from perfect loosened
# by a quarter, for PIL versions that rasterise boundary pixels differently.
MEASURED_AREA, MEASURED_IOU, MEASURED_PIL_FAR, MEASURED_REF_FAR = 0.98489, 0.93790, 0.0065118, 0.0047280
BAR_AREA_DEV = 1.25 * (1.0 - MEASURED_AREA)    # |1 - area ratio| <= 0.01889
BAR_IOU = 1.0 - 1.25 * (1.0 - MEASURED_IOU)    # IoU >= 0.92238
BAR_PIL_FAR = 1.25 * MEASURED_PIL_FAR          # <= 0.814 %
BAR_REF_FAR = 1.25 * MEASURED_REF_FAR          # <= 0.591 %


def test_arc_definition_is_close_to_pil():
    import PIL

    hw = (256, 256)
    arcs = resident.sample_arcs(np.random.RandomState(1234), 1, 2000, hw)[0]
    a_pil = a_ref = inter = union = pil_far = ref_far = 0
    for p in arcs:
        a, b = _pil_mask(p, hw), _ref_mask(p, hw)
        a_pil += int(a.sum())
        a_ref += int(b.sum())
        inter += int((a & b).sum())
        union += int((a | b).sum())
        pil_far += int((a & ~_dilate(b)).sum())
        ref_far += int((b & ~_dilate(a)).sum())
    area, iou = a_ref / a_pil, inter / union
    print(f"PIL {PIL.__version__}: area ratio {area:.5f} IoU {iou:.5f} PIL-far {pil_far / a_pil:.5%} "
          f"ref-far {ref_far / a_ref:.5%} over {a_pil} PIL pixels")
    assert abs(1.0 - area) <= BAR_AREA_DEV
    assert iou >= BAR_IOU
    assert pil_far / a_pil <= BAR_PIL_FAR
    assert ref_far / a_ref <= BAR_REF_FAR


DEGENERATE = [(3, 3, 3, 10), (3, 3, 10, 3), (5, 5, 5, 5), (4, 4, 4, 24), (4, 4, 24, 4), (0, 0, 0, 29), (0, 0, 29, 0)]


@pytest.mark.parametrize("box", DEGENERATE)
def test_degenerate_boxes_follow_pil(box):
    """x0 == x1, y0 == y1 and one-pixel boxes: PIL draws the line (or pixel) over the range of the ellipse
    parameter the angles sweep, whatever the width, and the definition follows it: exactly on vertical
    lines and one-pixel boxes (3,000 random ones agreed with PIL 12.2.0), and on horizontal lines up to the
    pixel next to the centre of a short line (76 of 3,000 random ones differed there, by that one pixel)."""
    hw = (30, 30)
    for a0, a1 in [(0, 360), (0, 180), (90, 270), (45, 135), (300, 20), (100, 200), (10, 20), (200, 100), (33, 33)]:
        for wd in (1, 2, 5):
            p = (*box, a0, a1, wd)
            assert np.array_equal(_pil_mask(p, hw), _ref_mask(p, hw)), p


@pytest.mark.parametrize("box,wd", [((2, 2, 20, 14), 3), ((4, 4, 24, 44), 1), ((3, 3, 6, 6), 2), ((3, 3, 3, 10), 1),
                                    ((5, 6, 40, 40), 30)])
def test_angle_facts_hold_for_pil_and_the_definition(box, wd):
    hw = (50, 50)
    for mask in (_pil_mask, _ref_mask):
        m = lambda a0, a1: mask((*box, a0, a1, wd), hw)  # noqa: E731
        assert not m(40, 40).any() and not m(0, 0).any()             # a0 == a1 draws nothing
        full = m(0, 360)
        assert full.any()
        assert np.array_equal(m(0, 400), full) and np.array_equal(m(-30, 700), full)  # span >= 360 == span 360
        assert np.array_equal(m(350, 10), m(350, 360) | m(0, 10))    # a wrapped arc == the union of its halves
    # widths: no hole once the stroke reaches a semi-axis; a width below 1 draws as 1
    assert np.array_equal(_ref_mask((*box, 0, 360, 0), hw), _ref_mask((*box, 0, 360, 1), hw))


def test_reference_window_is_a_crop_of_the_frame():
    """Arcs live in source-frame coordinates: the mask of a crop window is the crop of the frame's mask."""
    arcs = resident.sample_arcs(np.random.RandomState(5), 1, 50, (50, 72))[0]
    for p in arcs:
        rec = ref.make_record(*p)
        assert np.array_equal(ref.arc_mask(rec, 40, 56, 5, 8), ref.arc_mask(rec, 50, 72)[5:45, 8:64])


# ---------------------------------------------------------------------------- CLI and errors
def test_resident_dataset_flag_parses(tmp_path):
    from conftest import make_dummy_dataset

    from argus_amd.train import TrainConfig, parse_args

    d = make_dummy_dataset(tmp_path)
    base = ["--dataset-config.dataset-path", d, "--save-dir", str(tmp_path / "m")]
    assert parse_args(base).resident_dataset is False
    assert parse_args(base + ["--resident-dataset"]).resident_dataset is True
    assert parse_args(base + ["--no-resident-dataset"]).resident_dataset is False
    assert TrainConfig.__dataclass_fields__["resident_dataset"].default is False


def test_no_cpu_fallback(tmp_path):
    from conftest import make_dummy_dataset

    from argus_amd.data import CameraCubePoseDatasetConfig

    cfg = CameraCubePoseDatasetConfig(dataset_path=make_dummy_dataset(tmp_path))
    with pytest.raises(RuntimeError, match="HIP"):
        resident.ResidentDataset(cfg, None, train=True, device="cpu")
    ds = resident.ResidentDataset.__new__(resident.ResidentDataset)  # a dataset that claims a CPU device
    ds.device = torch.device("cpu")
    with pytest.raises(RuntimeError, match="HIP"):
        resident.ResidentLoader(ds, batch_size=4)
    with pytest.raises(TypeError):
        resident.ResidentLoader(object(), batch_size=4)


def test_exports_are_bound_and_reject_bad_arguments():
    from argus_amd._lib import SIGNATURES, ArgusHipError, lib

    header = (Path(__file__).resolve().parents[1] / "include" / "argus_hip.h").read_text()
    for name in ("argus_batch_gather_occlude", "argus_arc_record_bytes", "argus_sample_arc_params"):
        assert name in SIGNATURES and name + "(" in header
    L = lib()
    assert L.dll.argus_arc_record_bytes() == 4 * resident.ARC_WORDS
    ok = dict(batch=2, n_cams=2, h=8, w=8, store=16, n=3, index=16, arcs=16, n_arcs=1, y0=0, x0=0, out=16)
    for bad in (dict(n_arcs=-1), dict(store=None), dict(out=None), dict(index=None), dict(batch=0), dict(n_cams=0),
                dict(h=0), dict(w=0), dict(n=0), dict(arcs=None), dict(y0=-1), dict(x0=8190), dict(h=8193)):
        a = {**ok, **bad}
        with pytest.raises(ArgusHipError, match="batch_gather_occlude"):  # rejected before anything is launched
            L.batch_gather_occlude(a["batch"], a["n_cams"], a["h"], a["w"], a["store"], a["n"], a["index"], a["arcs"],
                                   a["n_arcs"], a["y0"], a["x0"], a["out"], None)
