"""CPU: the region of interest of the pose session. The fp64 restatement (roi_reference.py) against torch's
antialiased interpolate and against the crop; the exact-arithmetic construction the GPU test relies on; check_roi's
domain; argus_frames_resample / argus_stem_infer_roi declared, bound, exported and refusing every bad call before
anything touches a device; the timing CLI's --roi."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from argus_amd._lib import BF16, F16, F32, FP8, LIB_PATH, SIGNATURES, FrameSrc, lib
from tests.roi_reference import axis_matrix, exact_case, resample

ROOT = Path(__file__).resolve().parents[1]
NEW = ["argus_frames_resample", "argus_stem_infer_roi"]
P = C.c_void_p(4096)  # a non-null pointer no refused call may dereference
ERR_ARG = 1


def _err():
    return lib().dll.argus_last_error().decode()


# ---- the definition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [((47, 61), (24, 31)), ((33, 45), (50, 64)), ((96, 130), (48, 65)),
                                     ((40, 52), (40, 52)), ((37, 90), (30, 23))], ids=str)
def test_whole_frame_roi_is_torch_antialiased_interpolate(src, dst):
    g = torch.Generator().manual_seed(src[0] * dst[1])
    x = torch.rand(2, 3, *src, generator=g, dtype=torch.float64)
    want = F.interpolate(x, size=dst, mode="bilinear", antialias=True, align_corners=False)
    got = resample(x, [(0.0, 0.0, float(src[0]), float(src[1]))] * 2, dst)
    assert (got - want).abs().max().item() <= 1e-12


def test_unit_scale_at_an_integer_origin_is_the_crop():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 41, 77, generator=g, dtype=torch.float64)
    got = resample(x, [(5.0, 15.0, 30.0, 46.0), (0.0, 31.0, 30.0, 46.0)], (30, 46))
    assert torch.equal(got[0], x[0, :, 5:35, 15:61]) and torch.equal(got[1], x[1, :, 0:30, 31:77])


def test_scale_two_at_an_even_origin_has_taps_1_3_3_1_over_8():
    m = axis_matrix(40, 16, 4.0, 32.0)
    for i in range(16):
        want = torch.zeros(40, dtype=torch.float64)
        want[4 + 2 * i - 1:4 + 2 * i + 3] = torch.tensor([1, 3, 3, 1], dtype=torch.float64) / 8
        assert torch.equal(m[i], want), i


@pytest.mark.parametrize("tdt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_exact_case_is_exact_in_both_formats(tdt):
    frames, rois = exact_case(3, (70, 100), (30, 46), (6, 4))
    ref = resample(frames, rois, (30, 46))
    assert torch.equal(ref * 64, (ref * 64).round()) and 0 <= ref.min() and ref.max() < 4
    assert ref.unique().numel() > 100  # not a constant image
    assert torch.equal(ref.to(tdt).double(), ref) and torch.equal(ref.float().double(), ref)


# ---- check_roi --------------------------------------------------------------------------------------------
def test_check_roi_accepts_the_corners_of_the_domain():
    from argus_amd.pose_session import check_roi

    fhw, hw = (300, 400), (64, 96)
    for roi in [(0, 0, 256, 384), (0, 0, 16, 24), (44, 16, 256, 384), (284, 376, 16, 24), (0.5, 0.25, 255.5, 100.75),
                (118, 152, 64, 96)]:
        t = check_roi(roi, fhw, hw)
        assert t.dtype == torch.float32 and t.device.type == "cpu" and t.tolist() == [float(v) for v in roi]
    per_image = torch.tensor([[[0, 0, 256, 384], [0, 0, 16, 24]]] * 2, dtype=torch.float64)
    assert tuple(check_roi(per_image, fhw, hw).shape) == (2, 2, 4)


@pytest.mark.parametrize("roi,rule", [
    ((-0.01, 0, 64, 96), "origin"), ((0, -1, 64, 96), "origin"),
    ((236.01, 0, 64, 96), "inside the frame"), ((0, 304.01, 64, 96), "inside the frame"),
    ((0, 0, 15.99, 96), "scale"), ((0, 0, 256.01, 96), "scale"), ((0, 0, 64, 23.99), "scale"),
    ((0, 0, 64, 384.01), "scale"),
    ((0, 0, float("nan"), 96), "finite"), ((float("inf"), 0, 64, 96), "finite"),
    ((0, 0, 64), "shape"), ([[0, 0, 64, 96]], "shape"), ([[[0, 0, 64]]], "shape")], ids=str)
def test_check_roi_names_the_violated_rule(roi, rule):
    from argus_amd.pose_session import check_roi

    with pytest.raises(ValueError, match="roi " + rule):
        check_roi(roi, (300, 400), (64, 96))


# ---- the C ABI --------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported_at_abi_21():
    hdr = (ROOT / "include" / "argus_hip.h").read_text()
    declared = set(re.findall(r"^(?:int|size_t|const char\*)\s+(argus_[a-z0-9_]+)\(", hdr, re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (argus_[a-z0-9_]+)$", out, re.M))
    for name in NEW:
        assert name in declared and name in SIGNATURES and name in exported, name
    assert lib().dll.argus_abi_version() == 21  # no bump: the symbol is the detection


def _src(**kw):
    # 2 planar images of 3 x 40 x 48
    f = dict(base=4096, in_dtype=0, stride_img=3 * 40 * 48, stride_c=40 * 48, stride_y=48, stride_x=1, src_h=40,
             src_w=48, y0=0, x0=0)
    f.update(kw)
    return FrameSrc(*(f[k] for k, _ in FrameSrc._fields_))


def _resample(dtype=BF16, n=2, h=32, w=40, src=None, rois=P, x0=P):
    s = _src() if src is None else src
    return lib().dll.argus_frames_resample(dtype, n, h, w, C.byref(s) if s is not False else None, rois, x0, None)


def _stem(dtype=BF16, n=2, h=32, w=40, k=64, src=None, rois=P, ptrs=(P, P, P, P)):
    s = _src() if src is None else src
    return lib().dll.argus_stem_infer_roi(dtype, n, h, w, k, C.byref(s) if s is not False else None, rois, *ptrs, None)


CALLS = [_resample, _stem]


@pytest.mark.parametrize("call", CALLS, ids=NEW)
@pytest.mark.parametrize("dtype", [F32, FP8, 99])
def test_entry_points_refuse_other_dtypes(call, dtype):
    assert call(dtype=dtype) == ERR_ARG and "dtype" in _err()


@pytest.mark.parametrize("call", CALLS, ids=NEW)
def test_entry_points_refuse_bad_geometry_and_nulls(call):
    assert call(src=False) == ERR_ARG and "null" in _err()
    assert call(src=_src(base=None)) == ERR_ARG and "null" in _err()
    assert call(rois=None) == ERR_ARG and "null" in _err()
    for in_dtype in (2, -1):
        assert call(src=_src(in_dtype=in_dtype)) == ERR_ARG and "in_dtype" in _err()
    for kw in (dict(n=0), dict(h=7), dict(w=7)):
        assert call(**kw) == ERR_ARG, kw
    for kw in (dict(src_h=0), dict(src_w=-3), dict(y0=4), dict(x0=4)):  # the region holds the origin
        assert call(src=_src(**kw)) == ERR_ARG and "y0 = x0 = 0" in _err(), kw
    # offsets over the whole frame must fit the kernels' 32-bit index; negative strides are not served
    assert call(src=_src(stride_y=1 << 27)) == ERR_ARG and "31 bits" in _err()
    assert call(src=_src(stride_c=1 << 30)) == ERR_ARG and "31 bits" in _err()
    for name in ("stride_img", "stride_c", "stride_y", "stride_x"):
        assert call(src=_src(**{name: -1})) == ERR_ARG and "strides" in _err(), name
    assert call(dtype=F16, rois=None) == ERR_ARG and "null" in _err()  # fp16 is served: the next check fires


def test_each_output_and_operand_pointer_is_checked():
    assert _resample(x0=None) == ERR_ARG and "null" in _err()
    for i in range(4):
        ptrs = [P] * 4
        ptrs[i] = None
        assert _stem(ptrs=ptrs) == ERR_ARG and "null" in _err()
    assert _stem(k=128) == ERR_ARG and "k == 64" in _err()


# ---- Python -----------------------------------------------------------------------------------------------
def test_timing_cli_parses_roi(monkeypatch, capsys):
    """main() with pose_latency replaced: what the command line hands to the measurement."""
    from argus_amd import timing

    seen = []

    def fake(*args, **kw):
        seen.append((args, kw))
        return {"mean_s": 0.0}

    monkeypatch.setattr(timing, "pose_latency", fake)
    timing.main(["--frozen", "--pose", "--frame-hw", "720", "1280", "--layout", "hwc", "--roi", "10.5", "20", "480.25",
                 "640"])
    timing.main(["--frozen", "--pose"])
    (args, kw), (_, kw_plain) = seen
    assert kw["roi"] == [10.5, 20.0, 480.25, 640.0] and (1280 in args[6]) and "hwc" in args
    assert kw_plain["roi"] is None
    for bad in (["--roi", "1", "2", "3"], ["--roi", "1", "2", "3", "x"], ["--roi", "1", "2", "3", "4", "--parent"]):
        with pytest.raises(SystemExit):
            timing.main(["--frozen", "--pose", *bad])
    assert len(seen) == 2 and "--roi" in capsys.readouterr().err


def test_roi_session_has_no_cpu_fallback():
    from argus_amd.models import NCameraCNN
    from argus_amd.pose_session import PoseSession

    with pytest.raises(RuntimeError, match="HIP"):
        PoseSession(NCameraCNN(), 1, (64, 64), compute_dtype="bf16", frame_hw=(100, 130), roi=True)
