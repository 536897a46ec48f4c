"""GPU: the region of interest of the pose session: argus_frames_resample and argus_stem_infer_roi against the fp64
restatement of the antialiased triangle filter (roi_reference.py), against argus_stem_infer on the crop and on the
resampled pixels, and PoseSession(roi=True) end to end. Weights, coefficients, the NaN prefill with its guard and
the stem bars are test_gpu_stem_infer.py's.

Pixel bars: a resampled pixel is a convex combination of values in [0, 1] summed in fp32 (at most 81 terms, error
far below 2^-17), then rounded once to T: at most 1 ulp of T from T(reference), and different at all only where the
reference lies within that fp32 error of a rounding boundary of T: at most 1 % of the pixels."""
import ctypes as C

import pytest
import torch

from argus_amd._lib import FrameSrc, lib, ptr, stream
from test_gpu_infer import _randomize_bn
from test_gpu_stem_infer import DT, GUARD, TDT, TOL, _coeffs, _pooled, _reference, _run, _weights
from tests.roi_reference import exact_case, resample

pytestmark = pytest.mark.gpu

DTS = ["bf16", "fp16"]


def _src(t, layout, Hs, Ws):
    """The whole (n, 3, Hs, Ws) ("chw") or (n, Hs, Ws, 3) ("hwc") tensor ``t``: the region holds the origin."""
    st = (3 * Hs * Ws, Hs * Ws, Ws, 1) if layout == "chw" else (3 * Hs * Ws, 1, 3 * Ws, 3)
    return FrameSrc(ptr(t), 0 if t.dtype == torch.uint8 else 1, *st, Hs, Ws, 0, 0)


def _frames(gen, n, fhw, kind):
    """(device tensor in its layout, the (n, 3, Hs, Ws) fp64 pixels the network sees, layout)."""
    u8 = torch.randint(0, 256, (n, 3, *fhw), generator=gen, dtype=torch.uint8)
    layout, dtype = kind.split()
    host = u8 if layout == "chw" else u8.permute(0, 2, 3, 1).contiguous()
    if dtype == "f32":
        host = host.float() / 255.0
    return host, (u8.float() / 255.0).double(), layout


def _rois(rois, cuda):
    """The regions as the device reads them; ``.tolist()`` gives the reference the same fp32 values."""
    return torch.tensor(rois, dtype=torch.float32).to(cuda)


def _resample(cuda, dt, n, H, W, src, rois):
    """One argus_frames_resample launch into a NaN-prefilled buffer with a guard: ((n, H, W, 4) output, buffer)."""
    numel = n * H * W * 4
    buf = torch.full((numel + GUARD,), float("nan"), dtype=TDT[dt], device=cuda)
    lib().frames_resample(DT[dt], n, H, W, C.byref(src), ptr(rois), ptr(buf), stream())
    return buf[:numel].view(n, H, W, 4), buf


def _stem_roi(cuda, dt, n, H, W, src, rois, wf, scale, shift):
    H2, W2 = _pooled(H)[1], _pooled(W)[1]
    numel = n * H2 * W2 * 64
    buf = torch.full((numel + GUARD,), float("nan"), dtype=TDT[dt], device=cuda)
    lib().stem_infer_roi(DT[dt], n, H, W, 64, C.byref(src), ptr(rois), ptr(wf), ptr(scale), ptr(shift), ptr(buf),
                         stream())
    return buf[:numel].view(n, H2, W2, 64), buf


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- 1. unit scale at an integer origin is argus_stem_infer's crop, bit for bit ---------------------------
@pytest.mark.parametrize("dt", DTS)
def test_unit_scale_roi_is_the_crop_bitwise(cuda, dt):
    n, Hs, Ws, H, W = 2, 41, 77, 30, 46
    gen = torch.Generator().manual_seed(77)
    wf, _ = _weights(cuda, dt, gen)
    scale, shift = _coeffs(gen)
    sc, sh = scale.to(cuda), shift.to(cuda)
    rois = _rois([(5, 15, H, W)] * n, cuda)
    first = None
    for kind in ("chw u8", "chw f32", "hwc u8", "hwc f32"):
        host, _, layout = _frames(torch.Generator().manual_seed(5), n, (Hs, Ws), kind)
        t = host.to(cuda)
        src = _src(t, layout, Hs, Ws)
        crop = FrameSrc(*[getattr(src, f) for f, _ in FrameSrc._fields_[:8]], 5, 15)
        want, _ = _run(cuda, dt, n, H, W, crop, wf, sc, sh)
        got, buf = _stem_roi(cuda, dt, n, H, W, src, rois, wf, sc, sh)
        assert bool(torch.isfinite(got).all()) and bool(torch.isnan(buf[got.numel():]).all()), kind
        assert torch.equal(_bits(got), _bits(want)), kind
        first = got if first is None else first
        assert torch.equal(_bits(got), _bits(first)), kind  # one set of pixel values, one output


# ---- 2. exact arithmetic: the resampled pixels ARE the fp64 reference -------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n,H,W", [(2, 16, 16), (2, 30, 46), (3, 72, 104), (2, 24, 124)], ids=str)
def test_exact_case_equals_the_fp64_reference(cuda, dt, n, H, W):
    origin = (6, 4)
    fhw = (2 * H + origin[0] + 3, 2 * W + origin[1] + 5)
    frames, rois = exact_case(n, fhw, (H, W), origin, seed=H + W)
    ref = resample(frames, rois, (H, W)).permute(0, 2, 3, 1)  # (n, H, W, 3) fp64, exact in T
    t = frames.to(cuda)
    out, buf = _resample(cuda, dt, n, H, W, _src(t, "chw", *fhw), _rois(rois, cuda))
    assert bool(torch.isnan(buf[out.numel():]).all())
    assert torch.equal(out[..., :3].double().cpu(), ref)
    assert bool((out[..., 3] == 0).all())


# ---- 3. resample parity ------------------------------------------------------------------------------------
PARITY = [
    # frame, output, per-image regions, the frames' layout and dtype
    ((41, 77), (30, 46), [(2.25, 3.5, 37.5, 70.0)] * 2, "hwc u8"),
    ((96, 130), (30, 46), [(1.0, 2.0, 86.1, 124.2)] * 2, "chw f32"),       # about 2.87x
    ((40, 52), (64, 64), [(3.3, 4.7, 17.0, 19.0)] * 2, "hwc f32"),         # about 0.27x: upsampling
    ((96, 130), (24, 124), [(0.0, 0.0, 96.0, 130.0)] * 2, "chw u8"),       # the whole frame; 4x in y: 9 taps
    ((40, 52), (16, 16), [(1.5, 2.5, 33.3, 40.1)] * 2, "hwc u8"),
    ((100, 140), (72, 104), [(0.0, 0.0, 100.0, 140.0), (10.5, 20.25, 60.0, 99.5), (3.0, 7.0, 72.0, 104.0)], "hwc u8"),
]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("fhw,hw,rois,kind", PARITY, ids=[f"{c[0]}->{c[1]}x{len(c[2])}" for c in PARITY])
def test_resample_is_within_one_ulp_of_the_reference(cuda, dt, fhw, hw, rois, kind):
    n, (H, W) = len(rois), hw
    host, pix64, layout = _frames(torch.Generator().manual_seed(fhw[0] + 3 * hw[1]), n, fhw, kind)
    r = _rois(rois, cuda)
    ref = resample(pix64, r.tolist(), hw).permute(0, 2, 3, 1).to(TDT[dt])  # T(reference), (n, H, W, 3)
    t = host.to(cuda)
    out, buf = _resample(cuda, dt, n, H, W, _src(t, layout, *fhw), r)
    assert bool(torch.isnan(buf[out.numel():]).all())  # nothing beyond the tensor
    assert bool((out[..., 3] == 0).all())              # the pad channel
    got = out[..., :3].cpu()
    assert bool(torch.isfinite(got).all())
    ulps = (_bits(got).int() - _bits(ref).int()).abs()  # values in [0, 1]: the bit patterns are ordered
    differ = (ulps > 0).float().mean().item()
    print(f"resample {dt} {fhw}->{hw} x{n} {kind}: max {int(ulps.max())} ulp, {100 * differ:.4f} % differ")
    assert int(ulps.max()) <= 1
    assert differ <= 0.01


# ---- 4. fused = unfused pixels ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("fhw,hw,rois,kind", [PARITY[0], PARITY[3], PARITY[5]], ids=["30x46", "24x124", "72x104x3"])
def test_stem_infer_roi_is_stem_infer_on_the_resampled_pixels(cuda, dt, fhw, hw, rois, kind):
    n, (H, W) = len(rois), hw
    gen = torch.Generator().manual_seed(31 * H + W + n)
    host, pix64, layout = _frames(gen, n, fhw, kind)
    wf, w64 = _weights(cuda, dt, gen)
    scale, shift = _coeffs(gen)
    sc, sh = scale.to(cuda), shift.to(cuda)
    t, r = host.to(cuda), _rois(rois, cuda)
    src = _src(t, layout, *fhw)
    x0, _ = _resample(cuda, dt, n, H, W, src, r)
    up = x0.float().contiguous()  # NHWC4 fp32: T(fp32(x)) = x
    nhwc4 = FrameSrc(ptr(up), 1, H * W * 4, 1, 4 * W, 4, H, W, 0, 0)
    want, _ = _run(cuda, dt, n, H, W, nhwc4, wf, sc, sh)
    got, buf = _stem_roi(cuda, dt, n, H, W, src, r, wf, sc, sh)
    assert bool(torch.isfinite(got).all()) and bool(torch.isnan(buf[got.numel():]).all())
    assert torch.equal(_bits(got), _bits(want))
    again, _ = _stem_roi(cuda, dt, n, H, W, src, r, wf, sc, sh)
    assert torch.equal(_bits(got), _bits(again))  # bit-reproducible
    ref = _reference(resample(pix64, r.tolist(), hw).to(TDT[dt]).double(), w64, scale, shift)
    err = (got.double().cpu() - ref).abs().max().item()
    bound = TOL[dt] * ref.abs().max().item()
    print(f"stem_infer_roi {dt} {fhw}->{hw} x{n}: max error / bound = {err / bound:.3f}")
    assert bool((ref > 0).any()) and err <= bound


# ---- 5. the session ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(cuda):
    from argus_amd.models import NCameraCNN

    torch.manual_seed(11)
    out = {}
    for dt, model_dt in (("bf16", "bf16"), ("fp16", "fp32")):
        m = NCameraCNN(compute_dtype=model_dt)
        _randomize_bn(m)
        out[dt] = m.to(cuda).eval()
    return out


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("batch", [1, 2])
def test_session_roi(cuda, models, dt, batch):
    from argus_amd.pose_session import PoseSession

    hw, fhw, model = (64, 64), (100, 130), models[dt]
    n = 2 * batch
    g = torch.Generator().manual_seed(batch)
    frames = torch.randint(0, 256, (batch, 2, *fhw, 3), generator=g, dtype=torch.uint8).to(cuda)
    kw = dict(compute_dtype=dt, frame_hw=fhw, layout="hwc")
    s = PoseSession(model, batch, hw, roi=True, **kw)
    plain = PoseSession(model, batch, hw, **kw)
    assert s.launches_per_forward == plain.launches_per_forward == 55
    # left at its default: the center crop at unit scale, the bits of roi=False
    assert s.roi.tolist() == [[[18.0, 33.0, 64.0, 64.0]] * 2] * batch and plain.roi is None
    assert torch.equal(s.pose(frames), plain.pose(frames)) and torch.equal(s.pred, plain.pred)
    assert torch.equal(s(frames), plain(frames))

    # a region per image: a plain session on the frames argus_frames_resample makes of them
    ra = torch.tensor([[2.5, 3.25, 90.0, 120.5], [20.0, 31.0, 64.0, 64.0], [0.0, 0.0, 100.0, 130.0],
                       [30.5, 40.5, 40.0, 33.3]])[:n].view(batch, 2, 4)
    rb = torch.tensor([7.0, 9.5, 80.0, 111.0])
    pre = PoseSession(model, batch, hw, compute_dtype=dt)
    src = _src(frames, "hwc", *fhw)

    def resampled(roi):
        r = roi.expand(batch, 2, 4).reshape(n, 4).contiguous().to(cuda)
        x0, _ = _resample(cuda, dt, n, *hw, src, r)
        return x0[..., :3].float().permute(0, 3, 1, 2).reshape(batch, 6, *hw).contiguous()

    pa = s.pose(frames, roi=ra)
    assert torch.equal(s.roi, ra) and torch.equal(pa, pre.pose(resampled(ra))) and torch.equal(s.pred, pre.pred)
    ya = s.pred.clone()
    pb = s.pose(frames, roi=rb)
    assert torch.equal(s.roi, rb.expand(batch, 2, 4)) and torch.equal(pb, pre.pose(resampled(rb)))
    assert not torch.equal(pa, pb)
    # alternated over four replays: the graph follows the buffer, nothing is captured again
    outs = [s.pose(frames, roi=r) for r in (ra, rb, ra, rb)]
    assert torch.equal(outs[0], pa) and torch.equal(outs[2], pa) and torch.equal(outs[1], pb) and torch.equal(outs[3], pb)
    assert len(s._graphs) == 1
    s.set_roi(ra)
    assert torch.equal(s(None), ya) and torch.equal(s.pose(None), pa)  # replays on the static frames and regions

    eager = PoseSession(model, batch, hw, roi=True, graph=False, **kw)
    assert torch.equal(eager.pose(frames, roi=ra), pa) and torch.equal(eager.pose(frames, roi=rb), pb)
    assert torch.equal(eager(frames, roi=ra), ya)

    # fused_stem=False: argus_frames_resample in place of the NHWC4 copy, then the parent's stem launches
    un = PoseSession(model, batch, hw, roi=True, fused_stem=False, **kw)
    un_pre = PoseSession(model, batch, hw, compute_dtype=dt, fused_stem=False)
    assert un.launches_per_forward == un_pre.launches_per_forward == 57
    assert torch.equal(un.pose(frames, roi=ra), un_pre.pose(resampled(ra))) and torch.equal(un.pred, un_pre.pred)

    # refusals leave the device buffer as it was
    for bad, rule in (((0, 0, 101, 64), "inside the frame"), ((0, 0, 15, 64), "scale"),
                      (torch.cat([ra, ra]), "shape")):
        with pytest.raises(ValueError, match="roi " + rule):
            s.pose(frames, roi=bad)
    assert torch.equal(s.roi, ra)
    with pytest.raises(ValueError, match="roi=True"):
        plain.pose(frames, roi=rb)
