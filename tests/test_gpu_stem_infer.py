"""GPU: argus_stem_infer (frames -> conv1 -> bn1.eval() -> ReLU -> max-pool in one launch) against an fp64
restatement built from the kernel's own inputs: the T-rounded pixels, the T-rounded w_fwd and the fp32 scale /
shift. Bars: test_gpu_infer.py's TOL for bf16 (1.5e-2 of max |ref|), test_gpu_infer_f16.py's 2e-3 for fp16. The
three launches it replaces (images -> NHWC4, stem conv, BN + ReLU + max-pool) run on the same operands in the same
test: the fused kernel rounds once where they round twice, so its RMS error must not be the larger one."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from argus_amd._lib import BF16, F16, ConvDesc, FrameSrc, lib, ptr, stream
from argus_amd.data import center_crop_slices

pytestmark = pytest.mark.gpu

TOL = {"bf16": 1.5e-2, "fp16": 2e-3}
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
DT = {"bf16": BF16, "fp16": F16}
GUARD = 4096

# (n_img, H, W) after the crop. 16x16: one ragged tile, pooled 4x4; 30x46: conv 15x23 (odd: the last pool window
# hangs over both edges); 64x64: pooled 16 = one pooled tile width (15) + 1; 72x104: several tiles, ragged both
# ways, 3 images; 24x124: pooled 6x31 = two tile heights exactly, two tile widths + 1
SHAPES = [(2, 16, 16), (2, 30, 46), (2, 64, 64), (3, 72, 104), (2, 24, 124)]


def _pooled(h):
    h1 = (h - 1) // 2 + 1
    return h1, (h1 - 1) // 2 + 1


def _planar_src(t, n_img_stride, H, W, y0=0, x0=0, hs=None, ws=None):
    hs, ws = hs or H, ws or W
    return FrameSrc(ptr(t), 0 if t.dtype == torch.uint8 else 1, n_img_stride, hs * ws, ws, 1, hs, ws, y0, x0)


def _weights(cuda, dt, gen):
    """The stem's w_fwd as argus_conv_weight_prep writes it, and the same values (OIHW, fp64) for the reference."""
    w = (torch.randn(64, 3, 7, 7, generator=gen) / 147 ** 0.5).to(cuda)
    d = ConvDesc(1, 16, 16, 3, 64, 7, 7, 2, 3, 8, 8, 1)
    wf = torch.zeros(64, 8, 8, 4, dtype=TDT[dt], device=cuda)
    lib().conv_weight_prep(C.byref(d), DT[dt], ptr(w), (C.c_int64 * 4)(*w.stride()), ptr(wf), None, stream())
    return wf, wf.cpu()[:, :7, :7, :3].double().permute(0, 3, 1, 2)


def _coeffs(gen):
    """bn1.eval() coefficients with both signs of scale, and a shift negative enough that whole windows are 0."""
    scale = 0.5 + torch.rand(64, generator=gen)
    scale[::5] *= -1
    shift = 0.3 * torch.randn(64, generator=gen)
    shift[3::16] = -100.0
    return scale, shift


def _reference(pix64, w64, scale, shift):
    """fp64: (n, 3, H, W) pixels -> (n, H2, W2, 64)."""
    y = F.conv2d(pix64, w64, stride=2, padding=3)
    z = (y * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]).clamp_min(0)
    return F.max_pool2d(z, 3, 2, 1).permute(0, 2, 3, 1).contiguous()


def _run(cuda, dt, n, H, W, src, wf, scale, shift):
    """One argus_stem_infer launch into a NaN-prefilled buffer with a guard; returns (output, whole buffer)."""
    H2, W2 = _pooled(H)[1], _pooled(W)[1]
    numel = n * H2 * W2 * 64
    buf = torch.full((numel + GUARD,), float("nan"), dtype=TDT[dt], device=cuda)
    lib().stem_infer(DT[dt], n, H, W, 64, C.byref(src), ptr(wf), ptr(scale), ptr(shift), ptr(buf), stream())
    return buf[:numel].view(n, H2, W2, 64), buf


def _parent(cuda, dt, n, H, W, u8, wf, scale, shift):
    """The three launches of the parent session on the same operands."""
    L = lib()
    H1, H2 = _pooled(H)
    W1, W2 = _pooled(W)
    d = ConvDesc(n, H, W, 3, 64, 7, 7, 2, 3, H1, W1, 1)
    x0 = torch.empty(n, H, W, 4, dtype=TDT[dt], device=cuda)
    y0 = torch.empty(n, H1, W1, 64, dtype=TDT[dt], device=cuda)
    out = torch.empty(n, H2, W2, 64, dtype=TDT[dt], device=cuda)
    am = torch.empty(n, H2, W2, 64, dtype=torch.uint8, device=cuda)
    L.images_u8_to_nhwc4(DT[dt], n, H, W, ptr(u8), ptr(x0), stream())
    L.conv_fwd(C.byref(d), DT[dt], ptr(x0), ptr(wf), ptr(y0), None, None, None, stream())
    L.maxpool_fwd(DT[dt], n, H1, W1, 64, ptr(y0), ptr(scale), ptr(shift), ptr(out), ptr(am), stream())
    return out


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("n,H,W", SHAPES, ids=lambda v: str(v))
def test_stem_infer_matches_fp64_and_beats_the_three_launches(cuda, dt, n, H, W):
    gen = torch.Generator().manual_seed(31 * H + W + n)
    u8 = torch.randint(0, 256, (n, 3, H, W), generator=gen, dtype=torch.uint8)
    wf, w64 = _weights(cuda, dt, gen)
    scale, shift = _coeffs(gen)
    ref = _reference((u8.float() / 255.0).to(TDT[dt]).double(), w64, scale, shift)
    assert bool((ref[..., 3::16] == 0).all()) and bool((ref > 0).any())  # whole windows at 0; not everything
    u8g, sc, sh = u8.to(cuda), scale.to(cuda), shift.to(cuda)
    src = _planar_src(u8g, 3 * H * W, H, W)
    out, buf = _run(cuda, dt, n, H, W, src, wf, sc, sh)
    assert bool(torch.isfinite(out).all())                 # every element written (the prefill is NaN)
    assert bool(torch.isnan(buf[out.numel():]).all())      # nothing beyond the tensor
    again, _ = _run(cuda, dt, n, H, W, src, wf, sc, sh)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16))  # bit-reproducible
    theirs = _parent(cuda, dt, n, H, W, u8g, wf, sc, sh)
    e_ours = out.double().cpu() - ref
    e_theirs = theirs.double().cpu() - ref
    bound = TOL[dt] * ref.abs().max().item()
    rms_ours, rms_theirs = e_ours.pow(2).mean().sqrt().item(), e_theirs.pow(2).mean().sqrt().item()
    print(f"stem_infer {dt} {n}x{H}x{W}: max error / bound = {e_ours.abs().max().item() / bound:.3f} (three launches "
          f"{e_theirs.abs().max().item() / bound:.3f}); RMS error {rms_ours:.3e} against {rms_theirs:.3e}")
    assert e_ours.abs().max().item() <= bound
    assert rms_ours <= rms_theirs


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_layouts_crop_and_input_dtypes_give_the_same_bits(cuda, dt):
    """Interleaved 41x77 camera frames cropped on the fly at center_crop_slices' odd offsets (5, 15), the
    pre-cropped planar tensor, uint8 and the fp32 tensor u8 / 255: one set of pixel values, one output."""
    n, Hs, Ws, H, W = 2, 41, 77, 30, 46
    ys, xs = center_crop_slices((Hs, Ws), (H, W))
    assert (ys.start, xs.start) == (5, 15)
    gen = torch.Generator().manual_seed(77)
    hwc = torch.randint(0, 256, (n, Hs, Ws, 3), generator=gen, dtype=torch.uint8)
    chw = hwc[:, ys, xs, :].permute(0, 3, 1, 2).contiguous()
    wf, w64 = _weights(cuda, dt, gen)
    scale, shift = _coeffs(gen)
    sc, sh = scale.to(cuda), shift.to(cuda)
    tensors = {"chw u8": chw.to(cuda), "chw f32": (chw.float() / 255.0).to(cuda),
               "hwc u8": hwc.to(cuda), "hwc f32": (hwc.float() / 255.0).to(cuda)}
    outs = {}
    for name, t in tensors.items():
        if name.startswith("chw"):
            src = _planar_src(t, 3 * H * W, H, W)
        else:
            src = FrameSrc(ptr(t), 0 if t.dtype == torch.uint8 else 1, 3 * Hs * Ws, 1, 3 * Ws, 3, Hs, Ws, ys.start,
                           xs.start)
        outs[name], _ = _run(cuda, dt, n, H, W, src, wf, sc, sh)
    ref = _reference((chw.float() / 255.0).to(TDT[dt]).double(), w64, scale, shift)
    first = outs["chw u8"]
    assert (first.double().cpu() - ref).abs().max().item() <= TOL[dt] * ref.abs().max().item()
    for name, o in outs.items():
        assert torch.equal(o.view(torch.int16), first.view(torch.int16)), name
    # a planar tensor larger than the crop, cropped by the source descriptor
    big = hwc.permute(0, 3, 1, 2).contiguous().to(cuda)
    o, _ = _run(cuda, dt, n, H, W, _planar_src(big, 3 * Hs * Ws, H, W, ys.start, xs.start, Hs, Ws), wf, sc, sh)
    assert torch.equal(o.view(torch.int16), first.view(torch.int16))


def test_fp16_output_saturates_to_the_largest_finite(cuda):
    """A scale that drives the activations far past the fp16 range stores exactly 65504, never inf."""
    n, H, W = 2, 30, 46
    gen = torch.Generator().manual_seed(9)
    u8 = torch.randint(0, 256, (n, 3, H, W), generator=gen, dtype=torch.uint8)
    wf, w64 = _weights(cuda, "fp16", gen)
    scale, shift = torch.full((64,), 1e7), torch.zeros(64)
    ref = _reference((u8.float() / 255.0).to(torch.float16).double(), w64, scale, shift)
    u8g = u8.to(cuda)
    out, _ = _run(cuda, "fp16", n, H, W, _planar_src(u8g, 3 * H * W, H, W), wf, scale.to(cuda), shift.to(cuda))
    out = out.float().cpu()
    assert bool(torch.isfinite(out).all())
    hot = ref > 2 * 65504.0  # far enough above that the kernel's fp32 sum is above too
    assert int(hot.sum()) > hot.numel() // 2
    assert torch.equal(out[hot], torch.full_like(out[hot], 65504.0))
    assert out.max().item() == 65504.0
