"""GPU: frozen inference in fp16 (ARGUS_F16; InferenceSession(compute_dtype="fp16")).

References are fp64 computations on the operands as stored, with the helpers of tests/test_gpu_infer.py. The
kernel bar is 2e-3 of the reference's maximum magnitude: the bf16 bar (1.5e-2) over the unit-roundoff ratio 8,
rounded up; the error is the single output rounding (<= 2^-12 relative), the fp32 accumulation term is what the
fp32 kernel test bounds at 2e-5. Every fp16 store saturates to +-65504 (never inf), which the fold, the conv
epilogue and the session constructor are held to. The session is held to the fp64 oracle twice: within 2x the
reference's own fp16 autocast distance, and at most half the bf16 session's distance.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import test_gpu_infer as base
from argus_amd._lib import BF16, F16, ConvDesc, lib, ptr, stream
from argus_amd.profiling import KernelTimer
from infer_shapes import conv_kernel_name
from test_gpu_infer import PARITY, _bn_params, _desc, _images, _operands, _product, oracle, oracle_fp64  # noqa: F401

pytestmark = pytest.mark.gpu

F16_MAX = 65504.0
TOL16 = 2e-3
# the helpers of test_gpu_infer.py look the dtype up by name: teach them the new one
base.TDT.setdefault("fp16", torch.float16)
base.DT.setdefault("fp16", F16)
base.TOL.setdefault("fp16", TOL16)


def _sat16(t):
    """The library's fp16 rounding of an fp32 tensor: clamp to +-65504, then round to nearest even."""
    return t.clamp(-F16_MAX, F16_MAX).to(torch.float16)


# ---- 4. fold ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,k,hot", [(64, 64, 1, None), (64, 192, 3, None), (256, 64, 1, None), (64, 128, 3, 5)])
def test_fold_is_bit_exact_and_saturates(cuda, cin, cout, k, hot):
    L = lib()
    gen = torch.Generator().manual_seed(100 + cin + cout + k)
    w_oihw = torch.randn(cout, cin, k, k, generator=gen).to(cuda)
    gamma, beta, mean, var = _bn_params(cout, gen, cuda)
    if hot is not None:
        gamma[hot] = 3e5  # scale ~ 3e5: |w * scale| > 65504 wherever |w| > ~0.25
    eps = 1e-5
    scale, shift = torch.empty(cout, device=cuda), torch.empty(cout, device=cuda)
    L.bn_eval_coeffs(cout, ptr(gamma), ptr(beta), ptr(mean), ptr(var), C.c_float(eps), ptr(scale), ptr(shift), stream())
    d = _desc(2, 8, 8, cin, cout, k, 1)
    ohwi = w_oihw.permute(0, 2, 3, 1).contiguous()
    prod = ohwi * scale[:, None, None, None]
    want = prod.to(torch.float16) if hot is None else _sat16(prod)
    cl = w_oihw.contiguous(memory_format=torch.channels_last)
    for master, strides in ((ohwi, None), (cl, (C.c_int64 * 4)(*cl.stride()))):
        wf = torch.zeros(cout, k, k, cin, dtype=torch.float16, device=cuda)
        bias = torch.zeros(cout, device=cuda)
        L.conv_fold_bn(C.byref(d), F16, ptr(master), strides, ptr(gamma), ptr(beta), ptr(mean), ptr(var),
                       C.c_float(eps), ptr(wf), ptr(bias), stream())
        assert torch.equal(bias.view(torch.int32), shift.view(torch.int32))
        assert torch.equal(wf.view(torch.int16), want.view(torch.int16))
        assert bool(torch.isfinite(wf).all())
        if hot is not None:
            over = prod[hot].abs() > F16_MAX
            assert 0 < int(over.sum()) < over.numel()
            assert torch.equal(wf[hot][over].float(), torch.sign(prod[hot][over]) * F16_MAX)
            assert float(wf[torch.arange(cout, device=cuda) != hot].abs().max()) < 100  # the others: untouched


# ---- 5. kernel parity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PARITY, ids=lambda s: "x".join(map(str, s)))
def test_conv_infer_parity_fp16(cuda, shape):
    L = lib()
    d, x, wf, bias, res, y, resd = _operands(cuda, "fp16", *shape)
    assert (y < 0).float().mean() > 0.2  # ReLU matters
    mx = L.dll.argus_conv_infer_max_splits(C.byref(d), F16)
    assert mx == shape[5] * shape[5] * shape[3] // 64
    default = L.dll.argus_conv_infer_splits(C.byref(d), F16)
    assert 1 <= default <= mx
    nbytes = max(L.dll.argus_conv_infer_workspace_bytes(C.byref(d), F16, mx), 16)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=cuda)  # zeroed once for all the calls below
    splits = sorted({min(s, mx) for s in (1, 2, 3, mx)}) + [0]
    worst = 0.0
    with KernelTimer() as timer:
        for use_res in (False, True):
            for relu in (0, 1):
                ref = y + resd if use_res else y
                ref = ref.clamp_min(0) if relu else ref
                bound = TOL16 * ref.abs().max().item()
                for sp in splits:
                    out = torch.full(ref.shape, float("nan"), dtype=torch.float16, device=cuda)
                    L.conv_infer(C.byref(d), F16, ptr(x), ptr(wf), ptr(bias), ptr(res) if use_res else None, relu,
                                 ptr(out), sp, ptr(ws), ws.numel(), stream())
                    err = (out.double().cpu() - ref).abs().max().item()  # NaN (an unwritten element) fails the bound
                    worst = max(worst, err / bound)
                    assert err <= bound, f"{shape} fp16 res={use_res} relu={relu} splits={sp}: {err:.3e} > {bound:.3e}"
    want = conv_kernel_name("fwd", "fp16", shape)
    base._only_conv(timer, want, 4 * len(splits))  # the instantiation the tile-height rule names, and no other
    print(f"conv_infer {shape} fp16: worst error / bound = {worst:.3f} (default splits {default}, max {mx}); {want}")


# ---- 6. saturation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign,relu", [(1, 1), (-1, 0)])
def test_conv_infer_saturates_to_the_largest_finite(cuda, sign, relu):
    """Every second output channel gets a bias of +-7e4: those outputs leave the fp16 range and must read
    +-65504 exactly; the channels in between keep their bias and the parity bar."""
    L = lib()
    shape = PARITY[1]
    d, x, wf, bias, res, y, resd = _operands(cuda, "fp16", *shape)
    big = bias.clone()
    big[::2] = sign * 7e4
    ref = y - bias.double().cpu() + big.double().cpu() + resd
    ref = ref.clamp_min(0) if relu else ref
    hot = ref.abs() > F16_MAX
    assert bool(hot[..., ::2].all()) and not bool(hot[..., 1::2].any())
    default = L.dll.argus_conv_infer_splits(C.byref(d), F16)
    for sp in (1, 0, 3):  # unsplit, the default split, an uneven split
        nbytes = max(L.dll.argus_conv_infer_workspace_bytes(C.byref(d), F16, max(3, default)), 16)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=cuda)
        out = torch.full(ref.shape, float("nan"), dtype=torch.float16, device=cuda)
        L.conv_infer(C.byref(d), F16, ptr(x), ptr(wf), ptr(big), ptr(res), relu, ptr(out), sp, ptr(ws), ws.numel(),
                     stream())
        o = out.double().cpu()
        assert bool(torch.isfinite(o).all())  # no inf, no NaN anywhere
        assert torch.equal(o[hot], torch.full_like(o[hot], sign * F16_MAX))
        cold = ref[~hot]
        assert (o[~hot] - cold).abs().max().item() <= TOL16 * cold.abs().max().item()


# ---- 7. split determinism and ticket hygiene ------------------------------------------------------------------
def test_split_is_deterministic_and_leaves_tickets_zero_fp16(cuda):
    base.test_split_is_deterministic_and_leaves_tickets_zero(cuda, "fp16")  # the same body, NULL workspace included


# ---- 8. the stem, both kernels --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,W", [(2, 64, 64), (1, 24, 64), (1, 72, 104)], ids=["lds-full", "lds-ragged", "igemm"])
def test_stem_forward_fp16(cuda, n, H, W):
    """64x64 -> 32x32 (LDS-patch kernel, full tiles); 24x64 -> 12x32 (LDS-patch, ragged: exactly 75 % useful);
    72x104 -> 36x52 (73 % useful: the implicit-GEMM fallback)."""
    L = lib()
    gen = torch.Generator().manual_seed(11 + H + W)
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    d = ConvDesc(n, H, W, 3, 64, 7, 7, 2, 3, Ho, Wo, 1)
    x = torch.zeros(n, H, W, 4, dtype=torch.float16)
    x[..., :3] = torch.randn(n, H, W, 3, generator=gen).to(torch.float16)
    w = (torch.randn(64, 3, 7, 7, generator=gen) / 147 ** 0.5).to(cuda)
    wf = torch.full((64, 8, 8, 4), float("nan"), dtype=torch.float16, device=cuda)
    L.conv_weight_prep(C.byref(d), F16, ptr(w), (C.c_int64 * 4)(*w.stride()), ptr(wf), None, stream())
    want_w = torch.zeros(64, 8, 8, 4, dtype=torch.float16)
    want_w[:, :7, :7, :3] = w.cpu().permute(0, 2, 3, 1).to(torch.float16)
    assert torch.equal(wf.cpu().view(torch.int16), want_w.view(torch.int16))  # padded (r8, s8, c4), zeros in the pad
    ref = F.conv2d(x[..., :3].double().permute(0, 3, 1, 2), want_w[:, :7, :7, :3].double().permute(0, 3, 1, 2),
                   stride=2, padding=3).permute(0, 2, 3, 1)
    numel, guard = n * Ho * Wo * 64, 4096
    buf = torch.full((numel + guard,), float("nan"), dtype=torch.float16, device=cuda)
    from argus_amd.profiling import KernelTimer

    xg = x.to(cuda)
    with KernelTimer() as t:
        L.conv_fwd(C.byref(d), F16, ptr(xg), ptr(wf), ptr(buf), None, None, None, stream())
    names = list(t.summary())
    lds = "argus::stem_fwd_kernel<_Float16>"
    assert names == [lds if (H, W) != (72, 104) else "argus::igemm_kernel<_Float16, 128, 64, true, false, 4, 0>"], names
    out = buf[:numel].view(n, Ho, Wo, 64).double().cpu()
    assert bool(torch.isnan(buf[numel:]).all())  # nothing beyond the tensor
    assert not bool(torch.isnan(out).any())      # every pixel written
    err, bound = (out - ref).abs().max().item(), TOL16 * ref.abs().max().item()
    print(f"stem fp16 {n}x{H}x{W}: error / bound = {err / bound:.3f}")
    assert err <= bound


# ---- 9. layout and pools --------------------------------------------------------------------------------------
def test_images_to_nhwc4_fp16(cuda):
    L = lib()
    gen = torch.Generator().manual_seed(5)
    n, H, W = 3, 10, 14
    xf = torch.rand(n, 3, H, W, generator=gen)
    u8 = torch.randint(0, 256, (n, 3, H, W), generator=gen, dtype=torch.uint8)
    for src, val, fn in ((xf, xf, L.images_to_nhwc4), (u8, u8.float() / 255.0, L.images_u8_to_nhwc4)):
        out = torch.full((n, H, W, 4), float("nan"), dtype=torch.float16, device=cuda)
        srcg = src.to(cuda)  # (held: a temporary's memory could be handed out again before the launch runs)
        fn(F16, n, H, W, ptr(srcg), ptr(out), stream())
        want = torch.zeros(n, H, W, 4, dtype=torch.float16)
        want[..., :3] = val.permute(0, 2, 3, 1).to(torch.float16)
        assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


def test_pools_fp16(cuda):
    L = lib()
    gen = torch.Generator().manual_seed(6)
    n, H, W, c = 2, 13, 9, 64
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.randn(n, H, W, c, generator=gen).to(torch.float16)
    sc, sh = 0.5 + torch.rand(c, generator=gen), 0.3 * torch.randn(c, generator=gen)
    out = torch.full((n, Ho, Wo, c), float("nan"), dtype=torch.float16, device=cuda)
    am = torch.full((n, Ho, Wo, c), 255, dtype=torch.uint8, device=cuda)
    yg, scg, shg = y.to(cuda), sc.to(cuda), sh.to(cuda)
    L.maxpool_fwd(F16, n, H, W, c, ptr(yg), ptr(scg), ptr(shg), ptr(out), ptr(am), stream())
    # fmaf(y, scale, shift): the product of an fp16 and an fp32 is exact in fp64, so one fp64 sum rounded to fp32
    z = (y.double() * sc.double() + sh.double()).float().clamp_min(0)
    best = torch.full((n, Ho, Wo, c), float("-inf"))
    idx = torch.zeros(n, Ho, Wo, c, dtype=torch.uint8)
    for r in range(3):  # the kernels' convention: taps in (r, s) order, a strictly larger value wins
        for t in range(3):
            for oh in range(Ho):
                ih = 2 * oh - 1 + r
                if not 0 <= ih < H:
                    continue
                ows = [ow for ow in range(Wo) if 0 <= 2 * ow - 1 + t < W]
                cand = z[:, ih, [2 * ow - 1 + t for ow in ows]]
                cur = best[:, oh, ows]
                win = cand > cur
                best[:, oh, ows] = torch.where(win, cand, cur)
                idx[:, oh, ows] = torch.where(win, torch.full_like(idx[:, oh, ows], r * 3 + t), idx[:, oh, ows])
    assert torch.equal(out.cpu().view(torch.int16), best.to(torch.float16).view(torch.int16))
    assert torch.equal(am.cpu(), idx)
    # the bf16 kernel's argmax on inputs both formats hold exactly (multiples of 1/16 below 4: ties in most windows)
    yq = torch.randint(-64, 64, (n, H, W, c), generator=gen).float() / 16
    ob, ab = torch.empty(n, Ho, Wo, c, dtype=torch.bfloat16, device=cuda), torch.empty_like(am)
    o16, a16 = torch.empty_like(out), torch.empty_like(am)
    yqb, yqh = yq.to(torch.bfloat16).to(cuda), yq.to(torch.float16).to(cuda)
    L.maxpool_fwd(BF16, n, H, W, c, ptr(yqb), ptr(scg), ptr(shg), ptr(ob), ptr(ab), stream())
    L.maxpool_fwd(F16, n, H, W, c, ptr(yqh), ptr(scg), ptr(shg), ptr(o16), ptr(a16), stream())
    assert torch.equal(ab, a16)
    # average pool: activations after a ReLU are non-negative, so "relative to the mean" is well conditioned
    x = (4 * torch.rand(n, H * W, c, generator=gen)).to(torch.float16)
    feat = torch.full((n, c), float("nan"), device=cuda)
    xg = x.to(cuda)
    L.avgpool_fwd(F16, n, H * W, c, ptr(xg), ptr(feat), stream())
    want = x.double().mean(1)
    assert ((feat.double().cpu() - want).abs() / want).max().item() <= 1e-6


# ---- 10. the session against the fp64 oracle --------------------------------------------------------------------
# LDS-patch stem / fallback stem / the smallest session with 64-row conv tiles (LDS-patch stem)
@pytest.mark.parametrize("hw", base.SESSION_HW, ids=base.SESSION_IDS)
def test_fp16_session_matches_the_fp64_oracle(cuda, oracle, oracle_fp64, hw):
    """d = max |prediction - fp64 oracle|, B = 2. Measured on an MI355X: 64x64 fp16 session
    9.58e-3, reference fp16 autocast 7.74e-3, bf16 session 3.77e-2; 72x104 7.44e-3, 1.20e-2, 4.45e-2."""
    from argus_amd.infer import InferenceSession

    x = (_images(hw).float() / 255.0)
    ref = oracle_fp64[hw]
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.float16):
        d_ref = (oracle(x).double() - ref).abs().max().item()  # the reference's own --amp mode, on the CPU
    m = _product(oracle, cuda, "fp32")
    xc = x.to(cuda)
    s16 = InferenceSession(m, 2, hw, compute_dtype="fp16")
    d_fp16 = (s16(xc).double().cpu() - ref).abs().max().item()
    d_bf16 = (InferenceSession(_product(oracle, cuda, "bf16"), 2, hw)(xc).double().cpu() - ref).abs().max().item()
    peak = s16.activation_peak(xc)
    print(f"fp16 session vs fp64 oracle {hw}: fp16 session {d_fp16:.3e}; reference fp16 autocast (CPU) {d_ref:.3e}; "
          f"bf16 session {d_bf16:.3e}; max |pred| {ref.abs().max().item():.2f}; fp16 / bf16 {d_fp16 / d_bf16:.3f}; "
          f"fp16 / (2 x ref) {d_fp16 / (2 * d_ref):.3f}; activation peak {peak:.1f}")
    assert d_fp16 <= 2 * d_ref      # (a) within 2x the reference's own reduced-precision mode
    assert d_fp16 <= 0.5 * d_bf16   # (b) the point of the feature: a build that ran bf16 fails both


# ---- 11. session semantics --------------------------------------------------------------------------------------
class _Peek:
    """Forwards the library calls of a schedule and reads back |max| of every activation buffer one writes."""

    def __init__(self, L, pool):
        self._L, self.dll, self.n, self.peak = L, L.dll, 0, 0.0
        self._pool = {t.data_ptr(): t for t in pool}

    def _see(self, p, elements):
        self.peak = max(self.peak, float(self._pool[p][:elements].abs().max()))

    def __getattr__(self, name):
        fn = getattr(self._L, name)

        def call(*a):
            self.n += 1
            rc = fn(*a)
            if name == "conv_infer":
                d = a[0]._obj
                self._see(a[7], d.n * d.ho * d.wo * d.k)
            elif name == "conv_fwd":
                d = a[0]._obj
                self._see(a[4], d.n * d.ho * d.wo * d.k)
            elif name == "maxpool_fwd":
                self._see(a[8], a[1] * ((a[2] - 1) // 2 + 1) * ((a[3] - 1) // 2 + 1) * a[4])
            return rc
        return call


def test_fp16_session_semantics(cuda, oracle):
    from argus_amd.infer import InferenceSession

    hw = (64, 64)
    model = _product(oracle, cuda, "fp32")
    u8a, u8b = _images(hw, 1), _images(hw, 2)
    xa, xb = (u8a.float() / 255.0).to(cuda), (u8b.float() / 255.0).to(cuda)
    u8a = u8a.to(cuda)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    sg = InferenceSession(model, 2, hw, compute_dtype="fp16", graph=True)
    se = InferenceSession(model, 2, hw, compute_dtype="fp16", graph=False)
    assert sg.pool[0].dtype == torch.float16 and sg.stem_wf.dtype == torch.float16 and sg.compute_dtype == "fp16"
    ya = sg(xa)
    assert ya.shape == (2, 6) and ya.dtype == torch.float32
    assert torch.equal(ya, se(xa))  # replayed graph == eager launches
    yb = sg(xb)
    assert not torch.equal(ya, yb)
    assert torch.equal(sg(xa), ya) and torch.equal(se(xb), yb)
    assert torch.equal(sg(u8a), ya) and torch.equal(se(u8a), ya)  # uint8 == its /255 float batch
    assert ya.data_ptr() != sg(xa).data_ptr()  # a fresh tensor per call
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)  # the model is untouched
    assert sg.launches_per_forward == InferenceSession(model, 2, hw, compute_dtype="bf16").launches_per_forward
    # activation_peak against the same buffers read back from an eager run
    se.L = peek = _Peek(se.L, se.pool)
    se(xa)
    se.L = peek._L
    assert peek.n == se.launches_per_forward
    peak = sg.activation_peak(xa)
    assert abs(peak - peek.peak) <= 0.02 * peek.peak and 0 < peak < F16_MAX
    assert sg.activation_peak(u8a) == peak and torch.equal(sg(xa), ya)  # the diagnostic disturbs nothing
    # every dtype has it: the fp32 session sees the same activations up to fp16's rounding of them
    p32 = InferenceSession(model, 2, hw, compute_dtype="fp32", graph=False).activation_peak(xa)
    assert abs(p32 - peak) <= 0.02 * p32
    # a snapshot: a changed bias shows after refresh()
    model.output_mlp[4].bias.data += 1
    assert torch.equal(sg(xa), ya)
    sg.refresh()
    assert torch.allclose(sg(xa), ya + 1, rtol=0, atol=2e-6 * float(ya.abs().max() + 1))
    # a checkpoint fp16 cannot hold: one gamma scaled until a folded weight saturates
    model.resnet.layer2[1].bn2.weight.data[3] *= 1e7
    with pytest.raises(ValueError, match=r"layer2\.1\.conv2"):
        InferenceSession(model, 2, hw, compute_dtype="fp16")
    with pytest.raises(ValueError, match=r"layer2\.1\.conv2"):
        sg.refresh()
    InferenceSession(model, 2, hw, compute_dtype="bf16")  # the other dtypes still take it


# ---- 12. validate ---------------------------------------------------------------------------------------------
def test_validate_with_an_fp16_session(cuda, dummy_data_path, tmp_path):
    """The fixture of test_gpu_train.py's validate test (5 test samples, 256 x 256), batch 2: two full batches and
    a padded tail. Tolerance per example: with delta = 2 x d_ref (d_ref = the reference model's own max
    |fp16-autocast prediction - fp32 prediction| on these five samples, CPU), |loss16 - loss32| <=
    ||dloss/dpred||_1 * delta + 6 * delta^2: the first-order change of the loss for a prediction moved by delta
    in every coordinate (the loss kernel's exact gradient), plus the second-order term of a sum of six squares."""
    from argus_amd.data import AugmentationConfig, CameraCubePoseDataset, CameraCubePoseDatasetConfig
    from argus_amd.losses import geometric_loss_fn
    from argus_amd.models import NCameraCNN
    from argus_amd.validate import ValConfig, validate
    from oracle.ncamera import build_reference_model

    torch.manual_seed(4)
    src = NCameraCNN()
    path = tmp_path / "m.pth"
    torch.save(src.state_dict(), path)
    noaug = AugmentationConfig(num_spaghetti=0)
    dcfg = CameraCubePoseDatasetConfig(dummy_data_path)
    kw = dict(model_path=str(path), dataset_config=dcfg, aug_config=noaug, batch_size=2)
    l32 = validate(ValConfig(**kw))
    l16 = validate(ValConfig(**kw, session_dtype="fp16"))
    assert len(l16) == len(l32) == 5
    ds = CameraCubePoseDataset(dcfg, cfg_aug=noaug, train=False)
    x = torch.stack([ds[i]["images"] for i in range(5)])
    T = torch.stack([ds[i]["cube_pose"] for i in range(5)]).float()
    ref = build_reference_model(0)
    ref.load_state_dict(src.state_dict())
    ref.eval()
    with torch.no_grad():
        p32 = ref(x)
        with torch.autocast("cpu", dtype=torch.float16):
            d_ref = (ref(x).float() - p32).abs().max().item()
    pred = p32.to(cuda).requires_grad_(True)
    geometric_loss_fn(pred, T.to(cuda)).sum().backward()
    delta = 2 * d_ref
    tol = pred.grad.abs().sum(-1).cpu() * delta + 6 * delta * delta
    diff = (torch.tensor(l16) - torch.tensor(l32)).abs()
    print(f"validate fp16 session: d_ref {d_ref:.3e}, |loss16 - loss32| / tolerance {(diff / tol).tolist()}")
    assert bool((diff <= tol).all()), (l16, l32, tol.tolist())
