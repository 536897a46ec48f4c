"""GPU: the frozen gradient (argus_conv_fold_bn_dgrad, argus_conv_infer_dgrad, argus_avgpool_bwd_relu,
argus_amd.infer_grad.GradientSession).

Kernel bars are the existing ones of tests/test_gpu_kernels.py / test_gpu_infer.py: 2e-5 (fp32) / 1.5e-2 (bf16) of
the reference's maximum magnitude against an fp64 torch.nn.grad.conv2d_input on the operands as stored. The second
folded weight copy is checked bit for bit against argus_conv_fold_bn's. The session is checked launch by launch
(debug=True) against an fp64 re-derivation from the GPU tensors the schedule names as that launch's inputs, with
the stage bars of test_gpu_model.py / test_gpu_parity.py (rel_max 2e-5 fp32 / 1e-2 bf16; the stem stage with
test_stem_dgrad_kernel's with-apply bars 2e-5 / 3e-2), and end to end against the CPU oracle's eval-mode autograd
in double within twice the distance d_ref of the CPU reference's own bf16-autocast gradient from its fp32 one.

Measured on an MI355X (e = |g - g64| / |g64| of vjp against the fp64 oracle; d_ref as above; the CPU fp32
reference's own distance from fp64 in brackets):
  64x64:  fp32 e = 4.0e-6, bf16 e = 0.375, d_ref = 0.412 [3.4e-6];  72x104: fp32 e = 4.5e-3, bf16 e = 0.420,
  d_ref = 0.451 [1.4e-4]. Worst stage rel_max / bar: fp32 0.036 (layer4.0.downsample, 72x104), bf16 0.346
  (layer1.2.conv3, 64x64); stem stage 0.018 / 0.072. Worst kernel error / bound: fp32 0.113, bf16 0.191.
  128x128 (the smallest session with 64-row tiles): fp32 e = 6.2e-3, bf16 e = 0.385, d_ref = 0.430 [9.1e-4]; worst
  stage rel_max / bar fp32 0.054 (layer3.0.downsample), bf16 0.353 (layer2.1.conv1); forward conv by conv, worst
  error / bound fp32 0.039, bf16 0.245.

The parity shapes live in tests/infer_shapes.py with the Python mirror of the library's tile-height rule; every
parity case asserts through the kernel timer that it launched the instantiation the mirror names.
"""
import ctypes as C

import pytest
import torch
import torch.nn as nn

from argus_amd._lib import BF16, F32, ConvDesc, lib, ptr, stream
from argus_amd.profiling import KernelTimer
from infer_shapes import DGRAD_PARITY, conv_kernel_name, is_frozen_conv, session_convs

pytestmark = pytest.mark.gpu

TOL = {"fp32": 2e-5, "bf16": 1.5e-2}
STAGE = {"fp32": 2e-5, "bf16": 1e-2}
STEM = {"fp32": 2e-5, "bf16": 3e-2}
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
DT = {"fp32": F32, "bf16": BF16}
BITS = {"fp32": torch.int32, "bf16": torch.int16}


def _desc(n, h, w, cin, cout, k, s):
    p = 1 if k == 3 else 0
    return ConvDesc(n, h, w, cin, cout, k, k, s, p, (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1, 0)


def _plan(d, dt, splits_in=0):
    sp, mx, nb = C.c_int(0), C.c_int(0), C.c_size_t(0)
    lib().conv_infer_dgrad_plan(C.byref(d), DT[dt], splits_in, C.byref(sp), C.byref(mx), C.byref(nb))
    return sp.value, mx.value, nb.value


def _dx64(d, dy64_nhwc, w64_oihw):
    """fp64 conv_transpose: F.conv2d's gradient with respect to its input, NHWC in and out."""
    g = torch.nn.grad.conv2d_input((d.n, d.c, d.h, d.w), w64_oihw, dy64_nhwc.permute(0, 3, 1, 2).contiguous(),
                                   stride=d.stride, padding=d.pad)
    return g.permute(0, 2, 3, 1).contiguous()


def _rel_max(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ---- 1. fold: the second copy holds argus_conv_fold_bn's values, transposed and rotated ---------------------
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("cin,cout,k", [(64, 64, 1), (64, 192, 3), (256, 64, 1)])
def test_fold_dgrad_is_the_forward_fold_permuted_and_flipped(cuda, dt, cin, cout, k):
    L = lib()
    gen = torch.Generator().manual_seed(300 + cin + cout + k)
    w_oihw = torch.randn(cout, cin, k, k, generator=gen).to(cuda)
    gamma, beta, mean, var = [(0.5 + torch.rand(cout, generator=gen)).to(cuda) for _ in range(4)]
    eps = C.c_float(1e-5)
    d = _desc(2, 8, 8, cin, cout, k, 1)
    ohwi = w_oihw.permute(0, 2, 3, 1).contiguous()
    cl = w_oihw.contiguous(memory_format=torch.channels_last)
    for master, strides in ((ohwi, None), (cl, (C.c_int64 * 4)(*cl.stride())),
                            (w_oihw, (C.c_int64 * 4)(*w_oihw.stride()))):
        wf = torch.zeros(cout, k, k, cin, dtype=TDT[dt], device=cuda)
        bias = torch.zeros(cout, device=cuda)
        L.conv_fold_bn(C.byref(d), DT[dt], ptr(master), strides, ptr(gamma), ptr(beta), ptr(mean), ptr(var), eps,
                       ptr(wf), ptr(bias), stream())
        wfd = torch.full((cin, k, k, cout), float("nan"), dtype=TDT[dt], device=cuda)
        L.conv_fold_bn_dgrad(C.byref(d), DT[dt], ptr(master), strides, ptr(gamma), ptr(beta), ptr(mean), ptr(var), eps,
                             ptr(wfd), stream())
        want = wf.permute(3, 1, 2, 0).flip(1, 2).contiguous()  # [c][R-1-r][S-1-s][k]
        assert torch.equal(wfd.view(BITS[dt]), want.view(BITS[dt]))


# ---- 2. kernel parity ---------------------------------------------------------------------------------------
PARITY = DGRAD_PARITY  # tests/infer_shapes.py: (n, h, w, cin, cout, k, stride)


def _only_conv(timer, want, launches):
    """The one frozen conv instantiation the launches under ``timer`` ran is ``want``, ``launches`` times."""
    got = {n: v["launches"] for n, v in timer.summary().items() if is_frozen_conv(n)}
    assert got == {want: launches}, f"launched {got}, expected {launches} of {want}"


def _operands(cuda, dt, n, h, w, cin, cout, k, s, seed=0):
    gen = torch.Generator().manual_seed(seed + 11 * cin + cout + k + s)
    d = _desc(n, h, w, cin, cout, k, s)
    dy = torch.randn(n, d.ho, d.wo, cout, generator=gen).to(TDT[dt])
    wf = (torch.randn(cout, k, k, cin, generator=gen) / (k * k * cout) ** 0.5).to(TDT[dt])  # the forward copy, OHWI
    wfd = wf.permute(3, 1, 2, 0).flip(1, 2).contiguous()  # what argus_conv_fold_bn_dgrad stores (test 1)
    addend = torch.randn(n, h, w, cin, generator=gen).to(TDT[dt])
    mask = torch.randn(n, h, w, cin, generator=gen)
    mask[torch.rand(n, h, w, cin, generator=gen) < 0.05] = 0.0  # exact zeros: > 0, not >= 0
    mask = mask.to(TDT[dt])
    ct = _dx64(d, dy.double(), wf.double().permute(0, 3, 1, 2).contiguous())
    reached = _dx64(d, torch.ones(n, d.ho, d.wo, cout, dtype=torch.float64),
                    torch.ones(cout, cin, k, k, dtype=torch.float64)) > 0  # dx pixels some tap reaches
    return d, dy.to(cuda), wfd.to(cuda), addend.to(cuda), mask.to(cuda), ct, reached


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", PARITY, ids=lambda s: "x".join(map(str, s)))
def test_conv_infer_dgrad_parity(cuda, dt, shape):
    L = lib()
    d, dy, wfd, addend, mask, ct, reached = _operands(cuda, dt, *shape)
    pos = (mask > 0).float().mean().item()
    assert 0.3 <= pos <= 0.7 and int((mask == 0).sum()) > 0  # the mask matters, zeros included
    default, mx, _ = _plan(d, dt)
    assert mx == shape[5] * shape[5] * shape[4] // (64 if dt == "bf16" else 32) and 1 <= default <= mx
    ws = torch.zeros(max(_plan(d, dt, mx)[2], 16), dtype=torch.uint8, device=cuda)  # zeroed once for all the calls
    splits = sorted({min(s, mx) for s in (1, 2, 3, mx)}) + [0]
    if shape[6] == 2 and shape[5] == 1:
        assert (~reached).float().mean() > 0.5  # a 1x1 stride-2 conv never reads most of its input
    add64, m64 = addend.double().cpu(), (mask.double().cpu() > 0).double()
    worst = 0.0
    with KernelTimer() as timer:
        for use_mask in (False, True):
            for use_add in (False, True):
                ref = ct + add64 if use_add else ct
                ref = ref * m64 if use_mask else ref
                bound = TOL[dt] * ref.abs().max().item()
                # where no tap reaches, dx is the (masked) addend, or zero, exactly
                exact = (add64 if use_add else torch.zeros_like(ct)) * (m64 if use_mask else 1.0)
                for sp in splits:
                    dx = torch.full(ref.shape, float("nan"), dtype=TDT[dt], device=cuda)
                    L.conv_infer_dgrad(C.byref(d), DT[dt], ptr(dy), ptr(wfd), ptr(addend) if use_add else None,
                                       ptr(mask) if use_mask else None, ptr(dx), sp, ptr(ws), ws.numel(), stream())
                    got = dx.double().cpu()
                    assert not torch.isnan(got).any(), f"{shape} {dt} splits={sp}: an element of dx was not written"
                    err = (got - ref).abs().max().item()
                    worst = max(worst, err / bound)
                    assert err <= bound, \
                        f"{shape} {dt} mask={use_mask} addend={use_add} splits={sp}: {err:.3e} > {bound:.3e}"
                    if shape[6] == 2:
                        assert torch.equal(got[~reached], exact[~reached]), f"{shape} {dt} splits={sp}: untouched pixels"
    want = conv_kernel_name("dgrad", dt, shape)
    _only_conv(timer, want, 4 * len(splits))  # the instantiation the tile-height rule names, and no other
    print(f"conv_infer_dgrad {shape} {dt}: worst error / bound = {worst:.3f} (default splits {default}, max {mx}); "
          f"{want}")


# ---- 3. split determinism and workspace hygiene ------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_split_is_deterministic_and_leaves_tickets_zero(cuda, dt):
    L = lib()
    d, dy, wfd, addend, mask, ct, _ = _operands(cuda, dt, 2, 8, 8, 512, 512, 3, 1)
    _, mx, _ = _plan(d, dt)
    wsb = [_plan(d, dt, s)[2] for s in (2, 3, 4)]
    slab = wsb[1] - wsb[0]
    tickets = wsb[0] - 2 * slab  # bytes of ticket words at the start of the workspace
    assert tickets > 0 and wsb[2] == tickets + 4 * slab
    ws = torch.zeros(_plan(d, dt, mx)[2], dtype=torch.uint8, device=cuda)  # zeroed once only
    for sp in (2, 3, 4, mx):
        outs = []
        for _ in range(2):
            dx = torch.empty(ct.shape, dtype=TDT[dt], device=cuda)
            L.conv_infer_dgrad(C.byref(d), DT[dt], ptr(dy), ptr(wfd), ptr(addend), ptr(mask), ptr(dx), sp, ptr(ws),
                               ws.numel(), stream())
            outs.append(dx)
            assert int(ws[:tickets].count_nonzero()) == 0  # every call leaves the tickets zero
        assert torch.equal(outs[0].view(BITS[dt]), outs[1].view(BITS[dt])), sp
    assert int(ws[tickets:].count_nonzero()) > 0  # the slabs were really used
    # splits = 1 takes no ticket and touches no workspace: NULL is fine
    dx1 = torch.empty(ct.shape, dtype=TDT[dt], device=cuda)
    L.conv_infer_dgrad(C.byref(d), DT[dt], ptr(dy), ptr(wfd), ptr(addend), ptr(mask), ptr(dx1), 1, None, 0, stream())
    ref = (ct + addend.double().cpu()) * (mask.double().cpu() > 0)
    assert (dx1.double().cpu() - ref).abs().max().item() <= TOL[dt] * ref.abs().max().item()


# test_gpu_infer.py's TICKETS_1056 with cin and cout swapped: dx is 2070 rows x 2048 columns, 33 x 32 = 1056 tiles
# of 64 rows, past the 1024 tickets of the fixed 4 KB region
TICKETS_1056 = (1, 45, 46, 2048, 256, 1, 1)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_forced_split_above_1024_tiles_grows_the_ticket_region(cuda, dt):
    """The default rule never splits such a grid; a caller may. The ticket region is then 8 KB, the slabs start
    behind it, and the hand-off works as below 1024 tiles: right, deterministic, every ticket left zero."""
    L = lib()
    d, dy, wfd, addend, mask, ct, _ = _operands(cuda, dt, *TICKETS_1056)
    assert _plan(d, dt)[0] == 1
    wsb = [_plan(d, dt, s)[2] for s in (2, 3, 4)]
    slab = wsb[1] - wsb[0]
    tickets = wsb[0] - 2 * slab  # bytes of ticket words at the start of the workspace
    assert tickets == 8192 and slab == 1056 * 64 * 64 * 4 and wsb[2] == tickets + 4 * slab
    ws = torch.zeros(wsb[0], dtype=torch.uint8, device=cuda)  # a workspace of its own, zeroed once only
    ref = (ct + addend.double().cpu()) * (mask.double().cpu() > 0)
    bound = TOL[dt] * ref.abs().max().item()
    outs = []
    with KernelTimer() as timer:
        for _ in range(2):
            dx = torch.full(ct.shape, float("nan"), dtype=TDT[dt], device=cuda)
            L.conv_infer_dgrad(C.byref(d), DT[dt], ptr(dy), ptr(wfd), ptr(addend), ptr(mask), ptr(dx), 2, ptr(ws),
                               ws.numel(), stream())
            outs.append(dx)
            assert int(ws[:tickets].count_nonzero()) == 0  # every call leaves every ticket byte zero
    _only_conv(timer, conv_kernel_name("dgrad", dt, TICKETS_1056), 2)
    assert conv_kernel_name("dgrad", dt, TICKETS_1056).endswith(", 64>")
    err = (outs[0].double().cpu() - ref).abs().max().item()
    print(f"conv_infer_dgrad {TICKETS_1056} {dt} splits=2, 1056 tiles: error / bound = {err / bound:.3f}")
    assert err <= bound, f"{err:.3e} > {bound:.3e}"
    assert torch.equal(outs[0].view(BITS[dt]), outs[1].view(BITS[dt]))
    assert int(ws[tickets:].count_nonzero()) > 0  # the slabs were really used


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_one_workspace_serves_convs_of_different_tile_counts(cuda, dt):
    """A session passes one workspace to every conv. A 128-tile conv and a 32-tile conv, both split, in turn: the
    slabs of the one must not land on the ticket words of the other (forward and data gradient)."""
    L = lib()
    gen = torch.Generator().manual_seed(17)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(TDT[dt]).to(cuda)  # noqa: E731
    small = _desc(2, 8, 8, 512, 512, 3, 1)     # 128 rows: 32 tiles either way
    wide = _desc(2, 32, 32, 128, 128, 1, 1)    # 2048 rows x 128 columns = 128 tiles, forward and data gradient
    ws = torch.zeros(1 << 23, dtype=torch.uint8, device=cuda)  # zeroed once
    xs, ws_ = rnd(2, 8, 8, 512), rnd(512, 9 * 512) * 0.02
    bias = torch.zeros(512, device=cuda)

    def fwd_wide(out):
        L.conv_infer(C.byref(wide), DT[dt], ptr(xw), ptr(ww), ptr(bias), None, 0, ptr(out), 2, ptr(ws), ws.numel(),
                     stream())

    def bwd_wide(out):
        L.conv_infer_dgrad(C.byref(wide), DT[dt], ptr(dyw), ptr(wdw), None, None, ptr(out), 2, ptr(ws), ws.numel(),
                           stream())

    xw, ww = rnd(2, 32, 32, 128), rnd(128, 128) * 0.1
    dyw, wdw = rnd(2, 32, 32, 128), rnd(128, 128) * 0.1
    shape = (2, 32, 32, 128)
    for run in (fwd_wide, bwd_wide):
        first = torch.full(shape, float("nan"), dtype=TDT[dt], device=cuda)
        run(first)
        assert not torch.isnan(first).any()
        o = torch.empty(2, 8, 8, 512, dtype=TDT[dt], device=cuda)
        L.conv_infer(C.byref(small), DT[dt], ptr(xs), ptr(ws_), ptr(bias), None, 0, ptr(o), 4, ptr(ws), ws.numel(),
                     stream())
        L.conv_infer_dgrad(C.byref(small), DT[dt], ptr(xs), ptr(ws_), None, None, ptr(o), 4, ptr(ws), ws.numel(),
                           stream())
        again = torch.full(shape, float("nan"), dtype=TDT[dt], device=cuda)
        run(again)
        assert not torch.isnan(again).any(), "stale output: the tickets held another launch's slab"
        assert torch.equal(first.view(BITS[dt]), again.view(BITS[dt]))


# ---- 4. avg-pool backward through the last ReLU -------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("hw", [6, 1])
def test_avgpool_bwd_relu(cuda, dt, hw):
    L = lib()
    gen = torch.Generator().manual_seed(40 + hw)
    n, c = 3, 2048
    dfeat = torch.randn(n, c, generator=gen).to(cuda)
    out = torch.randn(n, hw, c, generator=gen)
    out[torch.rand(n, hw, c, generator=gen) < 0.05] = 0.0
    out = out.to(TDT[dt]).to(cuda)
    dx = torch.full((n, hw, c), float("nan"), dtype=TDT[dt], device=cuda)
    L.avgpool_bwd_relu(DT[dt], n, hw, c, ptr(dfeat), ptr(out), ptr(dx), stream())
    ref = dfeat.double().cpu()[:, None, :] / hw * (out.double().cpu() > 0)
    got = dx.double().cpu()
    assert not torch.isnan(got).any()
    assert (got - ref).abs().max().item() <= TOL[dt] * ref.abs().max().item()
    assert torch.equal(got == 0, ref == 0)  # the mask exactly: > 0, zeros masked


# ---- 5 / 6 / 7. the session ---------------------------------------------------------------------------------
def _randomize_bn(model):
    """tests/test_gpu_infer.py's recipe: non-trivial BN parameters and running statistics from one generator."""
    g = torch.Generator().manual_seed(7)
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            c = m.num_features
            m.weight.data = 0.5 + torch.rand(c, generator=g)
            m.bias.data = 0.1 * torch.randn(c, generator=g)
            m.running_mean.data = 0.1 * torch.randn(c, generator=g)
            m.running_var.data = 0.5 + torch.rand(c, generator=g)


@pytest.fixture(scope="module")
def oracle():
    from oracle.ncamera import build_reference_model

    ref = build_reference_model(42)
    _randomize_bn(ref)
    return ref.eval()


def _images(hw, seed=1234, batch=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (batch, 6, *hw), generator=g, dtype=torch.uint8)


def _cotangent(batch=2):
    return torch.randn(batch, 6, generator=torch.Generator().manual_seed(99))


def _product(oracle, cuda, dtype):
    from argus_amd.models import NCameraCNN

    m = NCameraCNN(compute_dtype=dtype)
    m.load_state_dict(oracle.state_dict())
    return m.to(cuda).eval()


def _gelu_grad(x):
    return 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5


def _stage_references(s, dpred):
    """(role, bar kind, fp64 reference) of every backward launch of GradientSession ``s`` after a debug run, each
    derived from the GPU tensors the schedule says that launch reads: the previous launch's captured output, the
    stored forward activation, the folded weights (the forward copy) as stored."""
    dbg = {k: v.double().cpu() for k, v in s.debug.items()}
    f64 = lambda t: t.double().cpu()  # noqa: E731
    B, N, D, R = s.batch, s.N, s.n_cams * s.rdim, s.rdim
    hd = {k: f64(v) for k, v in s.head.items()}
    yield "head.dh2", "stage", (f64(dpred) @ hd["output_mlp.4", "weight"]) * _gelu_grad(f64(s.h2))
    yield "head.dh1", "stage", (dbg["head.dh2"] @ hd["output_mlp.2", "weight"]) * _gelu_grad(f64(s.h1))
    yield "head.dh0", "stage", (dbg["head.dh1"] @ hd["output_mlp.0", "weight"]) * _gelu_grad(f64(s.h0).view(B, D))
    yield "head.dfeat", "stage", dbg["head.dh0"].view(N, R) @ hd["resnet.fc", "weight"]
    last = f64(s.acts[-1][2])
    hf, wf = s.final_hw
    yield "bwd.avgpool", "stage", dbg["head.dfeat"][:, None, None, :] / (hf * wf) * (last > 0)
    w64 = lambda cv: f64(cv.wf).view(cv.desc.k, cv.desc.r, cv.desc.s, cv.desc.c).permute(0, 3, 1, 2).contiguous()  # noqa: E731
    dm3 = dbg["bwd.avgpool"]
    for i in range(len(s.schedule) - 1, -1, -1):
        c1, c2, c3, ds = s.schedule[i]
        a1, a2, _ = s.acts[i]
        h = s.acts[i - 1][2] if i else s.p0
        pf = c1.name[:-len(".conv1")]
        yield f"bwd.{pf}.conv3", "stage", _dx64(c3.desc, dm3, w64(c3)) * (f64(a2) > 0)
        yield f"bwd.{pf}.conv2", "stage", _dx64(c2.desc, dbg[f"bwd.{pf}.conv3"], w64(c2)) * (f64(a1) > 0)
        addend = dm3
        if ds is not None:
            yield f"bwd.{pf}.downsample", "stage", _dx64(ds.desc, dm3, w64(ds))
            addend = dbg[f"bwd.{pf}.downsample"]
        yield f"bwd.{pf}.conv1", "stage", (_dx64(c1.desc, dbg[f"bwd.{pf}.conv2"], w64(c1)) + addend) * (f64(h) > 0)
        dm3 = dbg[f"bwd.{pf}.conv1"]
    # max-pool backward from the stored argmax (index r*3 + t of the 3x3 / 2 window, offset -1), then the stem ReLU
    (H1, W1), (H2, W2) = s.stem_hw, s.pool_hw
    amax = s.amax.view(N, H2, W2, 64).cpu()
    dz = torch.zeros(N, H1 + 2, W1 + 2, 64, dtype=torch.float64)
    for r in range(3):
        for t in range(3):
            dz[:, r:r + 2 * H2:2, t:t + 2 * W2:2, :] += dm3 * (amax == r * 3 + t)
    y0, scale, shift = f64(s.y0), f64(s.stem_coef[0]), f64(s.stem_coef[1])
    yield "bwd.maxpool", "stage", dz[:, 1:1 + H1, 1:1 + W1, :] * (y0 * scale + shift > 0)
    # stem data gradient of scale * dm0, the eval-mode BatchNorm derivative
    wst = f64(s.stem_wf).view(64, 8, 8, 4)[:, :7, :7, :3].permute(0, 3, 1, 2).contiguous()
    H, W = s.hw
    dy0 = (dbg["bwd.maxpool"] * scale).permute(0, 3, 1, 2).contiguous()
    ref = torch.nn.grad.conv2d_input((N, 3, H, W), wst, dy0, stride=2, padding=3)
    yield "bwd.dx", "stem", ref.view(B, 3 * s.n_cams, H, W)


def _planned_kernels(dt, hw, directions, batch=2):
    """The frozen conv instantiations a session of this size launches, by the mirror of the tile-height rule."""
    return {conv_kernel_name(direction, dt, shape) for shape in session_convs(batch, hw).values()
            for direction in directions}


def _launched_kernels(timer):
    return {n for n in timer.summary() if is_frozen_conv(n)}


# 72x104: ragged 9x13, 5x7, 3x4; 128x128: the smallest session with 64-row tiles (forward 1x1 s1; backward 1x1 s1, s2)
SESSION_HW = [(64, 64), (72, 104), (128, 128)]
SESSION_IDS = ["64x64", "72x104", "128x128"]


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("hw", SESSION_HW, ids=SESSION_IDS)
def test_session_stage_by_stage(cuda, oracle, dt, hw):
    from argus_amd.infer_grad import GradientSession

    s = GradientSession(_product(oracle, cuda, dt), 2, hw, debug=True)
    assert s.graph is False and s.debug == {}
    x = (_images(hw).float() / 255.0).to(cuda)
    dpred = _cotangent().to(cuda)
    s.dx.fill_(float("nan"))
    with KernelTimer() as timer:
        g = s.vjp(x, dpred)
    launched = _launched_kernels(timer)
    assert launched == _planned_kernels(dt, hw, ("fwd", "dgrad")), launched
    rows64 = {n for n in launched if n.endswith(", 64>")}
    assert len(rows64) == (2 if hw == (128, 128) else 0), launched  # forward and data gradient, or neither
    assert g.shape == (2, 6, *hw) and g.dtype == torch.float32 and not torch.isnan(g).any()
    assert len(s.debug) == s.launches_per_backward == 4 + 1 + 52 + 2
    worst, seen = {"stage": (0.0, ""), "stem": (0.0, "")}, 0
    for role, kind, ref in _stage_references(s, dpred):
        got = s.debug[role].double().cpu()
        assert got.shape == ref.shape, (role, got.shape, ref.shape)
        assert ref.abs().max().item() > 0, role
        e = _rel_max(got, ref)
        bar = (STAGE if kind == "stage" else STEM)[dt]
        if e / bar > worst[kind][0]:
            worst[kind] = (e / bar, role)
        assert e <= bar, f"{role} {dt} {hw}: rel_max {e:.3e} > {bar:.1e}"
        seen += 1
    assert seen == len(s.debug)
    print(f"frozen gradient stages {dt} {hw}: worst rel_max / bar = {worst['stage'][0]:.3f} at {worst['stage'][1]}, "
          f"stem {worst['stem'][0]:.3f}")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("hw", [(72, 104), (128, 128)], ids=["72x104", "128x128"])
def test_session_forward_conv_by_conv(cuda, oracle, dt, hw):
    """The forward counterpart of test_session_stage_by_stage: every conv launch of a GradientSession forward against
    fp64 conv2d of the stored input with the stored folded weight, + bias, + the residual, through the ReLU, at the
    kernel bars of the parity test (2e-5 / 1.5e-2 of the reference's maximum magnitude). The inputs are the tensors
    the session keeps for its backward (p0, a1 / a2 / out of every block). The downsample output borrows a pool
    buffer that the next stride block overwrites, so it is captured here as the backward's _keep captures a
    gradient: a clone taken right after its launch, checked itself and then used as conv3's residual."""
    import torch.nn.functional as F

    from argus_amd.infer_grad import GradientSession

    s = GradientSession(_product(oracle, cuda, dt), 2, hw, debug=True)
    x = (_images(hw).float() / 255.0).to(cuda)
    yd = {}
    conv = s._conv

    def conv_and_keep(cv, xin, out, res, relu, st, probe=None):
        conv(cv, xin, out, res, relu, st, probe)
        if ".downsample." in cv.name:
            d = cv.desc
            yd[cv.name] = out[:d.n * d.ho * d.wo * d.k].view(d.n, d.ho, d.wo, d.k).clone()

    s._conv = conv_and_keep
    for acts in s.acts:
        for t in acts:
            t.fill_(float("nan"))
    with KernelTimer() as timer:
        s(x)
    launched = _launched_kernels(timer)
    assert launched == _planned_kernels(dt, hw, ("fwd",)), launched
    assert len({n for n in launched if n.endswith(", 64>")}) == (1 if hw == (128, 128) else 0), launched
    f64 = lambda t: t.double().cpu()  # noqa: E731

    def ref(cv, xin, res, relu):
        d = cv.desc
        w = f64(cv.wf).view(d.k, d.r, d.s, d.c).permute(0, 3, 1, 2)
        y = F.conv2d(xin.permute(0, 3, 1, 2), w, stride=d.stride, padding=d.pad).permute(0, 2, 3, 1) + f64(cv.bias)
        y = y if res is None else y + res
        return y.clamp_min(0) if relu else y

    worst, seen = (0.0, ""), 0
    h = f64(s.p0)
    for (c1, c2, c3, ds), (a1, a2, out) in zip(s.schedule, s.acts):
        a1, a2, out = f64(a1), f64(a2), f64(out)
        res = h
        checks = [(c1, a1, ref(c1, h, None, 1)), (c2, a2, ref(c2, a1, None, 1))]
        if ds is not None:
            res = f64(yd[ds.name])
            checks.append((ds, res, ref(ds, h, None, 0)))
        checks.append((c3, out, ref(c3, a2, res, 1)))
        for cv, got, want in checks:
            assert got.shape == want.shape, (cv.name, got.shape, want.shape)
            bound = TOL[dt] * want.abs().max().item()
            assert bound > 0, cv.name
            err = (got - want).abs().max().item()  # NaN (an unwritten element) fails the bound
            if err / bound > worst[0]:
                worst = (err / bound, cv.name)
            assert err <= bound, f"{cv.name} {dt} {hw}: {err:.3e} > {bound:.3e}"
            seen += 1
        h = out
    assert seen == len(s.convs) == 52 and len(yd) == 4
    print(f"frozen forward convs {dt} {hw}: worst error / bound = {worst[0]:.3f} at {worst[1]}")


@pytest.fixture(scope="module")
def oracle_grads(oracle):
    """hw -> (g64, d_ref): the oracle's eval-mode d<pred, cot>/d images under CPU autograd in double, and the
    distance of its bf16-autocast gradient from its fp32 gradient (computed once per size, shared, never modified)."""
    import copy

    cache = {}

    def get(hw):
        if hw not in cache:
            x, cot = _images(hw).float() / 255.0, _cotangent()

            def grad(model, xin, autocast=False):
                xin = xin.clone().requires_grad_(True)
                with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
                    pred = model(xin)
                (g,) = torch.autograd.grad((pred.to(xin.dtype) * cot.to(xin.dtype)).sum(), xin)
                return g.double()

            g64 = grad(copy.deepcopy(oracle).double().eval(), x.double())
            g32 = grad(oracle, x)
            g16 = grad(oracle, x, autocast=True)
            cache[hw] = (g64, ((g16 - g32).norm() / g32.norm()).item(), ((g32 - g64).norm() / g64.norm()).item())
        return cache[hw]

    return get


@pytest.mark.parametrize("hw", SESSION_HW, ids=SESSION_IDS)
def test_session_matches_the_fp64_oracle(cuda, oracle, oracle_grads, hw):
    """A gross-error check (the decisive ones are the kernel parity and the stages): a deep random ReLU net is
    chaotic in its masks, so the bar is the CPU reference's own bf16 distance, doubled as in
    test_gpu_infer.py::test_session_matches_the_fp64_oracle; 2 * d_ref < 1 keeps a zero or sign-flipped gradient out."""
    from argus_amd.infer_grad import GradientSession

    g64, d_ref, d32 = oracle_grads(hw)
    assert 2 * d_ref < 1
    x = (_images(hw).float() / 255.0).to(cuda)
    cot = _cotangent().to(cuda)
    for dt in ("fp32", "bf16"):
        g = GradientSession(_product(oracle, cuda, dt), 2, hw).vjp(x, cot).double().cpu()
        e = ((g - g64).norm() / g64.norm()).item()
        print(f"frozen gradient vs fp64 oracle {hw} {dt}: e = {e:.3e}, d_ref = {d_ref:.3f} (CPU fp32 reference: {d32:.1e})")
        assert e <= 2 * d_ref, (dt, hw, e, d_ref)


def test_session_semantics(cuda, oracle):
    from argus_amd.infer import InferenceSession
    from argus_amd.infer_grad import GradientSession
    from argus_amd.losses import geometric_loss_fn
    from argus_amd.utils import se3_exp

    hw = (64, 64)
    model = _product(oracle, cuda, "fp32")
    u8 = _images(hw, 1)
    xa, xb = (u8.float() / 255.0).to(cuda), (_images(hw, 2).float() / 255.0).to(cuda)  # the division on the CPU
    u8 = u8.to(cuda)
    target = se3_exp(0.3 * torch.randn(2, 6, generator=torch.Generator().manual_seed(3)).to(cuda))
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert all(p.grad is None for p in model.parameters())
    sg, se = GradientSession(model, 2, hw, graph=True), GradientSession(model, 2, hw, graph=False)
    # the prediction is InferenceSession's
    ya = InferenceSession(model, 2, hw)(xa)
    assert torch.equal(sg(xa), ya) and torch.equal(se(xa), ya)
    # image_gradient: the loss function's losses, the gradient of their mean
    sg.dx.fill_(float("nan"))
    losses, grad = sg.image_gradient(xa, target)
    assert losses.shape == (2,) and grad.shape == xa.shape and grad.dtype == torch.float32
    assert not torch.isnan(grad).any() and float(grad.abs().max()) > 0
    assert torch.equal(losses, geometric_loss_fn(sg(xa), target))
    dpred = sg.dpred.clone()
    assert torch.equal(grad, sg.vjp(xa, dpred)) and torch.equal(grad, se.vjp(xa, dpred))
    le, ge = se.image_gradient(xa, target)
    assert torch.equal(le, losses) and torch.equal(ge, grad)  # graph == eager
    lb, gb = sg.image_gradient(xb, target)
    assert not torch.equal(gb, grad)
    l2, g2 = sg.image_gradient(xa, target)
    assert torch.equal(l2, losses) and torch.equal(g2, grad)  # replays: no stale state, no ticket residue
    assert grad.data_ptr() != g2.data_ptr()  # fresh tensors
    lu, gu = sg.image_gradient(u8, target)
    assert torch.equal(lu, losses) and torch.equal(gu, grad)  # uint8 == its /255 float batch
    assert torch.equal(se.image_gradient(u8, target)[1], grad)
    # the session never writes the model, whatever its mode
    model.train()
    assert torch.equal(sg.image_gradient(xa, target)[1], grad)
    assert torch.equal(GradientSession(model, 2, hw, graph=False).image_gradient(xa, target)[1], grad)
    model.eval()
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before) and "resnet.bn1.num_batches_tracked" in before
    assert "resnet.layer4.2.bn3.running_var" in before and all(p.grad is None for p in model.parameters())
    # a snapshot: changed weights show after refresh(), in both folded copies
    with torch.no_grad():
        model.resnet.layer3[1].conv2.weight.mul_(1.25)
        model.resnet.layer1[0].downsample[1].running_var.mul_(0.5)
    assert torch.equal(sg.image_gradient(xa, target)[1], grad)
    sg.refresh()
    fresh = GradientSession(model, 2, hw, graph=False)
    lr, gr = sg.image_gradient(xa, target)
    lf, gf = fresh.image_gradient(xa, target)
    assert torch.equal(lr, lf) and torch.equal(gr, gf) and not torch.equal(gr, grad)
    # refusals
    for bad in (xa[:1], xa[:, :3], xa[..., :32]):
        with pytest.raises(ValueError, match="shape"):
            sg.vjp(bad, dpred)
        with pytest.raises(ValueError, match="shape"):
            sg.image_gradient(bad, target)
    with pytest.raises(ValueError, match="float32 or uint8"):
        sg.vjp(xa.double(), dpred)
    with pytest.raises(ValueError, match="dpred"):
        sg.vjp(xa, dpred[:1])
    with pytest.raises(ValueError, match="target"):
        sg.image_gradient(xa, target[:, :6])
    with pytest.raises(ValueError, match="'fp32' and 'bf16'"):
        GradientSession(model, 2, hw, compute_dtype="fp16")
    assert sg.saved_bytes > 0 and sg.launches_per_forward == 61
