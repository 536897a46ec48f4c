"""GPU, C ABI level: the bf16x3 split arithmetic of the fp32 conv GEMMs (policy key 53; igemm.h).

The bar, elementwise against fp64: |got - ref| <= 4 * 2^-16 * (|a| conv |b|) + 1e-30, where the second factor
is the same conv pass on absolute values. 3 * 2^-16 is the worst case of the three dropped terms (each
operand's residual after hi + lo is <= 2^-16 |x|, and lo*lo); the fp32 accumulation of the exact bf16
products adds <= 3.5e-7 = 0.02 * 2^-16 of the same sum. A single bf16 product (a missing cross term) is
12..115 * 2^-16 away and fails it.
"""
import ctypes as C
import functools
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

from argus_amd._lib import F32, ConvDesc, lib, ptr, stream  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 4 * 2.0 ** -16
KEY = 53
N = 2
# (cin, cout, k, stride, size): 64- and 128-row tiles with partial row tiles, stride-2 dgrad phases of
# unequal size, K from 64 to 4608, both weight-gradient tile shapes
SHAPES = [(64, 64, 1, 1, 12), (64, 256, 1, 1, 12), (64, 64, 3, 1, 12), (128, 128, 3, 2, 12), (256, 512, 1, 2, 12),
          (256, 256, 3, 2, 9), (2048, 512, 1, 1, 4), (512, 512, 3, 1, 4), (512, 2048, 1, 1, 4)]
INT_SHAPES = [(64, 64, 3, 1, 12), (2048, 512, 1, 1, 4), (128, 128, 3, 2, 12)]


def _desc(n, h, w, cin, cout, k, s, tune, stem=False):
    p = 3 if stem else (1 if k == 3 else 0)
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    return ConvDesc(n, h, w, cin, cout, k, k, s, p, ho, wo, int(stem)).with_tuning(tune), p


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def _merge_stats(part, tile, count):
    """Chan-merge per-tile {sum, M2} partials (rows, C, 2) -> per-channel (mean, biased variance)."""
    n = torch.tensor([min(tile, count - t * tile) for t in range(part.shape[0])], dtype=torch.float64)
    mean_t = part[..., 0] / n[:, None]
    mean = part[..., 0].sum(0) / count
    q = (part[..., 1] + part[..., 0] * mean_t).sum(0)
    return mean, q / count - mean * mean


def _within(got, ref, mag, what):
    err = (got.double().cpu() - ref).abs()
    worst = (err / (mag + 1e-300)).max().item()
    print(f"{what}: worst |err| / (|a| conv |b|) = {worst / 2.0 ** -16:.3f} * 2^-16")
    assert (err <= BAR * mag + 1e-30).all(), f"{what}: {worst / 2.0 ** -16:.2f} * 2^-16 > 4 * 2^-16"


@functools.lru_cache(maxsize=None)
def _case(shape, integers=False):
    """CPU inputs (fp32, NHWC / OHWI) and the fp64 references + magnitudes of the three passes (NCHW)."""
    cin, cout, k, s, hin = shape
    g = torch.Generator().manual_seed(cin + 3 * cout + 5 * k + 7 * s + hin + (1000 if integers else 0))
    p = 1 if k == 3 else 0
    ho = (hin + 2 * p - k) // s + 1
    if integers:
        x = torch.randint(-3, 4, (N, hin, hin, cin), generator=g).float()
        w = torch.randint(-2, 3, (cout, k, k, cin), generator=g).float()
        dy = torch.randint(-2, 3, (N, ho, ho, cout), generator=g).float()
        dx0 = torch.zeros(N, hin, hin, cin)
    else:
        x = torch.randn(N, hin, hin, cin, generator=g)
        w = torch.randn(cout, k, k, cin, generator=g) * (2.0 / (k * k * cin)) ** 0.5
        dy = torch.randn(N, ho, ho, cout, generator=g)
        dx0 = torch.randn(N, hin, hin, cin, generator=g)
    xr, wr, dyr = (t.double().permute(0, 3, 1, 2) for t in (x, w, dy))
    kw = dict(stride=s, padding=p)
    c = dict(x=x, w=w, dy=dy, dx0=dx0, p=p,
             fwd=F.conv2d(xr, wr, **kw), fwd_mag=F.conv2d(xr.abs(), wr.abs(), **kw),
             dgrad=torch.nn.grad.conv2d_input(xr.shape, wr, dyr, **kw) + dx0.double().permute(0, 3, 1, 2),
             dgrad_mag=torch.nn.grad.conv2d_input(xr.shape, wr.abs(), dyr.abs(), **kw),
             wgrad=torch.nn.grad.conv2d_weight(xr, wr.shape, dyr, **kw),
             wgrad_mag=torch.nn.grad.conv2d_weight(xr.abs(), wr.shape, dyr.abs(), **kw))
    return c


def _run(cuda, shape, key, integers=False, bm128=False):
    """The three passes of one shape with policy key 53 = key: (y, stats, tile, dx, dw) on the CPU.
    bm128: 128-row forward / data-gradient tiles (policy keys 0 / 1; these small GEMMs get 64 rows otherwise)."""
    L = lib()
    cin, cout, k, s, hin = shape
    c = _case(shape, integers)
    d, p = _desc(N, hin, hin, cin, cout, k, s, {KEY: key, **({0: 128, 1: 128} if bm128 else {})})
    xg, wg, dyg = c["x"].to(cuda), c["w"].to(cuda), c["dy"].to(cuda)
    wf = torch.empty(cout, k * k * cin, device=cuda)
    wt = torch.empty(cin, k * k * cout, device=cuda)
    L.conv_weight_prep(C.byref(d), F32, ptr(wg), None, ptr(wf), ptr(wt), stream())
    y = torch.empty(N, d.ho, d.wo, cout, device=cuda)
    rows = L.dll.argus_conv_fwd_stat_rows(C.byref(d), F32)
    tile = L.dll.argus_conv_fwd_stat_tile(C.byref(d), F32)
    stats = torch.empty(rows, cout, 2, device=cuda)
    L.conv_fwd(C.byref(d), F32, ptr(xg), ptr(wf), ptr(y), None, None, ptr(stats), stream())
    dx = c["dx0"].to(cuda)  # accumulate onto a non-zero buffer
    L.conv_dgrad(C.byref(d), F32, ptr(dyg), ptr(wt), ptr(dx), ptr(dx), None, stream())
    ws = torch.empty(L.dll.argus_conv_wgrad_workspace_bytes(C.byref(d), F32), dtype=torch.uint8, device=cuda)
    dw = torch.empty(cout, k, k, cin, device=cuda)
    L.conv_wgrad(C.byref(d), F32, ptr(xg), None, None, ptr(dyg), ptr(dw), ptr(ws), ws.numel(), stream())
    torch.cuda.synchronize()
    return (y.permute(0, 3, 1, 2).cpu(), stats.cpu(), tile, dx.permute(0, 3, 1, 2).cpu(), dw.permute(0, 3, 1, 2).cpu())


_run_cached = functools.lru_cache(maxsize=None)(_run)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_split_bound_per_pass(cuda, shape):
    cin, cout, k, s, hin = shape
    c = _case(shape)
    y, stats, tile, dx, dw = _run_cached(cuda, shape, 7)
    _within(y, c["fwd"], c["fwd_mag"], f"fwd {shape}")
    _within(dx, c["dgrad"], c["dgrad_mag"], f"dgrad {shape}")
    _within(dw, c["wgrad"], c["wgrad_mag"], f"wgrad {shape}")
    # the BN statistics partials describe the stored fp32 y (as test_conv_fwd_dgrad_wgrad_all_shapes asks of fp32)
    yr = y.double().permute(0, 2, 3, 1).reshape(-1, cout)
    mean, var = _merge_stats(stats.double(), tile, yr.shape[0])
    assert _rel(mean, yr.mean(0)) < 1e-4 or (mean - yr.mean(0)).abs().max() < 1e-5 * yr.std(0).max()
    assert _rel(var, yr.var(0, unbiased=False)) < 1e-5
    # key 53 = 0: the exact path, at its existing bar, and not the same bits
    y0, stats0, _, dx0, dw0 = _run_cached(cuda, shape, 0)
    for got, ref, got7, what in ((y0, c["fwd"], y, "fwd"), (dx0, c["dgrad"], dx, "dgrad"), (dw0, c["wgrad"], dw, "wgrad")):
        assert _rel(got, ref) < 2e-5, (what, shape)
        assert not torch.equal(got, got7), f"{what} {shape}: key 53 = 7 gave the exact path's bits"


@pytest.mark.parametrize("shape", [(64, 256, 1, 1, 12), (64, 64, 3, 1, 12), (256, 256, 3, 2, 9), (512, 512, 3, 1, 4)],
                         ids=lambda s: "x".join(map(str, s)))
def test_split_bound_128_row_tiles(cuda, shape):
    """Forward and data gradient on 128-row tiles (one partial tile, or one tile per stride-2 phase), whose
    lo*hi products run in a second pass: the same bar, and exact on integer operands."""
    c = _case(shape)
    y, stats, tile, dx, _ = _run(cuda, shape, 7, bm128=True)
    assert tile == 128
    _within(y, c["fwd"], c["fwd_mag"], f"fwd 128-row {shape}")
    _within(dx, c["dgrad"], c["dgrad_mag"], f"dgrad 128-row {shape}")
    yr = y.double().permute(0, 2, 3, 1).reshape(-1, shape[1])
    mean, var = _merge_stats(stats.double(), tile, yr.shape[0])
    assert _rel(mean, yr.mean(0)) < 1e-4 or (mean - yr.mean(0)).abs().max() < 1e-5 * yr.std(0).max()
    assert _rel(var, yr.var(0, unbiased=False)) < 1e-5
    y0, _, _, dx0, _ = _run(cuda, shape, 0, bm128=True)
    assert not torch.equal(y, y0) and not torch.equal(dx, dx0)
    ci = _case(shape, True)
    yi, _, _, dxi, _ = _run(cuda, shape, 7, True, bm128=True)
    assert torch.equal(yi.double(), ci["fwd"]) and torch.equal(dxi.double(), ci["dgrad"])


def test_split_bound_stem(cuda):
    """The stem, 3 -> 64 7x7/2 on 2 x 30 x 30 NHWC4 input: forward (+ statistics) and weight gradient."""
    L = lib()
    H = 30
    g = torch.Generator().manual_seed(3)
    img = torch.rand(N, 3, H, H, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1  # OIHW master
    outs = {}
    for key in (7, 0):
        d, _ = _desc(N, H, H, 3, 64, 7, 2, {KEY: key}, stem=True)
        dy = torch.randn(N, d.ho, d.wo, 64, generator=torch.Generator().manual_seed(4))
        x4 = torch.empty(N, H, H, 4, device=cuda)
        imgg, wg, dyg = img.to(cuda), w.to(cuda), dy.to(cuda)
        L.images_to_nhwc4(F32, N, H, H, ptr(imgg), ptr(x4), stream())
        wf = torch.empty(64, 256, device=cuda)
        L.conv_weight_prep(C.byref(d), F32, ptr(wg), (C.c_int64 * 4)(*wg.stride()), ptr(wf), None, stream())
        y = torch.empty(N, d.ho, d.wo, 64, device=cuda)
        rows = L.dll.argus_conv_fwd_stat_rows(C.byref(d), F32)
        tile = L.dll.argus_conv_fwd_stat_tile(C.byref(d), F32)
        stats = torch.empty(rows, 64, 2, device=cuda)
        L.conv_fwd(C.byref(d), F32, ptr(x4), ptr(wf), ptr(y), None, None, ptr(stats), stream())
        ws = torch.empty(L.dll.argus_conv_wgrad_workspace_bytes(C.byref(d), F32), dtype=torch.uint8, device=cuda)
        dw = torch.empty(64, 7, 7, 3, device=cuda)
        L.conv_wgrad(C.byref(d), F32, ptr(x4), None, None, ptr(dyg), ptr(dw), ptr(ws), ws.numel(), stream())
        torch.cuda.synchronize()
        outs[key] = (y.permute(0, 3, 1, 2).cpu(), dw.permute(0, 3, 1, 2).cpu(), stats.cpu(), tile)
    xr, wr, dyr = img.double(), w.double(), dy.double().permute(0, 3, 1, 2)
    ref = F.conv2d(xr, wr, stride=2, padding=3)
    refw = torch.nn.grad.conv2d_weight(xr, wr.shape, dyr, stride=2, padding=3)
    y, dw, stats, tile = outs[7]
    _within(y, ref, F.conv2d(xr, wr.abs(), stride=2, padding=3), "stem fwd")
    _within(dw, refw, torch.nn.grad.conv2d_weight(xr, wr.shape, dyr.abs(), stride=2, padding=3), "stem wgrad")
    yr = y.double().permute(0, 2, 3, 1).reshape(-1, 64)
    mean, var = _merge_stats(stats.double(), tile, yr.shape[0])
    assert _rel(mean, yr.mean(0)) < 1e-4 or (mean - yr.mean(0)).abs().max() < 1e-5 * yr.std(0).max()
    assert _rel(var, yr.var(0, unbiased=False)) < 1e-5
    y0, dw0, _, _ = outs[0]
    assert _rel(y0, ref) < 2e-5 and _rel(dw0, refw) < 2e-5
    assert not torch.equal(y0, y) and not torch.equal(dw0, dw)


@pytest.mark.parametrize("shape", INT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_inputs_are_exact(cuda, shape):
    """Small-integer operands: every partial sum is an exact fp32 integer (< 2^24), so the split path must
    give the fp64 result bit for bit, as the exact path does: any k-mapping, LDS-layout or swizzle mismatch
    between the two operands shows with zero tolerance."""
    c = _case(shape, True)
    y, _, _, dx, dw = _run(cuda, shape, 7, True)
    y0, _, _, dx0, dw0 = _run(cuda, shape, 0, True)
    assert max(c["fwd_mag"].max(), c["dgrad_mag"].max(), c["wgrad_mag"].max()) < 2 ** 24
    for got, got0, ref, what in ((y, y0, c["fwd"], "fwd"), (dx, dx0, c["dgrad"], "dgrad"), (dw, dw0, c["wgrad"], "wgrad")):
        assert torch.equal(got.double(), ref), f"{what} {shape}: {(got.double() - ref).abs().max().item()}"
        assert torch.equal(got, got0), (what, shape)


@pytest.mark.parametrize("shape", [(64, 64, 3, 1, 10), (256, 64, 1, 1, 6)], ids=lambda s: "x".join(map(str, s)))
def test_bn_relu_prologue_is_applied_before_the_split(cuda, shape):
    """Forward and weight gradient with the BN+ReLU prologue: the bar against fp64 of relu(x*sc+sh) (the
    split follows the prologue; the padding of the 3x3 stays zero, not relu(shift))."""
    L = lib()
    cin, cout, k, s, hin = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, hin, hin, cin, generator=g)
    sc, sh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.5
    w = torch.randn(cout, k, k, cin, generator=g) * 0.05
    d, p = _desc(N, hin, hin, cin, cout, k, s, {KEY: 7})
    dy = torch.randn(N, d.ho, d.wo, cout, generator=g)
    xg, wg, dyg, scg, shg = (t.to(cuda) for t in (x, w, dy, sc, sh))
    wf = torch.empty(cout, k * k * cin, device=cuda)
    wt = torch.empty(cin, k * k * cout, device=cuda)
    L.conv_weight_prep(C.byref(d), F32, ptr(wg), None, ptr(wf), ptr(wt), stream())
    y = torch.empty(N, d.ho, d.wo, cout, device=cuda)
    L.conv_fwd(C.byref(d), F32, ptr(xg), ptr(wf), ptr(y), ptr(scg), ptr(shg), None, stream())
    ws = torch.empty(L.dll.argus_conv_wgrad_workspace_bytes(C.byref(d), F32), dtype=torch.uint8, device=cuda)
    dw = torch.empty(cout, k, k, cin, device=cuda)
    L.conv_wgrad(C.byref(d), F32, ptr(xg), ptr(scg), ptr(shg), ptr(dyg), ptr(dw), ptr(ws), ws.numel(), stream())
    torch.cuda.synchronize()
    xa = torch.relu(x.double() * sc.double() + sh.double()).permute(0, 3, 1, 2)
    wr, dyr = w.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2)
    _within(y.permute(0, 3, 1, 2), F.conv2d(xa, wr, stride=s, padding=p), F.conv2d(xa, wr.abs(), stride=s, padding=p),
            f"prologue fwd {shape}")
    _within(dw.permute(0, 3, 1, 2), torch.nn.grad.conv2d_weight(xa, wr.shape, dyr, stride=s, padding=p),
            torch.nn.grad.conv2d_weight(xa, wr.shape, dyr.abs(), stride=s, padding=p), f"prologue wgrad {shape}")


def test_dgrad_bn_mask_bits_epilogue(cuda):
    """argus_conv_dgrad_bn, mask-bits epilogue, on (256, 64, 1, 1, 8): dm within the bar and the
    {sum dm, sum dm*xhat} partials consistent with the stored dm (as test_conv_dgrad_bn_epilogue checks)."""
    from argus_amd._lib import BnBwdEpilogue

    L = lib()
    cin, cout, k, s, hin = 256, 64, 1, 1, 8
    g = torch.Generator().manual_seed(5)
    d, p = _desc(N, hin, hin, cin, cout, k, s, {KEY: 7})
    w = torch.randn(cout, k, k, cin, generator=g) * (2.0 / cin) ** 0.5
    dy = torch.randn(N, d.ho, d.wo, cout, generator=g)
    y = torch.randn(N, hin, hin, cin, generator=g) * 2 + 0.3
    mean, invstd = torch.randn(cin, generator=g) * 0.1 + 0.3, torch.rand(cin, generator=g) + 0.5
    bits = torch.randint(0, 256, (N * hin * hin * cin // 4,), generator=g, dtype=torch.uint8)
    wg, dyg, yg, meang, invstdg, bitsg = (t.to(cuda) for t in (w, dy, y, mean, invstd, bits))
    wf = torch.empty(cout, k * k * cin, device=cuda)
    wt = torch.empty(cin, k * k * cout, device=cuda)
    L.conv_weight_prep(C.byref(d), F32, ptr(wg), None, ptr(wf), ptr(wt), stream())
    rows = L.dll.argus_conv_dgrad_bn_rows(C.byref(d), F32)
    part = torch.full((rows, cin, 2), float("nan"), device=cuda)
    dm = torch.empty(N, hin, hin, cin, device=cuda)
    e = BnBwdEpilogue()
    e.y, e.mean, e.invstd, e.mask_mode, e.part, e.mask_bits = ptr(yg), ptr(meang), ptr(invstdg), 3, ptr(part), ptr(bitsg)
    L.conv_dgrad_bn(C.byref(d), F32, ptr(dyg), ptr(wt), ptr(dm), None, C.byref(e), None, stream())
    torch.cuda.synchronize()
    wr, dyr = w.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2)
    v = torch.nn.grad.conv2d_input((N, cin, hin, hin), wr, dyr).permute(0, 2, 3, 1)
    mag = torch.nn.grad.conv2d_input((N, cin, hin, hin), wr.abs(), dyr.abs()).permute(0, 2, 3, 1)
    mask = ((bits.long().repeat_interleave(4).reshape(N, hin, hin, cin) >> (torch.arange(cin) % 4)) & 1).bool()
    got = dm.double().cpu()
    assert (got[~mask] == 0).all()
    _within(got, v * mask, mag * mask, "dgrad_bn dm")
    xh = (y.double() - mean.double()) * invstd.double()
    S, T_ = got.sum((0, 1, 2)), (got * xh).sum((0, 1, 2))
    pc = part.double().cpu().sum(0)
    scale = got.abs().sum((0, 1, 2)).max()
    assert (pc[:, 0] - S).abs().max() <= 1e-5 * scale and (pc[:, 1] - T_).abs().max() <= 4e-5 * scale


def test_pass_bits_select_passes(cuda):
    """Key 53 = 1 / 2 / 4: only the forward / data gradient / weight gradient leaves the exact path (the
    other two passes bit-identical to key 53 = 0), and the split pass is the f32x3 kernel instantiation."""
    from argus_amd.profiling import KernelTimer

    shape = (64, 256, 1, 1, 12)
    base = _run_cached(cuda, shape, 0)
    all3 = _run_cached(cuda, shape, 7)
    for bit, idx in ((1, 0), (2, 3), (4, 4)):
        with KernelTimer() as kt:
            out = _run(cuda, shape, bit)
        names = list(kt.summary())
        want = "argus::wgrad_kernel<argus::f32x3" if bit == 4 else "argus::igemm_kernel<argus::f32x3"
        assert sum(nm.startswith(want) for nm in names) == 1, names
        assert sum("f32x3" in nm for nm in names) == 1, names
        for i in (0, 3, 4):
            if i == idx:
                assert torch.equal(out[i], all3[i]) and not torch.equal(out[i], base[i]), (bit, i)
            else:
                assert torch.equal(out[i], base[i]), (bit, i)
        assert torch.equal(out[1], all3[1] if bit == 1 else base[1])  # the statistics follow the forward


def test_two_calls_give_identical_bits(cuda):
    for shape in [(128, 128, 3, 2, 12), (512, 2048, 1, 1, 4)]:
        a, b = _run(cuda, shape, 7), _run(cuda, shape, 7)
        for i in (0, 1, 3, 4):
            assert torch.equal(a[i], b[i]), (shape, i)


def test_key_is_ignored_for_bf16(cuda):
    """ARGUS_BF16 calls ignore key 53: identical bits with and without it."""
    from argus_amd._lib import BF16

    L = lib()
    cin, cout, k, s, hin = 64, 64, 3, 1, 12
    c = _case((cin, cout, k, s, hin))
    outs = []
    for key in (0, 7):
        d, _ = _desc(N, hin, hin, cin, cout, k, s, {KEY: key})
        xg, wg = c["x"].to(cuda, torch.bfloat16), c["w"].to(cuda)
        wf = torch.empty(cout, k * k * cin, device=cuda, dtype=torch.bfloat16)
        wt = torch.empty(cin, k * k * cout, device=cuda, dtype=torch.bfloat16)
        L.conv_weight_prep(C.byref(d), BF16, ptr(wg), None, ptr(wf), ptr(wt), stream())
        y = torch.empty(N, d.ho, d.wo, cout, device=cuda, dtype=torch.bfloat16)
        L.conv_fwd(C.byref(d), BF16, ptr(xg), ptr(wf), ptr(y), None, None, None, stream())
        torch.cuda.synchronize()
        outs.append(y.cpu())
    assert torch.equal(outs[0], outs[1])
