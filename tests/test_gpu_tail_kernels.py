"""The fp32 tail of the training step at its edge regimes, kernel by kernel through the C ABI:
csrc/loss.hip (pose loss, SE(3) Exp), csrc/head.hip (head GEMM, column sum, GELU) and csrc/optim.hip
(global norm, Adam). References are fp64 on the CPU; the pose-loss oracle is itself pinned to the
matrix-exponential / matrix-logarithm definition by tests/test_oracle.py on the same inputs
(tests/se3_cases.py). Every output buffer is pre-filled with NaN, so an element a kernel does not write
cannot pass on what the allocator left there.
"""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from argus_amd._lib import lib, ptr, stream
from oracle import se3
from tests import se3_cases

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _rel(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _nan(cuda, *shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=cuda)


def _f32(x: float) -> float:
    """x as the kernel receives it through a C float argument."""
    return torch.tensor(x, dtype=torch.float32).item()


# ----------------------------------------------------------------------------------------------------
# pose loss
# ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle(name):
    """fp64 oracle per-sample losses and d loss_b / d pred_b of a regime (computed once)."""
    return se3.loss_and_grad(*se3_cases.regimes()[name], mean=False)


def _se3_loss(cuda, pred, T, gscale, with_grad=True):
    B = pred.shape[0]
    loss = _nan(cuda, B + 1)  # one spare element each: must stay NaN
    dpred = _nan(cuda, B + 1, 6) if with_grad else None
    pg, tg = pred.to(cuda), T.to(cuda)
    lib().se3_loss(B, ptr(pg), ptr(tg), ptr(loss), ptr(dpred), C.c_float(gscale), stream())
    loss = loss.cpu()
    assert torch.isnan(loss[B]) and torch.isfinite(loss[:B]).all()
    if with_grad:
        dpred = dpred.cpu()
        assert torch.isnan(dpred[B]).all() and torch.isfinite(dpred[:B]).all()
        return loss[:B], dpred[:B]
    return loss[:B], None


def _check_loss(name, loss, dpred, gscale):
    """Per sample: 2^-22 of the sample's own |loss| / |grad|_inf (the kernel's one fp32 output rounding,
    2^-24, with 4x margin for the device libm) plus the regime's fp64 cancellation floor
    (se3_cases.BARS, measured oracle-against-definition)."""
    bar = se3_cases.BARS[name]
    ref_l, ref_g = _oracle(name)
    err_l = (loss.double() - ref_l).abs()
    bar_l = 2.0**-22 * ref_l.abs() + bar["a_loss"]
    assert (err_l <= bar_l).all(), (name, "loss", err_l.tolist(), bar_l.tolist())
    if dpred is not None:
        ref_g = ref_g * gscale
        err_g = (dpred.double() - ref_g).abs().amax(-1)
        bar_g = 2.0**-22 * ref_g.abs().amax(-1) + bar["a_grad"] * gscale
        assert (err_g <= bar_g).all(), (name, "grad", gscale, err_g.tolist(), bar_g.tolist())


@pytest.mark.parametrize("name", list(se3_cases.regimes()))
def test_se3_loss_regimes(cuda, name):
    pred, T = se3_cases.regimes()[name]
    B = pred.shape[0]
    loss, dpred = _se3_loss(cuda, pred, T, 1.0)
    _check_loss(name, loss, dpred, 1.0)
    gs = _f32(1.0 / B)
    loss_s, dpred_s = _se3_loss(cuda, pred, T, gs)
    assert torch.equal(loss_s, loss)  # grad_scale touches the gradient only
    _check_loss(name, loss_s, dpred_s, gs)
    loss_n, _ = _se3_loss(cuda, pred, T, 1.0, with_grad=False)  # dpred = NULL
    assert torch.equal(loss_n, loss)


def test_se3_loss_mixed_batch_bit_identical(cuda):
    """All regimes in one launch: a batch that is no multiple of a block's 256 / 6 samples, samples of
    every branch side by side in one wave. A sample's result depends on nothing but the sample."""
    R = se3_cases.regimes()
    pred = torch.cat([p for p, _ in R.values()])
    T = torch.cat([t for _, t in R.values()])
    assert pred.shape[0] * 6 > 256 and (pred.shape[0] * 6) % 256 != 0
    loss, dpred = _se3_loss(cuda, pred, T, 1.0)
    at = 0
    for name, (p, t) in R.items():
        l1, g1 = _se3_loss(cuda, p, t, 1.0)
        assert torch.equal(loss[at:at + len(p)], l1) and torch.equal(dpred[at:at + len(p)], g1), name
        at += len(p)


@pytest.mark.parametrize("B", [1, 63, 65])
def test_se3_exp_kernel(cuda, B):
    """argus_se3_exp against the oracle's Exp (pinned to the matrix exponential in tests/test_oracle.py):
    absolute 2^-22 * max(1, |t|_inf) per sample (one fp32 output rounding with 4x margin; |q| <= 1)."""
    pool = torch.cat([se3_cases.regimes()[n][0] for n in ("pred_beyond_pi", "pred_small_angle", "generic")])
    xi = pool.repeat((B + len(pool) - 1) // len(pool), 1)[:B].contiguous()
    ref = se3.se3_exp(xi.double())
    xg = xi.to(cuda)
    outs = []
    for canon in (0, 1):
        out = _nan(cuda, B + 1, 7)
        lib().se3_exp(B, ptr(xg), ptr(out), canon, stream())
        out = out.cpu()
        assert torch.isnan(out[B]).all() and torch.isfinite(out[:B]).all()
        outs.append(out[:B])
    raw, can = outs
    bar = 2.0**-22 * ref[:, :3].abs().amax(-1).clamp_min(1.0)
    assert ((raw.double() - ref).abs().amax(-1) <= bar).all()
    # canonical_w: every w >= 0; a rotation angle in (pi, 3 pi) has cos(theta / 2) < 0, so q is negated
    # exactly there and nothing else changes
    theta = xi[:, 3:].double().norm(dim=-1)
    assert theta.max() < 3 * math.pi
    flip = theta > math.pi
    if B >= 12:
        assert flip.any() and (~flip).any()
    assert (can[:, 6] >= 0).all()
    assert (raw[flip, 6] < 0).all() and (raw[~flip, 6] > 0).all()
    assert torch.equal(can[:, :3], raw[:, :3])
    assert torch.equal(can[flip, 3:], -raw[flip, 3:]) and torch.equal(can[~flip, 3:], raw[~flip, 3:])


# ----------------------------------------------------------------------------------------------------
# head GEMM
# ----------------------------------------------------------------------------------------------------

def _padded(cuda, t, ld):
    """Device copy of the 2-D tensor t with leading dimension ld; the padding is NaN."""
    buf = _nan(cuda, t.shape[0], ld)
    buf[:, :t.shape[1]] = t.to(cuda)
    return buf


def _splits(m, n, k):
    """K-slices argus_gemm_f32 takes when it is given the workspace it asks for."""
    b = lib().dll.argus_gemm_f32_workspace_bytes(m, n, k)
    assert b % (m * n * 4) == 0
    return max(1, b // (m * n * 4))


def _gemm(cuda, m, n, k, a, ta, b, tb, epi, use_ws, bias=None, aux=None, c0=None, pad=(0, 0, 0)):
    """One argus_gemm_f32 call on CPU operands a (m x k, or k x m if ta) and b (k x n, or n x k if tb);
    returns (C, aux) as (m, n) CPU tensors after checking that the padding columns are still NaN."""
    lda, ldb, ldc = a.shape[1] + pad[0], b.shape[1] + pad[1], n + pad[2]
    ag, bg = _padded(cuda, a, lda), _padded(cuda, b, ldb)
    cg = _nan(cuda, m, ldc)
    if c0 is not None:
        cg[:, :n] = c0.to(cuda)
    auxg = None
    if epi == 2:
        auxg = _nan(cuda, m, ldc)
    elif epi == 3:
        auxg = _padded(cuda, aux, ldc)
    biasg = None if bias is None else bias.to(cuda)
    ws, ws_bytes = None, 0
    if use_ws:
        ws_bytes = max(16, lib().dll.argus_gemm_f32_workspace_bytes(m, n, k))
        ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=cuda)  # NaN bit patterns
    lib().gemm_f32(m, n, k, ptr(ag), lda, ta, ptr(bg), ldb, tb, ptr(cg), ldc, ptr(biasg), epi, ptr(auxg), ptr(ws),
                   ws_bytes, stream())
    cg = cg.cpu()
    assert torch.isnan(cg[:, n:]).all() and torch.isfinite(cg[:, :n]).all()
    if auxg is not None:
        auxg = auxg.cpu()
        assert torch.isnan(auxg[:, n:]).all() and torch.isfinite(auxg[:, :n]).all()
        auxg = auxg[:, :n].contiguous()
    return cg[:, :n].contiguous(), auxg


def _gemm_epilogues(cuda, m, n, k, ta, tb, epis, pad=(0, 0, 0), seed=0):
    """Every epilogue of `epis` at one shape and layout against fp64, with the split-K workspace and
    with workspace = NULL (the unsplit path). Bar: 1e-5 max-relative on C and on aux."""
    g = torch.Generator().manual_seed(1000 + seed)
    a = torch.randn((k, m) if ta else (m, k), generator=g)
    b = torch.randn((n, k) if tb else (k, n), generator=g)
    bias = torch.randn(n, generator=g)
    c0 = torch.randn(m, n, generator=g)
    ab = (a.double().T if ta else a.double()) @ (b.double().T if tb else b.double())
    pre = ab + bias.double()
    pre_t = pre.clone().requires_grad_(True)
    F.gelu(pre_t).backward(ab)  # epilogue 3 with the same operands: (A @ B) * gelu'(aux)
    want = {0: ab, 1: pre, 2: F.gelu(pre), 3: pre_t.grad, 4: c0.double() + ab}
    for use_ws in (True, False):
        aux = None
        for epi in sorted(set(epis) | ({2} if 3 in epis else set())):
            tag = (m, n, k, ta, tb, epi, use_ws, pad)
            c, aux_out = _gemm(cuda, m, n, k, a, ta, b, tb, epi, use_ws, bias=bias if epi in (1, 2) else None,
                               aux=aux, c0=c0 if epi == 4 else None, pad=pad)
            assert _rel(c, want[epi]) < 1e-5, tag
            if epi == 2:
                aux = aux_out  # what the kernel stored feeds the epilogue-3 call, as in the head's backward
                assert _rel(aux, pre) < 1e-5, tag
            if epi == 3:
                assert torch.equal(aux_out, aux), tag  # epilogue 3 only reads aux


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_f32_slice_ends_mid_ktile(cuda, ta, tb):
    # 2 slices of kc = 160: the second covers k in [160, 300) and ends 12 into its last K-tile
    assert _splits(9, 33, 300) == 2
    _gemm_epilogues(cuda, 9, 33, 300, ta, tb, (0, 1, 2, 3, 4), seed=1 + 2 * ta + tb)


def test_gemm_f32_empty_last_slice(cuda):
    # 8 slices of kc = 160 (130 rounded up to the K-tile): slice 6 ends at k = 1040 and slice 7 is empty
    assert _splits(9, 33, 1040) == 8
    _gemm_epilogues(cuda, 9, 33, 1040, 0, 0, (0, 1, 2, 4), seed=5)


@pytest.mark.parametrize("m,n,k,ta,tb,epis,splits", [
    (64, 128, 2048, 0, 1, (1, 2), 16),    # output_mlp.0 at B = 64: bias, aux and GELU in the reduce kernel
    (128, 1024, 2048, 0, 1, (1,), 16),    # fc at B = 64 (both camera views)
    (6, 128, 512, 1, 0, (0,), 4),         # output_mlp.4 weight gradient at B = 512
    (70, 6, 128, 0, 0, (1, 3), 1),        # unsplit, narrow N
])
def test_gemm_f32_head_shapes(cuda, m, n, k, ta, tb, epis, splits):
    assert _splits(m, n, k) == splits
    _gemm_epilogues(cuda, m, n, k, ta, tb, epis, seed=10 + m)


def test_gemm_f32_padded_leading_dimensions(cuda):
    # lda = ldb = k + 5, ldc = n + 7 (aux shares ldc); the padding is NaN on the way in and must be NaN after
    _gemm_epilogues(cuda, 9, 33, 300, 0, 1, (2, 3), pad=(5, 5, 7), seed=20)


@pytest.mark.parametrize("m,n,ld", [(1, 6, 6), (7, 128, 128), (64, 6, 6), (513, 130, 137)])
def test_colsum_f32(cuda, m, n, ld):
    g = torch.Generator().manual_seed(30 + m)
    x = torch.randn(m, n, generator=g)
    xg = _padded(cuda, x, ld)
    before = xg.clone()
    out = _nan(cuda, n + 5)
    lib().colsum_f32(m, n, ptr(xg), ld, ptr(out), stream())
    out = out.cpu()
    assert torch.isnan(out[n:]).all()
    assert _rel(out[:n], x.double().sum(0)) < 1e-6
    assert torch.equal(xg.view(torch.int32), before.view(torch.int32))  # input and its padding untouched


# ----------------------------------------------------------------------------------------------------
# GELU
# ----------------------------------------------------------------------------------------------------

GELU_COUNTS = [1, 255, 257, 4096 * 256 + 3]  # the last is past the 4096-block grid cap
_GELU_SPECIAL = [0.0, 1e-30, -1e-30, 6.0, -6.0, 40.0, -40.0]

# Worst |err| / max(1, |x|) of torch's own fp32 CPU F.gelu against fp64, and worst
# |err| / (max(1, |x|) * max(1, |dy|)) of its fp32 autograd derivative, measured with gelu_errors on
# gelu_inputs(4096 * 256 + 3) (torch CPU, the development machine): 3.41e-7 and 2.61e-7 (at 255 / 257
# points: 1.9e-7 and 1.6e-7). The kernels get 4x.
GELU_FWD_MEASURED = 3.41e-7
GELU_BWD_MEASURED = 2.61e-7


def gelu_inputs(count):
    """(x, dy) fp32: the special points, then a grid over [-12, 12]; dy ~ N(0, 1)."""
    sp = torch.tensor(_GELU_SPECIAL)[:count]
    x = torch.cat([sp, torch.linspace(-12.0, 12.0, count - len(sp))]) if count > len(sp) else sp
    dy = torch.randn(count, generator=torch.Generator().manual_seed(40))
    return x.float().contiguous(), dy


def gelu_errors(x, dy, y, dx):
    """The two per-element error measures of an fp32 (y, dx) against fp64 on (x, dy)."""
    x64 = x.double().requires_grad_(True)
    y64 = F.gelu(x64)
    y64.backward(dy.double())
    scale = x.double().abs().clamp_min(1.0)
    e_fwd = ((y.double() - y64.detach()).abs() / scale).max().item()
    e_bwd = ((dx.double() - x64.grad).abs() / (scale * dy.double().abs().clamp_min(1.0))).max().item()
    return e_fwd, e_bwd


@pytest.mark.parametrize("count", GELU_COUNTS)
def test_gelu_f32_and_bwd(cuda, count):
    x, dy = gelu_inputs(count)
    xg, dyg = x.to(cuda), dy.to(cuda)
    y, dx = _nan(cuda, count + 1), _nan(cuda, count + 1)
    lib().gelu_f32(count, ptr(xg), ptr(y), stream())
    lib().gelu_bwd_f32(count, ptr(xg), ptr(dyg), ptr(dx), stream())
    y, dx = y.cpu(), dx.cpu()
    assert torch.isnan(y[count]) and torch.isnan(dx[count])
    assert torch.isfinite(y[:count]).all() and torch.isfinite(dx[:count]).all()
    e_fwd, e_bwd = gelu_errors(x, dy, y[:count], dx[:count])
    assert e_fwd <= 4 * GELU_FWD_MEASURED, (count, e_fwd)
    assert e_bwd <= 4 * GELU_BWD_MEASURED, (count, e_bwd)


# ----------------------------------------------------------------------------------------------------
# optimizer
# ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,spread", [(1, False), (3, False), (4, False), (5, False), (1027, False), (1027, True),
                                      (3 * 2**20 + 7, False)])
def test_global_norm(cuda, n, spread):
    """Counts below one f32x4, a scalar tail, and 3 * 2^20 + 7: three sweeps of sumsq_kernel's
    1024 x 256 x 4-element grid plus the tail. Bar 1e-6 relative to the fp64 norm."""
    g = torch.Generator().manual_seed(50 + n % 97)
    x = torch.randn(n, generator=g)
    if spread:  # magnitudes from 1e-3 to 1e3
        x = x.sign() * 10.0 ** (torch.rand(n, generator=g) * 6 - 3)
        assert x.abs().min() < 2e-3 and x.abs().max() > 5e2
    L = lib()
    ws = torch.full((L.dll.argus_sumsq_workspace_bytes(n),), 0xFF, dtype=torch.uint8, device=cuda)
    xg = x.to(cuda)
    out = _nan(cuda, 2)
    L.global_norm(n, ptr(xg), ptr(out), ptr(ws), stream())
    out = out.cpu()
    ref = x.double().norm().item()
    assert torch.isnan(out[1]) and abs(out[0].item() - ref) <= 1e-6 * ref


BIG_ADAM = 4096 * 1024 + 1027  # past adam_kernel's 4096 x 256 x 4-element grid: the grid-stride loop, plus the tail


@pytest.mark.parametrize("n,wd,gscale,gnorm,use_norm", [
    (1027, 0.1, 1.0, 40.0, True),     # weight decay, clipping active
    (1027, 0.0, 0.25, 40.0, True),    # norm of the unscaled gradient is 40: 0.25 g has norm 10, clipped by 0.1
    (1027, 0.0, 0.25, 2.0, True),     # unscaled norm 2 > max_norm, scaled norm 0.5: clipping inactive
    (1027, 0.0, 1.0, 40.0, False),    # norm = NULL: no clipping whatever the gradient
    (1027, 0.1, 0.25, 40.0, False),
    (1, 0.1, 0.25, 40.0, True), (3, 0.1, 0.25, 40.0, True), (5, 0.1, 0.25, 40.0, True), (1027, 0.1, 0.25, 40.0, True),
    (BIG_ADAM, 0.1, 0.25, 40.0, True),
])
def test_adam_step(cuda, n, wd, gscale, gnorm, use_norm):
    """Three steps against torch.optim.Adam in fp64 on the same fp32 inputs; the reference scales the
    gradient by grad_scale, then clips it (clip_grad_norm_, max_norm 1) when a norm is given. Bars: 2e-6
    absolute on p (p ~ N(0, 1), lr 1e-4), 2e-5 max-relative on m and v."""
    g = torch.Generator().manual_seed(60 + n % 89)
    L = lib()
    p0 = torch.randn(n, generator=g)
    g0 = torch.randn(n, generator=g)
    g0 = g0 * (gnorm / g0.double().norm().item())
    pd, m, v = p0.to(cuda), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)
    ws = torch.empty(L.dll.argus_sumsq_workspace_bytes(n), dtype=torch.uint8, device=cuda)
    norm = _nan(cuda, 1)
    ref_p = p0.double().requires_grad_(True)
    opt = torch.optim.Adam([ref_p], lr=1e-4, weight_decay=wd)
    for step in range(1, 4):
        gs = g0 * (0.8 + 0.1 * step)
        ref_p.grad = gs.double() * gscale
        scaled_norm = ref_p.grad.norm().item()
        if use_norm:
            assert (scaled_norm > 1.5) == (gnorm * gscale > 1) and (scaled_norm > 1.5 or scaled_norm < 0.7)
            torch.nn.utils.clip_grad_norm_([ref_p], 1.0)
        opt.step()
        gd = gs.to(cuda)
        if use_norm:
            L.global_norm(n, ptr(gd), ptr(norm), ptr(ws), stream())  # of the unscaled gradient
        L.adam_step(n, ptr(pd), ptr(gd), ptr(m), ptr(v), ptr(norm) if use_norm else None, C.c_float(gscale),
                    C.c_float(1.0), C.c_float(1e-4), C.c_float(0.9), C.c_float(0.999), C.c_float(1e-8), C.c_float(wd),
                    C.c_float(1 - 0.9**step), C.c_float(1 - 0.999**step), stream())
    st = opt.state[ref_p]
    tag = (n, wd, gscale, gnorm, use_norm)
    assert (pd.cpu().double() - ref_p.detach()).abs().max().item() < 2e-6, tag
    assert _rel(m, st["exp_avg"]) < 2e-5, tag
    assert _rel(v, st["exp_avg_sq"]) < 2e-5, tag
