"""GPU: the two entry points of frozen fine-tuning against fp64 references of the GPU's own inputs.

argus_bias_grad: db[k] = sum_p dm[p][k]. Bar |err| <= 2e-5 * sum_p |dm[p][k]|: the project's fp32 stage bar
applied to the magnitude sum (the kernel's stated accumulation rule, fp32 runs of at most 64 rows and fp64 above,
bounds the error by 64 * 2^-24 = 3.9e-6 of it, below a quarter of the bar).

argus_conv_fold_bn_bwd: the derivative of argus_conv_fold_bn. Reference: fp64 autograd of
<w * scale, dwf> + <beta - mean * scale, db> with respect to (w, gamma, beta). dw at 2e-5 relative and bit-equal
to dwf * scale with argus_bn_eval_coeffs' scale; dgamma within 2e-5 * invstd * (sum_j |dwf * w| + |mean * db|)
(the lane-strided sum is at most about 80 additions deep: worst case 4.8e-6 of that magnitude); dbeta bit-equal
to db.
"""
import ctypes as C

import pytest
import torch

from argus_amd._lib import BF16, F32, ConvDesc, lib, ptr, stream

pytestmark = pytest.mark.gpu

DT = {"fp32": (F32, torch.float32), "bf16": (BF16, torch.bfloat16)}
TICKET_BYTES = 4096  # argus_conv_infer_workspace_bytes' ticket region: the partial rows start here


def _plan(dt, P, K, splits_in=0):
    L = lib()
    sp, mx, nb = C.c_int(0), C.c_int(0), C.c_size_t(0)
    L.bias_grad_plan(dt, P, K, splits_in, C.byref(sp), C.byref(mx), C.byref(nb))
    return sp.value, mx.value, nb.value


def _bias_grad(dt, dm, splits, ws):
    L = lib()
    P, K = dm.shape
    db = torch.full((K,), float("nan"), device=dm.device)
    L.bias_grad(dt, P, K, ptr(dm), ptr(db), splits, ptr(ws), 0 if ws is None else ws.numel(), stream())
    return db


def _workspace(cuda, nbytes):
    """Tickets zero, the slab region NaN-prefilled."""
    ws = torch.zeros(max(nbytes, TICKET_BYTES + 16), dtype=torch.uint8, device=cuda)
    ws[TICKET_BYTES:(ws.numel() - TICKET_BYTES) // 8 * 8 + TICKET_BYTES].view(torch.float64).fill_(float("nan"))
    return ws


BIAS_SHAPES = [(1, 64), (60, 64), (475, 2048), (4097, 192), (8192, 64)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", BIAS_SHAPES, ids=[f"{p}x{k}" for p, k in BIAS_SHAPES])
def test_bias_grad(cuda, dtype, shape):
    dt, tdt = DT[dtype]
    P, K = shape
    g = torch.Generator().manual_seed(P * 31 + K)
    # a mean well away from zero on some channels, mixed signs on others
    dm = (torch.randn(P, K, generator=g) + torch.linspace(-2, 2, K)).to(tdt).to(cuda)
    ref = dm.double().sum(0)
    mag = dm.double().abs().sum(0)
    sp0, mx, nb0 = _plan(dt, P, K)
    assert mx == min(P, 64) and 1 <= sp0 <= mx
    assert nb0 == (0 if sp0 == 1 else TICKET_BYTES + sp0 * K * 8)
    seen = set()
    for splits_in in (1, 2, 3, mx, 0):
        if splits_in > mx or splits_in in seen:
            continue  # (P = 1 has one slice; max may repeat an earlier value)
        seen.add(splits_in)
        sp, _, nb = _plan(dt, P, K, splits_in)
        assert sp == (splits_in or sp0) and nb == (0 if sp == 1 else TICKET_BYTES + sp * K * 8)
        ws = None if sp == 1 else _workspace(cuda, nb)
        db = _bias_grad(dt, dm, splits_in, ws)
        err = (db.double() - ref).abs()
        worst = float((err / mag.clamp_min(1e-300)).max())
        print(f"bias_grad {dtype} {shape} splits {splits_in or 'default'}={sp}: worst err / sum|dm| = {worst:.2e}")
        assert not torch.isnan(db).any()
        assert bool((err <= 2e-5 * mag).all()), (splits_in, worst)
        if ws is not None:
            assert int(ws[:TICKET_BYTES].view(torch.int32).abs().sum()) == 0  # tickets zero on return
            assert torch.equal(_bias_grad(dt, dm, splits_in, ws), db)  # and a second run is bit-equal


def test_bias_grad_one_workspace_serves_two_shapes(cuda):
    dt, tdt = DT["bf16"]
    g = torch.Generator().manual_seed(5)
    a = torch.randn(4097, 192, generator=g).to(tdt).to(cuda)
    b = torch.randn(700, 2048, generator=g).to(tdt).to(cuda)
    nb = max(_plan(dt, *a.shape, 3)[2], _plan(dt, *b.shape, 5)[2])
    ws = _workspace(cuda, nb)
    alone_a = _bias_grad(dt, a, 3, _workspace(cuda, nb))
    alone_b = _bias_grad(dt, b, 5, _workspace(cuda, nb))
    for _ in range(2):
        assert torch.equal(_bias_grad(dt, a, 3, ws), alone_a)
        assert torch.equal(_bias_grad(dt, b, 5, ws), alone_b)
    assert int(ws[:TICKET_BYTES].view(torch.int32).abs().sum()) == 0


FOLD_SHAPES = [(64, 64, 1), (64, 192, 3), (256, 64, 1), (512, 512, 3)]


@pytest.mark.parametrize("layout", ["ohwi", "channels_last_oihw"])
@pytest.mark.parametrize("shape", FOLD_SHAPES, ids=[f"{c}-{k}-{r}x{r}" for c, k, r in FOLD_SHAPES])
def test_conv_fold_bn_bwd(cuda, shape, layout):
    L = lib()
    cin, cout, ks = shape
    J = ks * ks * cin
    d = ConvDesc(2, 8, 8, cin, cout, ks, ks, 1, ks // 2, 8, 8, 0)
    g = torch.Generator().manual_seed(cin + 7 * cout + ks)
    w_ohwi = (torch.randn(cout, ks, ks, cin, generator=g) * 0.05).to(cuda)
    if layout == "ohwi":
        w, strides = w_ohwi, None
    else:  # the view FlatParams gives a conv weight: OIHW shape over OHWI storage
        w = w_ohwi.permute(0, 3, 1, 2)
        assert w.shape == (cout, cin, ks, ks) and w.stride() == (ks * ks * cin, 1, ks * cin, cin)
        strides = (C.c_int64 * 4)(*w.stride())
    gamma = (0.5 + torch.rand(cout, generator=g)).to(cuda)
    beta = (0.1 * torch.randn(cout, generator=g)).to(cuda)
    rm = (0.1 * torch.randn(cout, generator=g)).to(cuda)
    rv = (0.5 + torch.rand(cout, generator=g)).to(cuda)
    eps = 1e-5
    dwf = torch.randn(cout, J, generator=g).to(cuda)
    db = torch.randn(cout, generator=g).to(cuda)
    # fp64 autograd of <w * scale, dwf> + <beta - mean * scale, db>
    w64 = w_ohwi.double().view(cout, J).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    inv64 = 1.0 / torch.sqrt(rv.double() + eps)
    sc64 = g64 * inv64
    obj = (w64 * sc64[:, None] * dwf.double()).sum() + ((b64 - rm.double() * sc64) * db.double()).sum()
    rw, rg, rb = torch.autograd.grad(obj, (w64, g64, b64))
    mag = inv64 * ((dwf.double() * w_ohwi.double().view(cout, J)).abs().sum(1) + (rm.double() * db.double()).abs())
    scale, shift = torch.empty(cout, device=cuda), torch.empty(cout, device=cuda)
    L.bn_eval_coeffs(cout, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), C.c_float(eps), ptr(scale), ptr(shift), stream())
    results = []
    for in_place in (False, True):
        src = dwf.clone()
        dw = src if in_place else torch.full_like(dwf, float("nan"))
        dg, dbe = torch.full_like(db, float("nan")), torch.full_like(db, float("nan"))
        L.conv_fold_bn_bwd(C.byref(d), ptr(w), strides, ptr(gamma), ptr(rm), ptr(rv), C.c_float(eps), ptr(src), ptr(db),
                           ptr(dw), ptr(dg), ptr(dbe), stream())
        if not in_place:
            assert torch.equal(src, dwf)  # the input is read only
        assert torch.equal(dw, dwf * scale[:, None])  # one fp32 multiply by argus_bn_eval_coeffs' scale
        assert float((dw.double() - rw).abs().max()) <= 2e-5 * float(rw.abs().max())
        assert torch.equal(dbe, db) and torch.equal(dbe.double(), rb)
        err = (dg.double() - rg).abs()
        print(f"fold_bn_bwd {shape} {layout} in_place={in_place}: worst dgamma err / magnitude = "
              f"{float((err / mag).max()):.2e}")
        assert bool((err <= 2e-5 * mag).all())
        results.append((dw.clone(), dg))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])


def test_conv_fold_bn_bwd_gathers_any_strides(cuda):
    """A true OIHW-contiguous master (the gathered path) gives the bits of the OHWI one (same elements, same order)."""
    L = lib()
    cin, cout, ks = 64, 64, 3
    d = ConvDesc(2, 8, 8, cin, cout, ks, ks, 1, 1, 8, 8, 0)
    g = torch.Generator().manual_seed(3)
    w_oihw = (torch.randn(cout, cin, ks, ks, generator=g) * 0.05).to(cuda)
    w_ohwi = w_oihw.permute(0, 2, 3, 1).contiguous()
    gamma, rm, rv = (0.5 + torch.rand(cout, generator=g)).to(cuda), torch.randn(cout, generator=g).to(cuda), \
        (0.5 + torch.rand(cout, generator=g)).to(cuda)
    dwf, db = torch.randn(cout, ks * ks * cin, generator=g).to(cuda), torch.randn(cout, generator=g).to(cuda)
    out = []
    for w, st in ((w_ohwi, None), (w_oihw, (C.c_int64 * 4)(*w_oihw.stride()))):
        dw, dg, dbe = torch.empty_like(dwf), torch.empty_like(db), torch.empty_like(db)
        L.conv_fold_bn_bwd(C.byref(d), ptr(w), st, ptr(gamma), ptr(rm), ptr(rv), C.c_float(1e-5), ptr(dwf), ptr(db),
                           ptr(dw), ptr(dg), ptr(dbe), stream())
        out.append((dw, dg, dbe))
    assert all(torch.equal(a, b) for a, b in zip(*out))
