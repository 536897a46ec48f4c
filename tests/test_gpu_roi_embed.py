"""GPU: the two launches that condition the pose head on the region of interest, through the C ABI, against the
fp64 restatement (tests/roi_embed_reference.py).

argus_roi_embed (training / eval, any batch): |z_out - ref| <= 2^-19 S per element, S = |z_in| + sum_k |w_r[j][k]
rho[b][k]| (2^-17 S at 16 cameras: see the reference), rho within 4 ulp (roi_embed_reference.RHO_ULP), g the bits of
argus_gelu_f32 of the kernel's own z, complete writes, untouched guard words, optional outputs, reproducible bits,
and every refusal without a launch.

argus_pose_tail_roi (deployment, batch * n_cams <= 16): pred against the fp64 head with the term at
tests/test_gpu_pose_head.py's bar (max error < 1e-5 of the reference's maximum), pose the bits of argus_se3_exp of
its own pred, argus_pose_tail's bits at w_r = 0, zero tickets, one workspace for every batch, reproducible bits."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import roi_embed_reference as ref  # noqa: E402

from argus_amd._lib import lib, ptr, stream  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
TICKET_BYTES = 256


def _guarded(cuda, *shape):
    """A NaN-prefilled fp32 buffer of ``shape`` followed by GUARD words of a sentinel; (whole, payload view)."""
    n = int(np.prod(shape))
    whole = torch.full((n + GUARD,), float("nan"), device=cuda)
    whole[n:] = -7.5
    return whole, whole[:n].view(*shape)


def _guard_ok(whole):
    return bool((whole[-GUARD:] == -7.5).all())


def _embed(cuda, batch, n_cams, rois, w_r, z, with_g=True, with_rho=True):
    zw, zv = _guarded(cuda, batch, 128)
    zv.copy_(z)
    gw, gv = _guarded(cuda, batch, 128)
    rw, rv = _guarded(cuda, batch, 4 * n_cams)
    lib().roi_embed(batch, n_cams, *ref.FRAME_HW, *ref.HW, ptr(rois), ptr(w_r), ptr(zv), ptr(gv) if with_g else None,
                    ptr(rv) if with_rho else None, stream())
    assert _guard_ok(zw) and _guard_ok(gw) and _guard_ok(rw)
    return zv, gv, rv


@pytest.mark.parametrize("batch,n_cams", ref.EMBED_CASES, ids=lambda v: str(v))
def test_roi_embed(cuda, batch, n_cams):
    L = lib()
    rois, w_r, z = ref.embed_case(batch, n_cams)
    rho64 = ref.features(rois, n_cams)
    want = ref.embed(z, rho64, w_r)
    S = ref.embed_scale(z, rho64, w_r)
    rg, wg, zg = (torch.from_numpy(a).to(cuda) for a in (rois, w_r, z))
    zo, go, ro = _embed(cuda, batch, n_cams, rg, wg, zg)
    assert bool(torch.isfinite(zo).all()) and bool(torch.isfinite(go).all()) and bool(torch.isfinite(ro).all())
    ratio = (np.abs(zo.double().cpu().numpy() - want) / (ref.embed_bar(n_cams) * S)).max()
    ulps = (np.abs(ro.double().cpu().numpy() - rho64).reshape(-1, 4) / ref.RHO_ULP).max()
    print(f"roi_embed ({batch}, {n_cams}): max |z - ref| / bar = {ratio:.3f}; rho {ulps:.2f} ulp")
    assert ratio <= 1.0
    assert ulps <= 4.0
    if batch * n_cams > 1:  # the exact centre crop: features exactly zero
        assert not bool(ro.view(-1, 4)[0].any())
    gel = torch.empty_like(zo)
    L.gelu_f32(zo.numel(), ptr(zo), ptr(gel), stream())
    assert torch.equal(go.view(torch.int32), gel.view(torch.int32))  # argus_gelu_f32 of the kernel's own z
    # optional outputs leave z alone (and are not written); two runs give the same bits
    z2, g2, r2 = _embed(cuda, batch, n_cams, rg, wg, zg, with_g=False, with_rho=False)
    assert torch.equal(z2.view(torch.int32), zo.view(torch.int32))
    assert bool(torch.isnan(g2).all()) and bool(torch.isnan(r2).all())
    z3, g3, r3 = _embed(cuda, batch, n_cams, rg, wg, zg)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in ((z3, zo), (g3, go), (r3, ro)))


def test_roi_embed_refusals_launch_nothing(cuda):
    L = lib().dll
    rois, w_r, z = (torch.from_numpy(a).to(cuda) for a in ref.embed_case(2, 2))
    zw, zv = _guarded(cuda, 2, 128)
    zv.copy_(z)
    before = zw.clone()
    ok = dict(batch=2, n_cams=2, frame_h=96, frame_w=128, h=64, w=64, rois=ptr(rois), w_r=ptr(w_r), z=ptr(zv))
    for kw, name in ((dict(rois=None), "rois"), (dict(w_r=None), "w_r"), (dict(z=None), "z"), (dict(batch=0), "batch"),
                     (dict(n_cams=-1), "n_cams"), (dict(frame_h=0), "frame_h"), (dict(frame_w=0), "frame_w"),
                     (dict(h=7), "h"), (dict(w=4), "w"), (dict(h=97), "h > frame_h"), (dict(w=129), "w > frame_w"),
                     (dict(n_cams=17), "n_cams")):
        a = {**ok, **kw}
        rc = L.argus_roi_embed(a["batch"], a["n_cams"], a["frame_h"], a["frame_w"], a["h"], a["w"], a["rois"], a["w_r"],
                               a["z"], None, None, stream())
        assert rc == 1 and name in L.argus_last_error().decode(), (kw, L.argus_last_error())
    torch.cuda.synchronize()
    assert torch.equal(zw.view(torch.int32), before.view(torch.int32))  # nothing ran


# ---- argus_pose_tail_roi ------------------------------------------------------------------------------------------
def _mlp(gen, d):
    shapes = [(128, d), (128,), (128, 128), (128,), (6, 128), (6,)]
    return [torch.randn(*s, generator=gen) / (s[-1] ** 0.5 if len(s) == 2 else 2.0) for s in shapes]


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _tail(cuda, batch, n_cams, g0, params, rois, w_r, ws):
    pw, pred = _guarded(cuda, batch, 6)
    qw, pose = _guarded(cuda, batch, 7)
    args = (batch, g0.shape[1], ptr(g0), *[ptr(p) for p in params], ptr(pred), ptr(pose), 0)
    if w_r is None:
        lib().pose_tail(*args, ptr(ws), ws.numel(), stream())
    else:
        lib().pose_tail_roi(*args, n_cams, *ref.FRAME_HW, *ref.HW, ptr(rois), ptr(w_r), ptr(ws), ws.numel(), stream())
    assert int(ws[:TICKET_BYTES].count_nonzero()) == 0  # ticket words are zero on return
    assert _guard_ok(pw) and _guard_ok(qw)
    assert bool(torch.isfinite(pred).all()) and bool(torch.isfinite(pose).all())
    return pred, pose


@pytest.fixture(scope="module")
def tail_ws(cuda):
    """One workspace per d, sized for the largest batch (16) and zeroed once: it serves every smaller batch."""
    return {d: torch.zeros(lib().dll.argus_pose_tail_workspace_bytes(16, d), dtype=torch.uint8, device=cuda)
            for d in (64, 128, 2048)}


@pytest.mark.parametrize("d", [64, 128, 2048])
@pytest.mark.parametrize("batch,n_cams", [(1, 1), (1, 2), (2, 2), (3, 3), (8, 2), (16, 1)], ids=lambda v: str(v))
def test_pose_tail_roi(cuda, tail_ws, d, batch, n_cams):
    L = lib()
    gen = torch.Generator().manual_seed(1000 * d + 10 * batch + n_cams)
    params = _mlp(gen, d)
    g0 = torch.nn.functional.gelu(torch.randn(batch, d, generator=gen))
    rois, w_r, _ = ref.embed_case(batch, n_cams, seed=d)
    rho = ref.features(rois, n_cams)
    want = ref.head(g0.numpy(), [p.numpy() for p in params], rho, w_r)
    plain = ref.head(g0.numpy(), [p.numpy() for p in params])
    ws = tail_ws[d]
    g0g, pg = g0.to(cuda), [p.to(cuda) for p in params]
    rg, wg = torch.from_numpy(rois).to(cuda), torch.from_numpy(w_r).to(cuda)
    (pred, pose), (pred2, pose2) = [_tail(cuda, batch, n_cams, g0g, pg, rg, wg, ws) for _ in range(2)]
    assert torch.equal(pred.view(torch.int32), pred2.view(torch.int32))  # bit-reproducible
    assert torch.equal(pose.view(torch.int32), pose2.view(torch.int32))
    err = _rel(pred, want)
    print(f"pose_tail_roi d={d} ({batch}, {n_cams}): pred relative error {err:.3e}; the term moves pred by "
          f"{_rel(plain, want):.3e}")
    assert err < 1e-5
    assert _rel(plain, want) > 1e-3  # the term is not negligible in this case: the comparison sees it
    se3 = torch.empty(batch, 7, device=cuda)
    L.se3_exp(batch, ptr(pred.contiguous()), ptr(se3), 0, stream())
    assert torch.equal(pose.view(torch.int32), se3.view(torch.int32))  # argus_se3_exp of this launch's own pred
    # w_r = 0: argus_pose_tail's bits, both outputs
    zero = torch.zeros_like(wg)
    p0, q0 = _tail(cuda, batch, n_cams, g0g, pg, rg, zero, ws)
    p1, q1 = _tail(cuda, batch, n_cams, g0g, pg, None, None, ws)
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32)) and torch.equal(q0.view(torch.int32), q1.view(torch.int32))


def test_pose_tail_roi_refuses_17_images(cuda, tail_ws):
    L = lib().dll
    ws = tail_ws[128]
    t = torch.zeros(17 * 128, device=cuda)
    for batch, n_cams in ((17, 1), (9, 2), (1, 17)):
        rc = L.argus_pose_tail_roi(batch, 128, *[ptr(t)] * 9, 0, n_cams, *ref.FRAME_HW, *ref.HW, ptr(t), ptr(t), ptr(ws),
                                   1 << 30, stream())
        assert rc == 1 and b"pose_tail_roi" in L.argus_last_error(), (batch, n_cams)
    assert int(ws[:TICKET_BYTES].count_nonzero()) == 0


def test_both_launches_make_the_same_features_and_term(cuda, tail_ws):
    """One device function states a feature and one the dot product: with the MLP behind output_mlp.0 cut off
    (w0 = 0, so the pre-activation is b0 + e in both), argus_roi_embed's z followed by the plain launches'
    arithmetic cannot be told from the fused tail. Checked on h1 through pred: w2 = identity rows, w4 picks six."""
    batch, n_cams, d = 3, 2, 64
    rois, w_r, z = ref.embed_case(batch, n_cams, seed=5)
    b0 = torch.from_numpy(z[0]).clone()
    w2, b2 = torch.eye(128), torch.zeros(128)
    w4, b4 = torch.zeros(6, 128), torch.zeros(6)
    for o in range(6):
        w4[o, 20 * o] = 1.0
    params = [torch.zeros(128, d), b0, w2, b2, w4, b4]
    g0 = torch.ones(batch, d)
    rg, wg = torch.from_numpy(rois).to(cuda), torch.from_numpy(w_r).to(cuda)
    pred, _ = _tail(cuda, batch, n_cams, g0.to(cuda), [p.to(cuda) for p in params], rg, wg, tail_ws[d])
    zin = b0.expand(batch, 128).contiguous().to(cuda)
    zo, go, _ = _embed(cuda, batch, n_cams, rg, wg, zin)
    g2 = torch.empty_like(go)
    lib().gelu_f32(go.numel(), ptr(go.contiguous()), ptr(g2), stream())  # output_mlp.2 = identity, then its GELU
    assert torch.equal(pred.view(torch.int32), g2[:, 0:120:20].contiguous().view(torch.int32))
