"""GPU: the frozen pose head in two launches, through the C ABI. argus_pool_fc_gelu (avg-pool + resnet.fc + GELU)
and argus_pose_tail (output MLP + se(3) Exp) against fp64 from their own inputs at test_gemm_f32_epilogues' bar
(max error below 1e-5 of the reference's maximum), the pooled mean taken in fp64 from the T tensor. Both split
their reduction over workgroups behind a ticket: two runs must agree bit for bit and leave every ticket zero, with
one workspace (zeroed once) serving every row count."""
import pytest
import torch
import torch.nn.functional as F

from argus_amd._lib import BF16, F16, lib, ptr, stream
from oracle import se3
from tests import se3_cases

pytestmark = pytest.mark.gpu

TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
DT = {"bf16": BF16, "fp16": F16}
C_IN = 2048
TICKET_BYTES = 256


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def fc(cuda):
    """rdim -> (w_fc, b_fc) on the device and in fp64, and one workspace for every case: sized for 16 rows, zeroed
    once here and never again."""
    gen = torch.Generator().manual_seed(3)
    out = {}
    for rdim in (1024, 64):
        w = torch.randn(rdim, C_IN, generator=gen) / C_IN ** 0.5
        b = 0.5 * torch.randn(rdim, generator=gen)
        out[rdim] = (w.to(cuda), b.to(cuda), w.double(), b.double())
    nbytes = lib().dll.argus_pool_fc_gelu_workspace_bytes(16, C_IN, 1024)
    assert nbytes >= lib().dll.argus_pool_fc_gelu_workspace_bytes(16, C_IN, 64) > 0
    out["ws"] = torch.zeros(nbytes, dtype=torch.uint8, device=cuda)
    return out


# hw 12: a 72 x 104 frame's 3 x 4 final map; 64: 256 x 256's 8 x 8. Every hw with every n at the real rdim = 1024
CASES = [(n, hw, 1024, "bf16") for hw in (1, 4, 12, 64) for n in (1, 2, 16)] + \
        [(2, 12, 1024, "fp16"), (16, 64, 1024, "fp16"), (1, 1, 64, "fp16"), (16, 12, 64, "bf16"), (2, 64, 64, "bf16")]


@pytest.mark.parametrize("n,hw,rdim,dt", CASES, ids=lambda v: str(v))
def test_pool_fc_gelu(cuda, fc, n, hw, rdim, dt):
    L = lib()
    gen = torch.Generator().manual_seed(1000 * n + 10 * hw + rdim)
    x = (4 * torch.rand(n, hw, C_IN, generator=gen) * (torch.rand(n, hw, C_IN, generator=gen) > 0.3)).to(TDT[dt])
    wg, bg, w64, b64 = fc[rdim]
    ws = fc["ws"]
    ref = F.gelu(x.double().mean(1) @ w64.T + b64)
    xg = x.to(cuda)
    outs = []
    for _ in range(2):
        g0 = torch.full((n + 1, rdim), float("nan"), device=cuda)
        L.pool_fc_gelu(DT[dt], n, hw, C_IN, ptr(xg), ptr(wg), ptr(bg), rdim, ptr(g0), ptr(ws), ws.numel(), stream())
        assert int(ws[:TICKET_BYTES].count_nonzero()) == 0  # every call leaves the tickets zero
        assert bool(torch.isnan(g0[n]).all()) and bool(torch.isfinite(g0[:n]).all())
        outs.append(g0[:n])
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))  # bit-reproducible
    err = _rel(outs[0], ref)
    print(f"pool_fc_gelu n={n} hw={hw} rdim={rdim} {dt}: relative error {err:.3e}")
    assert err < 1e-5


def test_head_refuses_more_than_16_rows(cuda, fc):
    wg, bg, _, _ = fc[1024]
    ws = fc["ws"]
    x = torch.zeros(17, 1, C_IN, dtype=torch.bfloat16, device=cuda)
    g0 = torch.zeros(17, 1024, device=cuda)
    rc = lib().dll.argus_pool_fc_gelu(BF16, 17, 1, C_IN, ptr(x), ptr(wg), ptr(bg), 1024, ptr(g0), ptr(ws), 1 << 30, stream())
    assert rc == 1 and b"16 rows" in lib().dll.argus_last_error()
    assert int(ws[:TICKET_BYTES].count_nonzero()) == 0


def _mlp(gen, d=2 * 1024):
    shapes = [(128, d), (128,), (128, 128), (128,), (6, 128), (6,)]
    return [torch.randn(*s, generator=gen) / (s[-1] ** 0.5 if len(s) == 2 else 2.0) for s in shapes]


def _tail(cuda, batch, g0, params, canon, ws):
    pred = torch.full((batch + 1, 6), float("nan"), device=cuda)
    pose = torch.full((batch + 1, 7), float("nan"), device=cuda)
    lib().pose_tail(batch, g0.shape[1], ptr(g0), *[ptr(p) for p in params], ptr(pred), ptr(pose), canon, ptr(ws),
                    ws.numel(), stream())
    assert int(ws[:TICKET_BYTES].count_nonzero()) == 0
    assert bool(torch.isnan(pred[batch]).all()) and bool(torch.isnan(pose[batch]).all())
    assert bool(torch.isfinite(pred[:batch]).all()) and bool(torch.isfinite(pose[:batch]).all())
    return pred[:batch], pose[:batch]


def _exp_bar(ref):
    """test_se3_exp_kernel's bar: 2^-22 * max(1, |t|_inf) per sample."""
    return 2.0 ** -22 * ref[:, :3].abs().amax(-1).clamp_min(1.0)


@pytest.mark.parametrize("batch", [1, 2, 8])
def test_pose_tail(cuda, batch):
    L = lib()
    gen = torch.Generator().manual_seed(50 + batch)
    d = 2048
    params = _mlp(gen)
    g0 = F.gelu(torch.randn(batch, d, generator=gen))  # what argus_pool_fc_gelu hands over: GELU outputs
    w0, b0, w2, b2, w4, b4 = [p.double() for p in params]
    ref = F.gelu(F.gelu(g0.double() @ w0.T + b0) @ w2.T + b2) @ w4.T + b4
    ws = torch.zeros(L.dll.argus_pose_tail_workspace_bytes(8, d), dtype=torch.uint8, device=cuda)  # for the largest batch
    g0g, pg = g0.to(cuda), [p.to(cuda) for p in params]
    runs = {canon: [_tail(cuda, batch, g0g, pg, canon, ws) for _ in range(2)] for canon in (0, 1)}
    for canon, ((pred, pose), (pred2, pose2)) in runs.items():
        assert torch.equal(pred.view(torch.int32), pred2.view(torch.int32))  # bit-reproducible
        assert torch.equal(pose.view(torch.int32), pose2.view(torch.int32))
        assert torch.equal(pred.view(torch.int32), runs[0][0][0].view(torch.int32))  # canonical_w leaves pred alone
        err = _rel(pred, ref)
        print(f"pose_tail batch={batch} canonical_w={canon}: pred relative error {err:.3e}")
        assert err < 1e-5
        want = torch.empty(batch, 7, device=cuda)
        L.se3_exp(batch, ptr(pred.contiguous()), ptr(want), canon, stream())
        assert torch.equal(pose.view(torch.int32), want.view(torch.int32))  # argus_se3_exp of this launch's own pred
    pred, pose = runs[0][0]
    exp = se3.se3_exp(pred.double().cpu())
    assert bool(((pose.double().cpu() - exp).abs().amax(-1) <= _exp_bar(exp)).all())


@pytest.mark.parametrize("regime", ["pred_small_angle", "pred_beyond_pi"])
def test_pose_tail_exp_regimes(cuda, regime):
    """Rows of tests/se3_cases.py forced through the launch by w4 = 0, b4 = xi: the Taylor branch below 1e-4 rad
    and rotation angles beyond pi (where canonical_w negates the quaternion)."""
    L = lib()
    gen = torch.Generator().manual_seed(8)
    params = _mlp(gen)
    params[4] = torch.zeros(6, 128)
    xis = se3_cases.regimes()[regime][0][:4]
    batch, d = 2, 2048
    g0 = F.gelu(torch.randn(batch, d, generator=gen)).to(cuda)
    ws = torch.zeros(L.dll.argus_pose_tail_workspace_bytes(batch, d), dtype=torch.uint8, device=cuda)
    for xi in xis:
        params[5] = xi.clone()
        pg = [p.to(cuda) for p in params]
        ref = se3.se3_exp(xi.double()[None].repeat(batch, 1))
        for canon in (0, 1):
            pred, pose = _tail(cuda, batch, g0, pg, canon, ws)
            assert torch.equal(pred.cpu(), xi[None].repeat(batch, 1))  # 0 * h + b4 exactly
            want = torch.empty(batch, 7, device=cuda)
            L.se3_exp(batch, ptr(pred.contiguous()), ptr(want), canon, stream())
            assert torch.equal(pose.view(torch.int32), want.view(torch.int32))
            got = pose.double().cpu()
            if canon:
                assert bool((got[:, 6] >= 0).all())
                got = torch.where(ref[:, 6:] < 0, torch.cat([got[:, :3], -got[:, 3:]], -1), got)
            assert bool(((got - ref).abs().amax(-1) <= _exp_bar(ref)).all())
