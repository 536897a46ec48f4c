"""The layer-1 y3 recompute on the persistent conv1 data gradient (conv_p1x1.hip, p1x1_dgrad_kernel<64, BW, true>):
bn3's input y3 = conv3(a2) is rebuilt per tile from a2 and conv3's bf16 forward weights instead of read, and the
engine then never stores it for the blocks whose every reader recomputes it. Everything is compared bit for bit
against the same kernels reading the y3 the forward stored.
"""
import ctypes as C

import pytest
import torch

from argus_amd._lib import BF16, ConvDesc, lib, ptr, stream

pytestmark = pytest.mark.gpu


def _desc(n, hw, cin, cout):
    return ConvDesc(n, hw, hw, cin, cout, 1, 1, 1, 0, hw, hw, 0)


def _prep(d, w_ohwi, cuda):
    k, _, _, c = w_ohwi.shape
    wf = torch.empty(k, c, dtype=torch.bfloat16, device=cuda)
    wd = torch.empty(c, k, dtype=torch.bfloat16, device=cuda)
    lib().conv_weight_prep(C.byref(d), BF16, ptr(w_ohwi), None, ptr(wf), ptr(wd), stream())
    return wf, wd


def _stored_vs_recomputed(cuda, n, hw, w3, k1, dual, with_add, with_pro):
    """The data gradient k1 -> 4*w3 channels of the next block's conv1 with the block-output BN's backward
    epilogue (mask bits, folded finalize), once reading the y3 argus_conv_fwd stored, once recomputing it from
    a2: ((dm bits, part, part2, the ten finalize outputs, kernel names) of both runs)."""
    from argus_amd._lib import BnBwdEpilogue, BnBwdPrologue
    from argus_amd.profiling import KernelTimer

    torch.manual_seed(97)
    L = lib()
    cout = 4 * w3
    P = n * hw * hw
    d3 = _desc(n, hw, w3, cout)
    a2 = torch.relu(torch.randn(P, w3, device=cuda)).to(torch.bfloat16)
    wf3, _ = _prep(d3, (torch.randn(cout, 1, 1, w3) * (2.0 / w3) ** 0.5).to(cuda), cuda)
    y3 = torch.empty(P, cout, dtype=torch.bfloat16, device=cuda)
    st3 = torch.empty(L.dll.argus_conv_fwd_stat_rows(C.byref(d3), BF16) * cout * 2, device=cuda)
    L.conv_fwd(C.byref(d3), BF16, ptr(a2), ptr(wf3), ptr(y3), None, None, ptr(st3), stream())
    d = _desc(n, hw, cout, k1)
    _, wt = _prep(d, (torch.randn(k1, 1, 1, cout) * (2.0 / cout) ** 0.5).to(cuda), cuda)
    dm1 = torch.randn(P, k1, device=cuda).to(torch.bfloat16)
    y1 = torch.randn(P, k1, device=cuda).to(torch.bfloat16)
    ca, cb, cc = (torch.randn(k1, device=cuda) * 0.5 for _ in range(3))
    dh = torch.randn(P, cout, device=cuda).to(torch.bfloat16)
    yd = torch.randn(P, cout, device=cuda).to(torch.bfloat16)
    bits = torch.randint(0, 256, (P * cout // 8,), dtype=torch.uint8, device=cuda)
    mean, invstd = torch.randn(cout, device=cuda) * 0.1, torch.rand(cout, device=cuda) + 0.5
    mean2, invstd2 = torch.randn(cout, device=cuda) * 0.1, torch.rand(cout, device=cuda) + 0.5
    gamma, gamma2 = torch.rand(cout, device=cuda) + 0.5, torch.rand(cout, device=cuda) + 0.5
    # partial rows: the library's count, the persistent kernel's row splits (<= 256), the igemm recompute's 64-row tiles
    rows = max(L.dll.argus_conv_dgrad_bn_rows(C.byref(d), BF16), 256, (P + 63) // 64) + 8
    outs = []
    for rec in (False, True):
        out = torch.empty(P, cout, dtype=torch.bfloat16, device=cuda)
        part = torch.zeros(rows, cout, 2, device=cuda)
        part2 = torch.zeros(rows, cout, 2, device=cuda)
        ws = torch.zeros(L.dll.argus_bn_workspace_bytes(cout), dtype=torch.uint8, device=cuda)
        fin = [torch.full((cout,), float("nan"), device=cuda) for _ in range(10)]
        e = BnBwdEpilogue()
        e.mean, e.invstd, e.mask_mode, e.mask_bits, e.part = ptr(mean), ptr(invstd), 3, ptr(bits), ptr(part)
        e.workspace, e.gamma, e.dgamma, e.dbeta, e.ca, e.cb, e.cc = ptr(ws), ptr(gamma), *(ptr(t) for t in fin[:5])
        if dual:
            e.y2, e.mean2, e.invstd2, e.part2 = ptr(yd), ptr(mean2), ptr(invstd2), ptr(part2)
            e.gamma2, e.dgamma2, e.dbeta2, e.ca2, e.cb2, e.cc2 = ptr(gamma2), *(ptr(t) for t in fin[5:])
        if rec:
            e.y_x, e.y_w, e.y_k = ptr(a2), ptr(wf3), w3
        else:
            e.y = ptr(y3)
        pro = BnBwdPrologue(ptr(y1), ptr(ca), ptr(cb), ptr(cc), None) if with_pro else None
        with KernelTimer() as kt:
            L.conv_dgrad_bn(C.byref(d), BF16, ptr(dm1), ptr(wt), ptr(out), ptr(dh) if with_add else None, C.byref(e),
                            C.byref(pro) if pro is not None else None, stream())
        torch.cuda.synchronize()
        names = list(kt.summary())
        assert int(ws[:16384].view(torch.int32).abs().sum()) == 0  # finalize counters left at zero
        outs.append((out.view(torch.int16).cpu(), part.cpu(), part2.cpu(), [t.cpu() for t in fin], names))
    return outs


def _assert_identical(outs, dual):
    (o0, p0, q0, f0, _), (o1, p1, q1, f1, _) = outs
    assert torch.equal(o0, o1)
    assert torch.equal(p0, p1) and torch.equal(q0, q1)
    for i, (a, b) in enumerate(zip(f0, f1)):
        if not dual and i >= 5:  # the second branch's outputs are not written
            continue
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), i
        assert torch.equal(a, b), i


# 75 pixels: two tiles, the last ragged; 432: one tile per workgroup; 18,000 = 281.25 tiles against 256 row
# splits: some workgroups walk two tiles, the last tile ragged
@pytest.mark.parametrize("n,hw", [(3, 5), (3, 12), (5, 60)])
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("with_add", [False, True])
def test_persistent_dgrad_y_recompute_bit_identical(cuda, n, hw, dual, with_add):
    """p1x1_dgrad_kernel<64, BW, true> against <64, BW> reading the stored y3: dm3 bits, both partials and the
    ten folded-finalize outputs equal, the finalize counters back at zero, both runs on the persistent kernel."""
    outs = _stored_vs_recomputed(cuda, n, hw, 64, 64, dual, with_add, True)
    _assert_identical(outs, dual)
    bw = 4 if dual else 3
    assert f"argus::p1x1_dgrad_kernel<64, {bw}>" in outs[0][4], outs[0][4]
    assert f"argus::p1x1_dgrad_kernel<64, {bw}, true>" in outs[1][4], outs[1][4]
    assert not any(nm.startswith("argus::igemm_kernel") for o in outs for nm in o[4]), outs


def test_wider_y_recompute_stays_on_the_igemm(cuda):
    """y_k = 128 (128 -> 512 channels, into a 128-wide conv1): not the persistent kernel's; the register-staged
    igemm's epilogue recomputes it, still bit-identical."""
    outs = _stored_vs_recomputed(cuda, 3, 6, 128, 128, True, True, False)
    _assert_identical(outs, True)
    for o in outs:
        assert any(nm.startswith("argus::igemm_kernel") for nm in o[4]), o[4]
        assert not any(nm.startswith("argus::p1x1_dgrad_kernel") for nm in o[4]), o[4]


def test_engine_layer1_y3_never_stored_bit_identical(cuda):
    """B = 10 at 128 x 128 (layer 1: 20,480 pixels = 320 tiles > 256 row splits): three bf16 training steps and
    an eval forward with the default schedule (y3 of the 64-wide blocks whose successor has no downsample
    recomputed in the persistent conv1 data gradient and the fused conv3 data + weight gradient, never stored)
    against yrec_epi = False, y3_free = False: losses, parameters, Adam moments, state_dict and predictions equal."""
    from argus_amd.models import NCameraCNN
    from argus_amd.profiling import KernelTimer
    from argus_amd.step import FusedTrainer
    from oracle import se3

    g = torch.Generator().manual_seed(5)
    x = (torch.randint(0, 256, (10, 6, 128, 128), generator=g, dtype=torch.uint8).float() / 255.0).to(cuda)
    T = se3.random_targets(10, generator=g).float().to(cuda)
    runs = []
    for attrs in ({}, {"yrec_epi": False, "y3_free": False}):
        torch.manual_seed(42)
        model = NCameraCNN(compute_dtype="bf16").to(cuda).train()
        tr = FusedTrainer(model, lr=1e-3, max_grad_norm=1.0)
        eng = model._engine(cuda)
        for k, v in attrs.items():
            setattr(eng, k, v)
        losses = [tr.step(x, T).clone() for _ in range(2)]
        with KernelTimer() as kt:
            losses.append(tr.step(x, T).clone())
        torch.cuda.synchronize()
        launches = {nm: v["launches"] for nm, v in kt.summary().items()}
        free = [i for i in range(len(eng.blocks)) if eng._y3_free(i)]
        stored = [i for i, a in enumerate(eng.act) if a["y3"] is not None]
        model.eval()
        with torch.no_grad():
            pe = model(x).clone()
        torch.cuda.synchronize()
        runs.append((torch.stack(losses).cpu(), tr.flat.param.cpu(), tr.exp_avg_sq.cpu(),
                     {k: v.cpu() for k, v in model.state_dict().items()}, pe.cpu(), launches, free, stored))
    (l1, p1, v1, s1, e1, k1, free1, stored1), (l0, p0, v0, s0, e0, k0, free0, stored0) = runs
    assert torch.equal(l1, l0) and torch.equal(p1, p0) and torch.equal(v1, v0)
    assert all(torch.equal(s1[k], s0[k]) for k in s1)
    assert torch.equal(e1, e0)
    # ResNet-50: layer 1's blocks 0 and 1 (block 2's y3 is read by layer 2's strided downsample data gradient)
    assert free1 == [0, 1] and free0 == []
    assert stored1 == list(range(2, 16)) and stored0 == list(range(16))  # the freed blocks' buffers never allocated
    assert k1.get("argus::p1x1_dgrad_kernel<64, 3, true>") == 1 and k1.get("argus::p1x1_dgrad_kernel<64, 4, true>") == 1, k1
    assert "argus::p1x1_dgrad_kernel<64, 3>" not in k1 and "argus::p1x1_dgrad_kernel<64, 4>" not in k1, k1
    assert k1.get("argus::dgw1x1_kernel<true, true>") == 2 and k1.get("argus::dgw1x1_kernel<true, false>") == 1, k1
    assert k0.get("argus::p1x1_dgrad_kernel<64, 3>") == 1 and k0.get("argus::p1x1_dgrad_kernel<64, 4>") == 1, k0
    assert k0.get("argus::dgw1x1_kernel<true, false>") == 3 and "argus::dgw1x1_kernel<true, true>" not in k0, k0
