"""CPU: the contract of tests/test_gpu_exact.py, proved on the fp64 references alone for every case of
tests/exact_cases.py. Coverage (every (tap, channel) position of a reduction is non-zero in some filter), the
range conditions (16-bit outputs are integers within the type's exact range, fp32 sums stay below 2^24 in any
order), MX-fp8 exactness of the operands, and the demonstration why the tests exist: one term dropped from a
4608-term reduction passes the tolerance tests' bound on their random data and breaks equality on integers.

These conditions hold the GPU assertions in place: a case that cannot meet them gets other inputs, not a tolerance.
"""
import pytest
import torch

import exact_cases as X


def _is_int(t):
    return bool((t == t.round()).all())


def _check_lo(case, values, bound):
    for nm, v in values.items():
        assert _is_int(v), (case, nm, "not integer-valued")
        assert v.abs().max().item() <= bound, (case, nm, v.abs().max().item(), bound)


def _check_f32(case, mags):
    for nm, v in mags.items():
        assert float(v) < X.F32_MAX, (case, nm, float(v))


def _check_coverage(case, w, dgrad):
    """w OHWI: every (tap, cin) has a non-zero weight in some filter; for a data gradient every (tap, cout) has
    one in some input channel."""
    assert bool((w != 0).any(0).all()), (case, "a (tap, cin) position no filter reads")
    if dgrad:
        assert bool((w != 0).any(3).all()), (case, "a (tap, cout) position no input channel reads")


CONV_TABLES = {
    "igemm": X.IGEMM_CASES, "glds": X.GLDS_CASES, "glds-ring": X.GLDS_RING_CASES, "halo": X.HALO_CASES,
    "dgrad-bn": [c[0] for c in X.DGRAD_BN_EXACT], "gather": X.WGRAD_GATHER_CASES,
}
CONV_IDS = [(fam, sh) for fam, tab in CONV_TABLES.items() for sh in tab]


@pytest.mark.parametrize("fam,shape", CONV_IDS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_conv_cases_meet_the_contract(fam, shape):
    c = X.conv_case(shape)
    wgrad_only = fam == "gather"
    if not wgrad_only:
        _check_coverage(c, c.wt, dgrad=True)
        _check_lo(c, c.lo_values(), X.BF16_MAX)
        # the epilogue's dm is a masked dx + addend: bounded by the unmasked value checked above
        for mode, add in ((2, False), (3, True)):
            assert c.dm(mode, add).abs().max() <= (c.dx + c.add).abs().max() + c.dx.abs().max()
        assert int((c.xa == 0).sum()) > 0 and int((c.x * c.sc + c.sh == 0).sum()) > 0  # the strict > 0 matters
        assert int((c.yb == 0).sum()) > 0  # y == 0 must mask in mode 2
    _check_f32(c, c.f32_magnitudes(dgrad=not wgrad_only))


@pytest.mark.parametrize("shape", X.WGRAD_HALO_CASES + X.WGRAD_DMA_CASES, ids=lambda s: "x".join(map(str, s)))
def test_wgrad_cases_meet_the_contract(shape):
    n, h, w, cin, cout = shape
    k = 3 if shape in X.WGRAD_HALO_CASES else 1
    c = X.wgrad_case(n, h, w, cin, cout, k, 1)
    _check_lo(c, {"x": c.x, "dy": c.dy, "dy_ap": c.dy_ap}, X.BF16_MAX)
    _check_f32(c, c.f32_magnitudes(dgrad=False))
    assert _is_int(c.dw) and _is_int(c.dw_ap)


@pytest.mark.parametrize("n,hw,w3,k1", [c[:4] for c in X.P1X1_STORED] + X.P1X1_YREC)
def test_p1x1_cases_meet_the_contract(n, hw, w3, k1):
    c = X.P1x1Case(n, hw, w3, k1)
    _check_coverage(c, c.w1, dgrad=True)
    _check_coverage(c, c.w3f, dgrad=False)
    _check_lo(c, c.lo_values(), X.BF16_MAX)
    _check_f32(c, c.f32_magnitudes())


@pytest.mark.parametrize("n,h,w", X.DGW_CASES)
def test_dgw_cases_meet_the_contract(n, h, w):
    c = X.conv_case((n, h, w, 64, 256, 1, 1))
    _check_coverage(c, c.wt, dgrad=True)
    a2 = c.x.clamp_min(0)  # the fused kernel's x operand is a ReLU output; y3 = conv3(a2) when recomputed
    y3 = X.conv_fwd(a2, c.wt, 1)
    dy = X.bn_bwd_apply(c.dy, y3, c.ca, c.cb, c.cc)
    dx = X.conv_dx(c.x.shape, c.wt, dy, 1)
    _check_lo(c, {**c.lo_values(fwd=False), "y3": y3, "dy(y3)": dy, "dx(y3)": dx, "dx(y3)+add": dx + c.add},
              X.BF16_MAX)
    _check_f32(c, c.f32_magnitudes())
    px = n * h * w
    assert px * float(dy.abs().max()) * 2 < X.F32_MAX  # dW over the recomputed-y3 dy
    assert float(((dx + c.add) * c.yb).abs().reshape(-1, 64).sum(0).max()) < X.F32_MAX


@pytest.mark.parametrize("shape", X.FP8_EXACT + X.X8_EXACT, ids=lambda s: "x".join(map(str, s)))
def test_fp8_cases_are_exact_in_mx_fp8(shape):
    """Quantising the operands to MX-fp8 (tightest E8M0 scale over 32 reduction elements, torch's e4m3 rounding)
    gives back the integers exactly, so the fp8 kernels are held to equality like the bf16 ones."""
    c = X.conv_case(shape)
    _check_coverage(c, c.wt, dgrad=True)
    _check_lo(c, c.lo_values(), X.BF16_MAX)
    _check_f32(c, c.f32_magnitudes(wgrad=False))
    ops = {"x": c.x, "xa": c.xa, "dy": c.dy, "dy_ap": c.dy_ap,
           "w fwd": c.wt.reshape(c.cout, -1), "w dgrad": c.wt.permute(3, 1, 2, 0).reshape(c.cin, -1)}
    for nm, t in ops.items():
        assert t.abs().max().item() <= X.FP8_MAX, (c, nm)
        assert torch.equal(X.mx_fp8_roundtrip(t), t), (c, nm, "not exact in MX-fp8")
    # the range the issue checked: blocks of 32 drawn from [-3, 3] and [-15, 15]
    g = X.gen(37)
    for hi in (3, 15):
        t = X.ints((64, 256), -hi, hi, g)
        assert torch.equal(X.mx_fp8_roundtrip(t), t)
    t = X.ints((64, 256), -17, 17, g)  # and the roundtrip helper does round: 17 needs five significant bits
    assert not torch.equal(X.mx_fp8_roundtrip(t), t)


@pytest.mark.parametrize("direction,shape", [("fwd", s) for s in X.INFER_FWD] + [("dgrad", s) for s in X.INFER_DGRAD],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_infer_cases_meet_the_contract(direction, shape):
    c = X.InferCase(*shape)
    _check_coverage(c, c.wt, dgrad=direction == "dgrad")
    if direction == "fwd":
        vals = {"y": c.y, "y+res": c.y + c.res, "x": c.x, "w": c.wt, "res": c.res}
        assert (c.y < 0).double().mean() > 0.2 and int((c.y == 0).sum()) >= 0  # ReLU matters
    else:
        vals = {"dx": c.dx, "dx+add": c.dx + c.add, "dy": c.dy, "w": c.wt, "mask": c.mask}
        assert int((c.mask == 0).sum()) > 0 and 0.2 < (c.mask > 0).double().mean() < 0.5
    _check_lo(c, vals, X.BF16_MAX)  # bf16's range: fp16 (2048) and fp32 hold it too
    # the split-K slabs are fp32 partial sums of the same terms
    assert float(c.wt.abs().reshape(c.cout, -1).sum(1).max() * 2 + 8) < X.F32_MAX


@pytest.mark.parametrize("n,h,w", X.STEM_CASES)
def test_stem_cases_meet_the_contract(n, h, w):
    c = X.StemCase(n, h, w)
    assert bool((c.wt != 0).all())  # dense
    assert c.y.abs().max() <= 147
    _check_lo(c, {"x": c.x, "w": c.wt, "y": c.y, "dy": c.dy, "dy_ap": c.dy_ap}, X.BF16_MAX)
    # fp32 outputs: dx (at most 16 taps x 64 filters a pixel) and dW (one term a pixel)
    assert 16 * 64 * float(c.dy_ap.abs().max()) < X.F32_MAX
    assert n * c.ho * c.wo * float(c.dy_ap.abs().max()) < X.F32_MAX
    assert _is_int(c.dx) and _is_int(c.dx_ap) and _is_int(c.dw) and _is_int(c.dw_ap)


def test_one_dropped_term_passes_the_tolerance_and_breaks_equality():
    """Why the exact tests exist. 512 -> 512 3x3 (4608 terms): on the tolerance tests' random-normal bf16 data,
    removing a single term of one output's reduction stays below their 1.5e-2 bound, so their assertion
    passes with the defect; on the integer case removing a non-zero term breaks equality."""
    n, hw, cin, cout, k = 2, 4, 512, 512, 3
    torch.manual_seed(0)
    x = torch.randn(n, hw, hw, cin).to(torch.bfloat16).double()
    w = (torch.randn(cout, k, k, cin) * (2.0 / (k * k * cin)) ** 0.5).to(torch.bfloat16).double()
    ref = X.conv_fwd(x, w, 1)
    # output (0, 1, 1, o): tap (r, s) reads x[0, r, s, :]; the worst single term over every o, tap and channel
    terms = torch.einsum("orsc,rsc->orsc", w, x[0, 0:3, 0:3, :])
    assert torch.allclose(terms.sum((1, 2, 3)), ref[0, 1, 1, :], atol=1e-9)
    bad = ref.clone()
    bad[0, 1, 1, 7] -= terms[7, 1, 1, 100]  # one term of one output
    e = X.rel(bad, ref)
    assert 0 < e < 1.5e-2, e  # today's assertion passes with the defect
    # and not by luck of the index: removing a single term stays below the bound for all but outlier terms
    hidden = (terms.abs() / ref.abs().max() < 1.5e-2).double().mean().item()
    assert hidden > 0.99, hidden
    c = X.conv_case((n, hw, hw, cin, cout, k, 1))
    iterms = torch.einsum("orsc,rsc->orsc", c.wt, c.x[0, 0:3, 0:3, :])
    assert torch.equal(iterms.sum((1, 2, 3)), c.y[0, 1, 1, :])
    o, r, s, ch = (int(v) for v in (iterms != 0).nonzero()[0])
    ibad = c.y.clone()
    ibad[0, 1, 1, o] -= iterms[o, r, s, ch]
    assert not torch.equal(ibad, c.y)
    assert X.rel(ibad, c.y) < 6e-2  # and the fp8 bound would have let it through as well


def test_assert_same_compares_values_and_sees_one_element():
    ref = torch.tensor([[0.0, 3.0], [-2.0, 256.0]], dtype=torch.float64)
    X.assert_same(torch.tensor([[-0.0, 3.0], [-2.0, 256.0]]).to(torch.bfloat16), ref, "signed zero")
    X.assert_same(ref.flatten().float(), ref, "another shape, same values")
    for bad in (torch.tensor([[0.0, 3.0], [-2.0, 255.0]]), torch.tensor([[0.0, float("nan")], [-2.0, 256.0]])):
        with pytest.raises(AssertionError, match="1 of 4 elements differ"):
            X.assert_same(bad, ref, "one element")
