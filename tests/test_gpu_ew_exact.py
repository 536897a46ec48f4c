"""GPU: the kernels of argus_amd/csrc/bn.hip (BatchNorm apply, backward reduce, backward apply, the two ticket
finalizes, max pool, average pool) held to equality with plain fp64 references on integer-valued operands, at every
launch geometry the training engine reaches (tests/ew_cases.py names them; tests/test_ew_exact_host.py proves on
the CPU that each case reaches its geometry and meets the range conditions that make equality the only right
answer). These kernels are the reference a dozen fused variants are held to bit for bit; this is their own anchor.

Every call goes through the C ABI. Every output buffer is pre-filled so that an unwritten element cannot compare
equal (NaN, 0xFF for mask and argmax bytes) and carries a guard band of the same fill after its last element that
must come back untouched. Values are compared, not bit patterns (-0.0 equals 0.0). The only bars that are not
equality are the one-ulp bounds of the finalizes, derived where they are used.
"""
import ctypes as C
import math

import pytest
import torch

import ew_cases as W
from argus_amd._lib import BF16, F16, F32, lib, ptr, stream

pytestmark = pytest.mark.gpu

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DT = {"fp32": F32, "bf16": BF16, "fp16": F16}
NAN = float("nan")
GUARD = 4096  # elements of the guard band after every output


class Out:
    """An output buffer of ``shape`` pre-filled with a sentinel, with a guard band of the same fill behind it."""

    def __init__(self, shape, dtype, cuda):
        self.n = math.prod(shape)
        self.bytes = dtype == torch.uint8
        self.raw = torch.full((self.n + GUARD,), 0xFF if self.bytes else NAN, dtype=dtype, device=cuda)
        self.t = self.raw[:self.n].view(tuple(shape))

    def band_untouched(self, *what):
        band = self.raw[self.n:]
        ok = (band == 0xFF).all() if self.bytes else torch.isnan(band).all()
        assert bool(ok), (*what, "wrote past the end of the buffer")


def _dev(t, dt, cuda):
    """An integer-valued fp64 tensor in the compute dtype on the GPU (exact: tests/test_ew_exact_host.py)."""
    return t.to(TDT[dt]).to(cuda).contiguous()


def _f32(t, cuda):
    return t.float().to(cuda).contiguous()


def _same(got, ref, cuda, *what):
    """Equality of values with the fp64 reference, compared on the device (tests/exact_cases.py: assert_same)."""
    W.assert_same(got, ref.to(cuda), *what)


def _pack(keep, E):
    """Mask bits as the kernels store them: E consecutive channels a byte (fp32 4, bf16 8), as fp64 byte values."""
    w = torch.pow(2.0, torch.arange(E, dtype=torch.float64, device=keep.device))
    return (keep.reshape(-1, E).double() * w).sum(1)


def _within_ulp(got, ref, *what):
    """|got - ref| <= one fp32 unit in the last place at ref."""
    g, r = got.double().cpu(), ref.double()
    bad = ~((g - r).abs() <= W.ulp32(r))
    assert not bool(bad.any()), (*what, int(bad.sum()), bad.nonzero()[:4].tolist(), g[bad][:4].tolist(), r[bad][:4].tolist())


EW_IDS = [f"C{c}-px{p}" for c, p, ro in W.EW_CASES if not ro]
EW_APPLY = [(c, p) for c, p, ro in W.EW_CASES if not ro]
RED_IDS = [f"C{c}-px{p}" for c, p, _ in W.EW_CASES]
EW_REDUCE = [(c, p) for c, p, _ in W.EW_CASES]


# ---- argus_bn_apply ---------------------------------------------------------------------------------------------
# (residual, residual scale / shift, relu, mask bits)
APPLY_FORMS = [(False, False, True, True), (True, False, True, True), (True, True, True, True),
               (True, True, False, False), (False, False, False, True), (False, False, True, False)]


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("C_,pixels", EW_APPLY, ids=EW_IDS)
def test_bn_apply_exact(cuda, C_, pixels, dt):
    """out = relu?(y * scale + shift [+ res * rsc + rsh]) and the mask bits of the stored output."""
    L = lib()
    c = W.ew_case(C_, pixels)
    E = W.ELEMS[dt]
    y, res = _dev(c.y, dt, cuda), _dev(c.res, dt, cuda)
    sc, sh, rsc, rsh = (_f32(v, cuda) for v in (c.scale, c.shift, c.rsc, c.rsh))
    for use_res, rs, do_relu, bits in APPLY_FORMS:
        what = ("bn_apply", dt, c, f"res={use_res} rsc={rs} relu={do_relu} bits={bits}")
        out = Out((pixels, C_), TDT[dt], cuda)
        mask = Out((pixels * C_ // E,), torch.uint8, cuda)
        L.bn_apply(DT[dt], pixels, C_, ptr(y), ptr(sc), ptr(sh), ptr(res) if use_res else None,
                   ptr(rsc) if rs else None, ptr(rsh) if rs else None, int(do_relu), ptr(out.t),
                   ptr(mask.t) if bits else None, stream())
        torch.cuda.synchronize()
        ref = c.out(use_res, rs, do_relu).to(cuda)
        _same(out.t, ref, cuda, *what, "out")
        out.band_untouched(*what, "out")
        if bits:
            _same(mask.t, _pack(ref > 0, E), cuda, *what, "mask bits")
        else:
            assert bool((mask.t == 0xFF).all()), (*what, "mask bits written without a mask_out")
        mask.band_untouched(*what, "mask bits")


# ---- argus_bn_bwd_reduce ----------------------------------------------------------------------------------------
def _mask_arg(c, mode, dt, E, cuda):
    if mode == 1:
        return _dev(c.msrc, dt, cuda)
    if mode == 3:
        return W.pack_bits(c.keep, E).to(cuda)
    return None


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("C_,pixels", EW_REDUCE, ids=RED_IDS)
def test_bn_bwd_reduce_exact(cuda, C_, pixels, dt):
    """Every partial row {sum dm, sum dm * xhat} equals the reference sum over that row's pixel range, the rows
    sum to the whole-tensor reference, and the rows past the returned count stay untouched."""
    L = lib()
    c = W.ew_case(C_, pixels)
    E = W.ELEMS[dt]
    geo = W.bwd_geometry(C_, E, pixels)
    rows = L.dll.argus_bn_bwd_rows(pixels, C_)
    assert rows == geo["rows"], (c, rows, geo)
    dz, y, y2 = _dev(c.dz, dt, cuda), _dev(c.y, dt, cuda), _dev(c.y2, dt, cuda)
    sc, sh, mu, istd, mu2, istd2 = (_f32(v, cuda) for v in (c.scale, c.shift, c.mean, c.invstd, c.mean2, c.invstd2))
    spare = 2  # rows past the returned count

    def check(part, mode, branch, what):
        s, t = c.terms(mode, branch)
        ref = torch.stack([W.row_sums(s, rows, geo["ppb"]), W.row_sums(t, rows, geo["ppb"])], -1)
        _same(part.t[:rows], ref, cuda, *what, "partial rows")
        _same(part.t[:rows].double().sum(0), torch.stack([s.sum(0), t.sum(0)], -1), cuda, *what, "sum over the rows")
        assert bool(torch.isnan(part.t[rows:]).all()), (*what, "rows past the returned count written")
        part.band_untouched(*what)

    for mode, dual in [(0, False), (1, False), (2, False), (3, False), (0, True), (1, True), (3, True)]:
        what = ("bn_bwd_reduce", dt, c, f"mode {mode}", "dual" if dual else "single")
        m = _mask_arg(c, mode, dt, E, cuda)
        p1, p2 = Out((rows + spare, C_, 2), torch.float32, cuda), Out((rows + spare, C_, 2), torch.float32, cuda)
        L.bn_bwd_reduce(DT[dt], pixels, C_, ptr(dz), mode, ptr(m), ptr(y), ptr(sc) if mode == 2 else None,
                        ptr(sh) if mode == 2 else None, ptr(mu), ptr(istd), ptr(p1.t), ptr(y2) if dual else None,
                        ptr(mu2) if dual else None, ptr(istd2) if dual else None, ptr(p2.t) if dual else None, stream())
        torch.cuda.synchronize()
        check(p1, mode, 0, what)
        if dual:
            check(p2, mode, 1, (*what, "branch 2"))
        else:
            assert bool(torch.isnan(p2.t).all())
    # a dual pass with the recomputed mask (mode 2) is refused
    p1, p2 = Out((rows, C_, 2), torch.float32, cuda), Out((rows, C_, 2), torch.float32, cuda)
    rc = L.dll.argus_bn_bwd_reduce(DT[dt], pixels, C_, ptr(dz), 2, None, ptr(y), ptr(sc), ptr(sh), ptr(mu), ptr(istd),
                                   ptr(p1.t), ptr(y2), ptr(mu2), ptr(istd2), ptr(p2.t), stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"bn_bwd_reduce" in L.dll.argus_last_error()
    assert bool(torch.isnan(p1.t).all()) and bool(torch.isnan(p2.t).all())


# ---- argus_bn_bwd_apply -----------------------------------------------------------------------------------------
# (mode, dual, dm_out)
BWD_APPLY_FORMS = [(0, False, True), (1, False, False), (2, False, True), (3, False, False), (0, True, False),
                   (1, True, True), (3, True, True)]


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("C_,pixels", EW_APPLY, ids=EW_IDS)
def test_bn_bwd_apply_exact(cuda, C_, pixels, dt):
    """dy = ca * dm + cb * y + cc with dm = mask ? dz : 0 (one or two branches), and dm itself when asked for."""
    L = lib()
    c = W.ew_case(C_, pixels)
    E = W.ELEMS[dt]
    dz, y, y2 = _dev(c.dz, dt, cuda), _dev(c.y, dt, cuda), _dev(c.y2, dt, cuda)
    sc, sh = _f32(c.scale, cuda), _f32(c.shift, cuda)
    ca, cb, cc, ca2, cb2, cc2 = (_f32(v, cuda) for v in (c.ca, c.cb, c.cc, c.ca2, c.cb2, c.cc2))
    for mode, dual, with_dm in BWD_APPLY_FORMS:
        what = ("bn_bwd_apply", dt, c, f"mode {mode}", "dual" if dual else "single", f"dm_out={with_dm}")
        m = _mask_arg(c, mode, dt, E, cuda)
        dy, dy2, dm = (Out((pixels, C_), TDT[dt], cuda) for _ in range(3))
        L.bn_bwd_apply(DT[dt], pixels, C_, ptr(dz), mode, ptr(m), ptr(y), ptr(sc) if mode == 2 else None,
                       ptr(sh) if mode == 2 else None, ptr(ca), ptr(cb), ptr(cc), ptr(dy.t),
                       ptr(dm.t) if with_dm else None, ptr(y2) if dual else None, ptr(ca2) if dual else None,
                       ptr(cb2) if dual else None, ptr(cc2) if dual else None, ptr(dy2.t) if dual else None, stream())
        torch.cuda.synchronize()
        _same(dy.t, c.dy(mode, 0), cuda, *what, "dy")
        if dual:
            _same(dy2.t, c.dy(mode, 1), cuda, *what, "dy2")
        else:
            assert bool(torch.isnan(dy2.t).all())
        if with_dm:
            _same(dm.t, c.dm(mode), cuda, *what, "dm_out")
        else:
            assert bool(torch.isnan(dm.t).all())
        for o in (dy, dy2, dm):
            o.band_untouched(*what)


# ---- argus_bn_bwd_finalize --------------------------------------------------------------------------------------
def _workspace(L, C_, cuda):
    return torch.zeros(L.dll.argus_bn_workspace_bytes(C_), dtype=torch.uint8, device=cuda)


def _counters_zero(ws, *what):
    assert not bool(ws[:W.BN_COUNTER_BYTES].any()), (*what, "ticket counters not reset")


@pytest.mark.parametrize("C_,rows", W.FIN_CASES)
def test_bn_bwd_finalize_exact(cuda, C_, rows):
    """dgamma / dbeta are integer column sums and ca a product of powers of two: exact. cb = -gi2 T / count and
    cc = -gi S / count + gi2 T / count * mean are evaluated in fp64 and rounded once by the kernel: within one fp32
    ulp of the same expressions in fp64 (with these operands each term takes its one rounding in the division,
    whatever the association)."""
    L = lib()
    f = W.BwdFinCase(C_, rows)
    part = _f32(f.part, cuda)
    gamma, mean, invstd = _f32(f.gamma, cuda), _f32(f.mean, cuda), _f32(f.invstd, cuda)
    ws = _workspace(L, C_, cuda)
    runs = []
    for call in range(2):
        outs = {nm: Out((C_,), torch.float32, cuda) for nm in ("dgamma", "dbeta", "ca", "cb", "cc")}
        L.bn_bwd_finalize(C_, rows, ptr(part), f.count, ptr(gamma), ptr(mean), ptr(invstd), ptr(outs["dgamma"].t),
                          ptr(outs["dbeta"].t), ptr(outs["ca"].t), ptr(outs["cb"].t), ptr(outs["cc"].t), ptr(ws), stream())
        torch.cuda.synchronize()
        what = ("bn_bwd_finalize", C_, rows, f"call {call}")
        _counters_zero(ws, *what)
        for nm in ("dgamma", "dbeta", "ca"):
            _same(outs[nm].t, f.ref[nm], cuda, *what, nm)
        for nm in ("cb", "cc"):
            _within_ulp(outs[nm].t, f.ref[nm], *what, nm)
        for nm, o in outs.items():
            o.band_untouched(*what, nm)
        runs.append({nm: o.t.clone() for nm, o in outs.items()})
    for nm in runs[0]:
        assert torch.equal(runs[0][nm].view(torch.int32), runs[1][nm].view(torch.int32)), (C_, rows, nm, "second call differs")


# ---- argus_bn_finalize ------------------------------------------------------------------------------------------
def _round32(v):
    """fp64 -> the nearest fp32, as fp64."""
    return v.float().double()


@pytest.mark.parametrize("counted", [False, True], ids=["tiles", "row-counts"])
@pytest.mark.parametrize("C_,rows", W.FIN_CASES)
def test_bn_finalize_exact(cuda, C_, rows, counted):
    """mean and invstd within one fp32 ulp of the fp64 merge (sum x^2 / M2 <= 2^10, so the merge's own error is
    far below an fp32 ulp and can only move a value across a rounding boundary); scale = gamma * invstd exact from
    the stored invstd; shift within 2^-23 (|beta| + |mean * scale|) of the fp64 value from the stored mean and
    scale (one rounding if the multiply-subtract is contracted, two if not); the running statistics with momentum
    0.5 the correctly rounded 0.5 old + 0.5 new (both products exact, one rounding); nbt + 1 a call."""
    L = lib()
    f = W.FwdFinCase(C_, rows, counted)
    m = f.merge
    buf = torch.zeros(rows * C_ * 2 + rows, dtype=torch.float32, device=cuda)
    buf[:rows * C_ * 2] = f.part.float().flatten().to(cuda)
    buf[rows * C_ * 2:].view(torch.int32).copy_(f.n.to(torch.int32).to(cuda))  # read in the row-count layout only
    gamma, beta = _f32(f.gamma, cuda), _f32(f.beta, cuda)
    ws = _workspace(L, C_, cuda)
    nbt = torch.zeros((), dtype=torch.int64, device=cuda)

    def call(rm, rv, what):
        outs = {nm: Out((C_,), torch.float32, cuda) for nm in ("mean", "invstd", "scale", "shift")}
        L.bn_finalize(C_, rows, f.tile_rows, ptr(buf), f.count, ptr(gamma), ptr(beta), C.c_float(f.eps), C.c_float(0.5),
                      ptr(rm), ptr(rv), ptr(nbt), ptr(outs["mean"].t), ptr(outs["invstd"].t), ptr(outs["scale"].t),
                      ptr(outs["shift"].t), ptr(ws), stream())
        torch.cuda.synchronize()
        _counters_zero(ws, *what)
        for nm, o in outs.items():
            o.band_untouched(*what, nm)
        return {nm: o.t.clone() for nm, o in outs.items()}

    what = ("bn_finalize", C_, rows, "row counts" if counted else "tiles")
    # 0. from zero running statistics: 0.5 * 0 + 0.5 * new is exact, so the call shows the fp32 mean / unbiased variance
    rm, rv = torch.zeros(C_, device=cuda), torch.zeros(C_, device=cuda)
    o0 = call(rm, rv, (*what, "call 0"))
    mean32, unb32 = o0["mean"].double().cpu(), 2.0 * rv.double().cpu()
    _within_ulp(o0["mean"], m["mean"], *what, "mean")
    _within_ulp(o0["invstd"], m["invstd"], *what, "invstd")
    _within_ulp(unb32, m["unbiased"], *what, "unbiased variance")
    W.assert_same(2.0 * rm.double().cpu(), mean32, *what, "running mean from 0")
    sc32 = o0["scale"].double().cpu()
    W.assert_same(sc32, (f.gamma.float() * o0["invstd"].cpu()).double(), *what, "scale")
    shift = f.beta - mean32 * sc32
    err = (o0["shift"].double().cpu() - shift).abs()
    assert bool((err <= 2.0 ** -23 * (f.beta.abs() + (mean32 * sc32).abs())).all()), (*what, "shift", err.max().item())
    assert int(nbt) == 1
    # 1., 2. from given running statistics, twice on the same workspace
    rm, rv = _f32(f.rm0, cuda), _f32(f.rv0, cuda)
    old_m, old_v = f.rm0, f.rv0
    for k in (1, 2):
        ok = call(rm, rv, (*what, f"call {k}"))
        for nm in o0:
            assert torch.equal(ok[nm].view(torch.int32), o0[nm].view(torch.int32)), (*what, nm, f"call {k} differs")
        old_m, old_v = _round32(0.5 * old_m + 0.5 * mean32), _round32(0.5 * old_v + 0.5 * unb32)
        W.assert_same(rm.double().cpu(), old_m, *what, f"running mean, call {k}")
        W.assert_same(rv.double().cpu(), old_v, *what, f"running var, call {k}")
        assert int(nbt) == 1 + k


# ---- max pool ---------------------------------------------------------------------------------------------------
MAXPOOL = [(s[:4], dt) for s in W.MAXPOOL_CASES for dt in s[4]]


@pytest.mark.parametrize("shape,dt", MAXPOOL, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_maxpool_exact(cuda, shape, dt):
    """Forward: relu(y * scale + shift) pooled 3x3/2, the argmax byte the first strict maximum in (r, t) scan order
    (4, the first valid tap, for an all-zero corner window). Backward: the scatter-add of the gradient by the
    library's own argmax, and by a hand-written argmax tensor that uses every byte value 0..8 (a byte naming a tap
    outside the image names a pixel no window covers: its gradient lands nowhere), so the gather is a function of
    the bytes and not of the forward."""
    L = lib()
    n, h, w, ch = shape
    c = W.maxpool_case(*shape)
    best, idx, _ = c.fwd
    what = ("maxpool", dt, c)
    y, sc, sh = _dev(c.y, dt, cuda), _f32(c.scale, cuda), _f32(c.shift, cuda)
    out, am = Out((n, c.ho, c.wo, ch), TDT[dt], cuda), Out((n, c.ho, c.wo, ch), torch.uint8, cuda)
    L.maxpool_fwd(DT[dt], n, h, w, ch, ptr(y), ptr(sc), ptr(sh), ptr(out.t), ptr(am.t), stream())
    torch.cuda.synchronize()
    _same(out.t, best, cuda, *what, "forward")
    _same(am.t, idx.double(), cuda, *what, "argmax bytes")
    corner = (best[:, 0, 0, :] == 0) & (idx[:, 0, 0, :] == 4)
    assert bool((am.t[:, 0, 0, :].cpu()[corner] == 4).all())
    out.band_untouched(*what, "forward")
    am.band_untouched(*what, "argmax bytes")
    for nm, dout, amax, ref in (("library argmax", c.dout, am.t, c.dz),
                                ("hand-written argmax", c.dout_hand, c.idx_hand.to(cuda), c.dz_hand)):
        dz = Out((n, h, w, ch), TDT[dt], cuda)
        g = _dev(dout, dt, cuda)
        L.maxpool_bwd(DT[dt], n, h, w, ch, ptr(g), ptr(amax), ptr(dz.t), stream())
        torch.cuda.synchronize()
        _same(dz.t, ref, cuda, *what, "backward", nm)
        dz.band_untouched(*what, "backward", nm)


# ---- average pool -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", W.AVG_FWD_DTYPES)
@pytest.mark.parametrize("n,hw,ch", W.AVG_FWD_CASES)
def test_avgpool_fwd_exact(cuda, n, hw, ch, dt):
    """feat = fp32(sum / hw): the sum of small integers is exact and the fp32 division rounds correctly."""
    L = lib()
    c = W.AvgCase(n, hw, ch)
    x = _dev(c.x, dt, cuda)
    feat = Out((n, ch), torch.float32, cuda)
    L.avgpool_fwd(DT[dt], n, hw, ch, ptr(x), ptr(feat.t), stream())
    torch.cuda.synchronize()
    _same(feat.t, c.feat, cuda, "avgpool_fwd", dt, (n, hw, ch))
    feat.band_untouched("avgpool_fwd", dt, (n, hw, ch))


AVG_BWD = [(s[:3], dt) for s in W.AVG_BWD_CASES for dt in s[3]]


@pytest.mark.parametrize("shape,dt", AVG_BWD, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_avgpool_bwd_exact(cuda, shape, dt):
    """dx = dfeat * fp32(1 / hw) rounded to the output type, at every pixel of the image."""
    L = lib()
    n, hw, ch = shape
    c = W.AvgCase(n, hw, ch)
    df = _f32(c.dfeat, cuda)
    dx = Out((n, hw, ch), TDT[dt], cuda)
    L.avgpool_bwd(DT[dt], n, hw, ch, ptr(df), ptr(dx.t), stream())
    torch.cuda.synchronize()
    _same(dx.t, c.dx(TDT[dt]).contiguous(), cuda, "avgpool_bwd", dt, shape)
    dx.band_untouched("avgpool_bwd", dt, shape)
