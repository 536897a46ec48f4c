"""GPU: every conv kernel variant the schedules launch, held to equality with an fp64 reference on integer-valued
operands (tests/exact_cases.py; tests/test_exact_host.py proves on the CPU that every case meets the range
conditions that make equality the only right answer). The tolerance tests (1.5e-2 for bf16, 6e-2 for fp8)
cannot see one dropped, duplicated or mis-indexed term of a long reduction; here it is a failed equality.

Every call goes through the C ABI. Values are compared, not bit patterns (-0.0 equals 0.0); outputs are pre-filled
with NaN so an unwritten element fails; every family asserts through the kernel timer that the intended
instantiation ran and prints the names it saw.
"""
import ctypes as C

import pytest
import torch

import exact_cases as X
from argus_amd._lib import BF16, F16, F32, FP8, BnBwdEpilogue, BnBwdPrologue, ConvDesc, lib, ptr, stream
from argus_amd.profiling import KernelTimer
from infer_shapes import conv_kernel_name, is_frozen_conv
from test_gpu_kernels import _deq_x8, _prep

pytestmark = pytest.mark.gpu

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16, "fp8": torch.bfloat16}
DT = {"fp32": F32, "bf16": BF16, "fp16": F16, "fp8": FP8}
NAN = float("nan")


def _cdesc(c, tuning=None):
    p = X.pad_of(c.k)
    d = ConvDesc(c.n, c.h, c.w, c.cin, c.cout, c.k, c.k, c.s, p, c.ho, c.wo, int(c.k == 7))
    return d.with_tuning(tuning)


def _dev(t, dt, cuda):
    """An integer-valued fp64 tensor in the compute dtype on the GPU (exact: tests/test_exact_host.py)."""
    return t.to(TDT[dt]).to(cuda).contiguous()


def _f32(t, cuda):
    return t.float().to(cuda).contiguous()


def _nan(shape, dtype, cuda):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=cuda)


def _same(got, ref, *what):
    """Equality of values with the fp64 reference (tests/exact_cases.py: assert_same)."""
    X.assert_same(got.double().cpu(), ref, *what)


def _names(timer):
    return sorted(timer.summary())


SEEN = {}


def _saw(family, names):
    SEEN.setdefault(family, set()).update(names)


def _report(family):
    print(f"\nexact[{family}] kernels: " + "; ".join(sorted(SEEN.get(family, ()))))


def _bits(keep, dt, cuda):
    return X.pack_bits(keep, 8 if dt != "fp32" else 4).to(cuda)


def _ones_zeros(c, cuda):
    return torch.ones(c, device=cuda), torch.zeros(c, device=cuda)


def _fwd(L, d, dt, c, x, wf, pro, cuda, kernel=None):
    """argus_conv_fwd with BN-statistics partials; returns (names, y, column sums of the partials' sum column)."""
    rows = L.dll.argus_conv_fwd_stat_rows(C.byref(d), DT[dt])
    y = _nan((c.n, c.ho, c.wo, c.cout), TDT[dt], cuda)
    stats = _nan((rows, c.cout, 2), torch.float32, cuda)
    sc, sh = (_f32(c.sc, cuda), _f32(c.sh, cuda)) if pro else (None, None)
    with KernelTimer(kernel) as t:
        L.conv_fwd(C.byref(d), DT[dt], ptr(x), ptr(wf), ptr(y), ptr(sc), ptr(sh), ptr(stats), stream())
    torch.cuda.synchronize()
    return _names(t), y, stats[..., 0].double().sum(0)


def _check_fwd(what, c, y, ssum, pro):
    ref = c.y_pro if pro else c.y
    _same(y, ref, what, "y")
    _same(ssum, ref.reshape(-1, c.cout).sum(0), what, "BN partials: sum column")  # integers: exact in any order


def _dgrads(L, d, dt, c, dy, wt, cuda, kernel=None):
    """argus_conv_dgrad plain, accumulated in place onto an integer buffer, and with a masked addend."""
    names = set()
    shape = (c.n, c.h, c.w, c.cin)
    add = _dev(c.add, dt, cuda)
    bits = _bits(c.keep, dt, cuda)
    outs = []
    for form in ("plain", "in place", "masked addend"):
        dx = add.clone() if form == "in place" else _nan(shape, TDT[dt], cuda)
        with KernelTimer(kernel) as t:
            L.conv_dgrad(C.byref(d), DT[dt], ptr(dy), ptr(wt), ptr(dx), None if form == "plain" else ptr(dx if form == "in place" else add),
                         ptr(bits) if form == "masked addend" else None, stream())
        torch.cuda.synchronize()
        names.update(_names(t))
        outs.append(dx)
    return sorted(names), outs


def _check_dgrads(what, c, outs):
    _same(outs[0], c.dx, what, "dgrad")
    _same(outs[1], c.dx + c.add, what, "dgrad accumulated in place")
    _same(outs[2], c.dx + c.add * c.keep, what, "dgrad + masked addend")


def _wgrad(L, d, dt, c, x, dy, cuda, pro=False, apply=False, kernel=None):
    wsb = L.dll.argus_conv_wgrad_workspace_bytes(C.byref(d), DT[dt])
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=cuda)
    dw = _nan((c.cout, c.k, c.k, c.cin), torch.float32, cuda)
    with KernelTimer(kernel) as t:
        if apply:
            ydy, ca, cb, cc = _dev(c.ydy, dt, cuda), _f32(c.ca, cuda), _f32(c.cb, cuda), _f32(c.cc, cuda)
            ap = BnBwdPrologue(ptr(ydy), ptr(ca), ptr(cb), ptr(cc), None)
            L.conv_wgrad_apply(C.byref(d), DT[dt], ptr(x), ptr(dy), C.byref(ap), ptr(dw), ptr(ws), wsb, stream())
        else:
            sc, sh = (_f32(c.sc, cuda), _f32(c.sh, cuda)) if pro else (None, None)
            L.conv_wgrad(C.byref(d), DT[dt], ptr(x), ptr(sc), ptr(sh), ptr(dy), ptr(dw), ptr(ws), wsb, stream())
        torch.cuda.synchronize()
    return _names(t), dw


# ---- 1. the register-staged implicit GEMM: fp32, bf16 and fp32 on the bf16x3 split arithmetic ---------------
IGEMM_ONLY = {8: 0, 10: 0, 11: 0, 43: 0, 45: 0, 47: 0}  # no glds / halo / persistent / LDS-DMA kernels
CTYPE = {"fp32": "float", "bf16": "__bf16", "bf16x3": "argus::f32x3"}


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
def test_igemm_exact(cuda, mode, tile):
    """All 22 conv shapes at n = 2 on igemm_kernel / wgrad_kernel with the row tile forced (keys 0 / 1 / 2):
    forward plain and with the BN+ReLU prologue (+ the sum column of the BN partials), data gradient plain /
    accumulated / masked addend, weight gradient plain and with the input prologue. bf16x3 (key 53 = 7) keeps
    small integers entirely in the hi part, so it is exact too."""
    L = lib()
    dt = "bf16" if mode == "bf16" else "fp32"
    ct = CTYPE[mode]
    tune = {0: tile, 1: tile, 2: tile, **IGEMM_ONLY, **({53: 7} if mode == "bf16x3" else {})}
    for shape in X.IGEMM_CASES:
        c = X.conv_case(shape)
        d = _cdesc(c, tune)
        what = (mode, tile, shape)
        tiles = [L.dll.argus_conv_launch_info(C.byref(d), DT[dt], p, None) % 1000000 for p in range(3)]
        assert tiles[0] // 1000 == tile and tiles[1] // 1000 == tile, (what, tiles)  # the forced row tile holds
        x, dy = _dev(c.x, dt, cuda), _dev(c.dy, dt, cuda)
        wf, wt = _prep(d, dt, _f32(c.wt, cuda), cuda)
        for pro in (False, True):
            names, y, ssum = _fwd(L, d, dt, c, x, wf, pro, cuda)
            bm, bn = divmod(tiles[0], 1000)
            want = f"argus::igemm_kernel<{ct}, {bm}, {bn}, false, {'true' if pro else 'false'},"
            assert len(names) == 1 and names[0].startswith(want), (what, "fwd", pro, names)
            _saw("igemm " + mode, names)
            _check_fwd((what, "prologue" if pro else "plain"), c, y, ssum, pro)
        names, outs = _dgrads(L, d, dt, c, dy, wt, cuda)
        bm, bn = divmod(tiles[1], 1000)
        assert names and all(nm.startswith(f"argus::igemm_kernel<{ct}, {bm}, {bn}, false, false,") for nm in names), \
            (what, "dgrad", names)
        _saw("igemm " + mode, names)
        _check_dgrads(what, c, outs)
        for pro in (False, True):
            names, dw = _wgrad(L, d, dt, c, x, dy, cuda, pro=pro)
            bm, bn = divmod(tiles[2], 1000)
            want = f"argus::wgrad_kernel<{ct}, {bm}, {bn}, false, {'true' if pro else 'false'},"
            assert any(nm.startswith(want) for nm in names), (what, "wgrad", names)
            _saw("igemm " + mode, names)
            _same(dw, c.dw_pro if pro else c.dw, what, "dW", "prologue" if pro else "plain")
    _report("igemm " + mode)


# ---- 2. the global->LDS implicit GEMM -----------------------------------------------------------------------
@pytest.mark.parametrize("minrows", ["default", 1])
@pytest.mark.parametrize("tile", [64, 128])
def test_glds_exact(cuda, tile, minrows):
    """igemm_glds_kernel forced on (keys 8 / 9; key 36 = 1 also serves the strided data gradients, whose phases
    have fewer than the default 1024 rows) at 64- and 128-row statistics partials: forward and data gradient
    plain / accumulated / masked addend. A shape the kernel does not serve runs the register-staged kernel,
    held to the same equality."""
    L = lib()
    tune = {0: tile, 1: tile, 8: 64, 9: 1, **({36: 1} if minrows == 1 else {})}
    served = {"fwd": 0, "dgrad": 0}
    for shape in X.GLDS_CASES:
        c = X.conv_case(shape)
        d = _cdesc(c, tune)
        what = ("glds", tile, minrows, shape)
        x, dy = _dev(c.x, "bf16", cuda), _dev(c.dy, "bf16", cuda)
        wf, wt = _prep(d, "bf16", _f32(c.wt, cuda), cuda)
        names, y, ssum = _fwd(L, d, "bf16", c, x, wf, False, cuda)
        on = [nm for nm in names if nm.startswith("argus::igemm_glds_kernel<")]
        if c.n * c.ho * c.wo >= 1024 and c.k * c.k * c.cin >= 64 and c.cout % 128 == 0:
            assert len(names) == 1 and on, (what, "fwd not on the glds kernel", names)
        served["fwd"] += bool(on)
        _saw("glds", names)
        _check_fwd(what, c, y, ssum, False)
        names, outs = _dgrads(L, d, "bf16", c, dy, wt, cuda)
        served["dgrad"] += any(nm.startswith("argus::igemm_glds_kernel<") for nm in names)
        _saw("glds", names)
        _check_dgrads(what, c, outs)
    assert served["fwd"] >= 2 and served["dgrad"] >= 1, served
    print(f"\nexact[glds] tile {tile} min rows {minrows}: served {served} of {len(X.GLDS_CASES)} shapes")
    _report("glds")


def test_glds_two_stage_ring_exact(cuda):
    """The two-stage ring of the data gradients (key 41 = 2) and the three-stage ring, plain and with the
    BN-backward epilogue (mask mode 2), on the shapes of test_glds_two_stage_ring_matches_three."""
    L = lib()
    for shape in X.GLDS_RING_CASES:
        c = X.conv_case(shape)
        per_ring = []
        for stages in (3, 2):
            d = _cdesc(c, {36: 1, 9: 1, 10: 0, 41: stages})
            what = ("glds ring", stages, shape)
            dy = _dev(c.dy, "bf16", cuda)
            _, wt = _prep(d, "bf16", _f32(c.wt, cuda), cuda)
            names, outs = _dgrads(L, d, "bf16", c, dy, wt, cuda)
            _check_dgrads(what, c, outs)
            n2, dm, parts = _dgrad_bn(L, d, "bf16", c, cuda, mode=2, dual=False, with_add=False, apply=False, store=False)
            _check_dgrad_bn(what, c, dm, parts, None, mode=2, dual=False, with_add=False, apply=False)
            names = sorted(set(names) | set(n2))
            assert names and all(nm.startswith("argus::igemm_glds_kernel<") and nm.endswith(f", {stages}>") for nm in names), \
                (what, names)
            _saw("glds ring", names)
            per_ring.append(names)
        assert not set(per_ring[0]) & set(per_ring[1]), per_ring  # two instantiations: the ring depth differs
    _report("glds ring")


# ---- 3. the LDS-halo 3x3 kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("deep", [0, 1])
@pytest.mark.parametrize("tile", [64, 128])
def test_halo_exact(cuda, tile, deep):
    """conv3x3_halo_kernel forced on (key 13 = 1) with the three- and the four-stage weight ring (key 51) at 64-
    and 128-row statistics partials: forward, data gradient plain / accumulated / masked addend; square frames
    and the non-square 16 x 32."""
    L = lib()
    tune = {0: tile, 1: tile, 13: 1, 51: deep}
    for shape in X.HALO_CASES:
        c = X.conv_case(shape)
        d = _cdesc(c, tune)
        what = ("halo", tile, deep, shape)
        x, dy = _dev(c.x, "bf16", cuda), _dev(c.dy, "bf16", cuda)
        wf, wt = _prep(d, "bf16", _f32(c.wt, cuda), cuda)
        names, y, ssum = _fwd(L, d, "bf16", c, x, wf, False, cuda)
        assert len(names) == 1 and names[0].startswith("argus::conv3x3_halo_kernel<"), (what, "fwd", names)
        _saw(f"halo deep={deep}", names)
        _check_fwd(what, c, y, ssum, False)
        names, outs = _dgrads(L, d, "bf16", c, dy, wt, cuda)
        assert names and all(nm.startswith("argus::conv3x3_halo_kernel<") for nm in names), (what, "dgrad", names)
        _saw(f"halo deep={deep}", names)
        _check_dgrads(what, c, outs)
    ring = {nm.endswith(", true>") for nm in SEEN[f"halo deep={deep}"]}
    assert (True in ring) == bool(deep), SEEN[f"halo deep={deep}"]  # the four-stage ring where the halo fits 384 positions
    _report(f"halo deep={deep}")


# ---- 4. data gradient with the BN-backward epilogue and / or the apply prologue ---------------------------------
def _dgrad_bn(L, d, dt, c, cuda, mode, dual, with_add, apply, store, epi=True):
    """argus_conv_dgrad_bn with mean 0, invstd 1 (xhat = y) and, in mask mode 2, scale 1, shift 0 (mask = y > 0).
    Returns (names, dm, (part, part2, dy_out))."""
    cin = c.cin
    rows = L.dll.argus_conv_dgrad_bn_rows(C.byref(d), DT[dt])
    part, part2 = _nan((rows, cin, 2), torch.float32, cuda), _nan((rows, cin, 2), torch.float32, cuda)
    one, zero = _ones_zeros(cin, cuda)
    yb, yb2 = _dev(c.yb, dt, cuda), _dev(c.yb2, dt, cuda)
    bits = _bits(c.keep, dt, cuda)
    e = BnBwdEpilogue()
    e.y, e.mean, e.invstd, e.mask_mode, e.part = ptr(yb), ptr(zero), ptr(one), mode, ptr(part)
    if mode == 2:
        e.scale, e.shift = ptr(one), ptr(zero)
    else:
        e.mask_bits = ptr(bits)
    if dual:
        e.y2, e.mean2, e.invstd2, e.part2 = ptr(yb2), ptr(zero), ptr(one), ptr(part2)
    dy = _dev(c.dy, dt, cuda)
    _, wt = _prep(d, dt, _f32(c.wt, cuda), cuda)
    shape = (c.n, c.h, c.w, c.cin)
    dm = _dev(c.add, dt, cuda) if with_add else _nan(shape, TDT[dt], cuda)
    dy_out = _nan(dy.shape, TDT[dt], cuda) if store else None
    pro = None
    if apply:
        ydy, ca, cb, cc = _dev(c.ydy, dt, cuda), _f32(c.ca, cuda), _f32(c.cb, cuda), _f32(c.cc, cuda)
        pro = BnBwdPrologue(ptr(ydy), ptr(ca), ptr(cb), ptr(cc), ptr(dy_out))
    with KernelTimer() as t:
        L.conv_dgrad_bn(C.byref(d), DT[dt], ptr(dy), ptr(wt), ptr(dm), ptr(dm) if with_add else None,
                        C.byref(e) if epi else None, C.byref(pro) if pro is not None else None, stream())
        torch.cuda.synchronize()
    return _names(t), dm, (part, part2, dy_out)


def _check_dgrad_bn(what, c, dm, parts, store, mode, dual, with_add, apply, epi=True):
    what = (what, f"mode {mode} dual {dual} addend {with_add} apply {apply} stored {store} epilogue {epi}")
    ref = c.dm(mode if epi else 0, with_add, apply)
    _same(dm, ref, what, "dm")
    part, part2, dy_out = parts
    if epi:  # both columns, summed over the rows: the per-row layout is the kernel's own
        _same(part.double().sum(0), X.ConvCase.partials(ref, c.yb), what, "partials {sum dm, sum dm*y}")
        if dual:
            _same(part2.double().sum(0), X.ConvCase.partials(ref, c.yb2), what, "second branch's partials")
    if store:
        _same(dy_out, c.dy_ap, what, "dy_out = ca*dm + cb*y + cc")


def _kname(tune, kname):
    if kname:
        return kname.split("<")[0]
    return "conv3x3_halo_kernel" if 13 in tune else ("igemm_glds_kernel" if 8 in tune else "igemm_kernel")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_dgrad_bn_exact(cuda, dt):
    """argus_conv_dgrad_bn on every kernel family its data gradient lands on (halo, glds, register-staged with
    strided and empty phases): mask mode 2 (y == 0 masks), mode 3 with packed bits, the dual branch, the integer
    addend; the apply prologue with dy stored and, where the kernel stages it itself, not stored; the prologue
    alone. dm, dy_out and both partial columns are exact."""
    L = lib()
    stages = set()
    for shape, tune, kname in X.DGRAD_BN_EXACT:
        fam = _kname(tune, kname)
        if dt == "fp32" and fam != "igemm_kernel":
            continue  # halo / glds are bf16 kernels
        c = X.conv_case(shape)
        d = _cdesc(c, {**tune, 43: 0})  # the persistent conv1 kernel has its own test
        what = ("dgrad_bn", dt, shape, fam)
        st = L.dll.argus_conv_dgrad_stages_prologue(C.byref(d), DT[dt])
        stages.add(st)
        forms = [(2, False, False, False, False, True), (3, False, True, False, False, True),
                 (3, True, True, False, False, True), (2, False, False, True, True, True),
                 (3, True, True, True, True, True), (0, False, False, True, True, False),
                 (0, False, True, True, True, False)]
        if st:  # dy never stored
            forms += [(2, False, False, True, False, True), (0, False, False, True, False, False)]
        for mode, dual, with_add, apply, store, epi in forms:
            names, dm, parts = _dgrad_bn(L, d, dt, c, cuda, mode or 2, dual, with_add, apply, store, epi)
            assert any(fam in nm for nm in names), (what, names)
            _saw("dgrad_bn " + fam, names)
            _check_dgrad_bn(what, c, dm, parts, store, mode, dual, with_add, apply, epi)
    assert stages == {0, 1}, stages  # the prologue staged by the kernel and materialised by the library
    for fam in ("igemm_kernel", "igemm_glds_kernel", "conv3x3_halo_kernel"):
        _report("dgrad_bn " + fam)


# ---- 5. the persistent conv1 data gradient -------------------------------------------------------------------
def _p1x1(L, c, cuda, key43, dual, with_add, rec, with_pro=True):
    d = ConvDesc(c.n, c.hw, c.hw, c.cout, c.k1, 1, 1, 1, 0, c.hw, c.hw, 0)  # conv1: 4*w3 -> k1; its dgrad: k1 -> 4*w3
    dk = d.with_tuning({43: key43, 49: 0})
    _, wt = _prep(d, "bf16", _f32(c.w1, cuda), cuda)
    P, cout = c.P, c.cout
    d3 = ConvDesc(c.n, c.hw, c.hw, c.w3, cout, 1, 1, 1, 0, c.hw, c.hw, 0)
    wf3, _ = _prep(d3, "bf16", _f32(c.w3f, cuda), cuda)
    a2, y3, yd = _dev(c.a2, "bf16", cuda), _dev(c.y3, "bf16", cuda), _dev(c.yd, "bf16", cuda)
    dm1, y1, dh = _dev(c.dm1, "bf16", cuda), _dev(c.y1, "bf16", cuda), _dev(c.dh, "bf16", cuda)
    ca, cb, cc = _f32(c.ca, cuda), _f32(c.cb, cuda), _f32(c.cc, cuda)
    bits = _bits(c.keep, "bf16", cuda)
    one, zero = _ones_zeros(cout, cuda)
    # partial rows: the library's count, the persistent kernel's row splits (<= 256), the igemm recompute's tiles
    rows = max(L.dll.argus_conv_dgrad_bn_rows(C.byref(dk), BF16), 256, (P + 63) // 64) + 8
    part, part2 = torch.zeros(rows, cout, 2, device=cuda), torch.zeros(rows, cout, 2, device=cuda)
    ws = torch.zeros(L.dll.argus_bn_workspace_bytes(cout), dtype=torch.uint8, device=cuda)
    fin = [_nan((cout,), torch.float32, cuda) for _ in range(10)]
    e = BnBwdEpilogue()
    e.mean, e.invstd, e.mask_mode, e.mask_bits, e.part = ptr(zero), ptr(one), 3, ptr(bits), ptr(part)
    e.workspace, e.gamma, e.dgamma, e.dbeta, e.ca, e.cb, e.cc = ptr(ws), ptr(one), *(ptr(t) for t in fin[:5])
    if dual:
        e.y2, e.mean2, e.invstd2, e.part2 = ptr(yd), ptr(zero), ptr(one), ptr(part2)
        e.gamma2, e.dgamma2, e.dbeta2, e.ca2, e.cb2, e.cc2 = ptr(one), *(ptr(t) for t in fin[5:])
    if rec:
        e.y_x, e.y_w, e.y_k = ptr(a2), ptr(wf3), c.w3
    else:
        e.y = ptr(y3)
    pro = BnBwdPrologue(ptr(y1), ptr(ca), ptr(cb), ptr(cc), None) if with_pro else None
    out = _nan((P, cout), torch.bfloat16, cuda)
    with KernelTimer() as t:
        L.conv_dgrad_bn(C.byref(dk), BF16, ptr(dm1), ptr(wt), ptr(out), ptr(dh) if with_add else None, C.byref(e),
                        C.byref(pro) if pro is not None else None, stream())
        torch.cuda.synchronize()
    assert int(ws[:16384].view(torch.int32).abs().sum()) == 0  # finalize counters left at zero
    return _names(t), out, part, part2


def _check_p1x1(what, c, out, part, part2, dual, with_add):
    ref = c.dm(with_add)
    _same(out, ref, what, "dm")
    _same(part.double().sum(0), X.ConvCase.partials(ref, c.y3), what, "partials {sum dm, sum dm*y3}")
    if dual:
        _same(part2.double().sum(0), X.ConvCase.partials(ref, c.yd), what, "downsample branch's partials")


@pytest.mark.parametrize("n,hw,w3,k1,dual", X.P1X1_STORED)
def test_p1x1_dgrad_exact(cuda, n, hw, w3, k1, dual):
    """p1x1_dgrad_kernel (key 43 = 1) reading the stored y3: apply prologue, addend, mask bits, optional downsample
    branch; dm and both partial columns of both branches exact; ragged row counts (hw = 5, 7, 9)."""
    L = lib()
    c = X.P1x1Case(n, hw, w3, k1)
    names, out, part, part2 = _p1x1(L, c, cuda, 1, dual, True, False)
    assert f"argus::p1x1_dgrad_kernel<{k1}, {4 if dual else 3}>" in names, names
    assert not any(nm.startswith("argus::igemm_kernel") for nm in names), names
    _saw("p1x1", names)
    _check_p1x1((c, dual), c, out, part, part2, dual, True)
    _report("p1x1")


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("n,hw,w3,k1", X.P1X1_YREC)
def test_p1x1_dgrad_y_recompute_exact(cuda, n, hw, w3, k1, dual, with_add):
    """The same data gradient with y3 = conv3(a2) rebuilt from y_x, y_w instead of read: on the persistent kernel
    at y_k = 64 (p1x1_dgrad_kernel<64, BW, true>), in the register-staged igemm's epilogue at y_k = 128. dm and
    the partials against y3 exact, so a wrong recomputed y3 shows in the second column."""
    L = lib()
    c = X.P1x1Case(n, hw, w3, k1)
    names, out, part, part2 = _p1x1(L, c, cuda, 1, dual, with_add, True, with_pro=w3 == 64)
    if w3 == 64:
        assert f"argus::p1x1_dgrad_kernel<64, {4 if dual else 3}, true>" in names, names
        assert not any(nm.startswith("argus::igemm_kernel") for nm in names), names
    else:
        assert any(nm.startswith("argus::igemm_kernel") for nm in names), names
        assert not any(nm.startswith("argus::p1x1_dgrad_kernel") for nm in names), names
    _saw("p1x1 y recompute", names)
    ref = (c.dx if w3 == 64 else X.conv_dx((c.n, c.hw, c.hw, c.cout), c.w1, c.dm1, 1)) + (c.dh if with_add else 0)
    ref = ref * c.keep
    _same(out, ref, c, "dm")
    _same(part.double().sum(0), X.ConvCase.partials(ref, c.y3), c, "partials {sum dm, sum dm*y3}")
    if dual:
        _same(part2.double().sum(0), X.ConvCase.partials(ref, c.yd), c, "downsample branch's partials")
    _report("p1x1 y recompute")


# ---- 6. the fused data + weight gradient of layer 1's conv3 -------------------------------------------------------
@pytest.mark.parametrize("n,h,w", X.DGW_CASES)
def test_fused_dgrad_wgrad_exact(cuda, n, h, w):
    """argus_conv_dgrad_wgrad_bn (64 -> 256, dgw1x1_kernel): with the mask-mode-2 epilogue, without it, and
    without it with the addend in place (the library takes an addend only without the epilogue), each reading the
    stored y3 and recomputing y3 = conv3(a2). dx, dW and the partial sums exact."""
    L = lib()
    c = X.conv_case((n, h, w, 64, 256, 1, 1))
    d = _cdesc(c)
    assert L.dll.argus_conv_dgrad_wgrad_ok(C.byref(d), BF16) == 1
    P, cin, cout = n * h * w, 64, 256
    a2r = c.x.clamp_min(0)  # a ReLU output
    wf, wt = _prep(d, "bf16", _f32(c.wt, cuda), cuda)
    a2, dm, yb = _dev(a2r, "bf16", cuda), _dev(c.dy, "bf16", cuda), _dev(c.yb, "bf16", cuda)
    ca, cb, cc = _f32(c.ca, cuda), _f32(c.cb, cuda), _f32(c.cc, cuda)
    one, zero = _ones_zeros(cin, cuda)
    for rec in (False, True):
        y3r = X.conv_fwd(a2r, c.wt, 1) if rec else c.ydy
        y3 = _dev(y3r, "bf16", cuda)
        dyr = X.bn_bwd_apply(c.dy, y3r, c.ca, c.cb, c.cc)
        dxr = X.conv_dx(c.x.shape, c.wt, dyr, 1)
        dwr = X.conv_dw(a2r, c.wt.shape, dyr, 1)
        for with_bn, with_add in ((True, False), (False, False), (False, True)):
            what = (c, "recomputed y3" if rec else "stored y3", "epilogue" if with_bn else "plain", "addend" if with_add else "")
            rows = L.dll.argus_conv_dgrad_wgrad_bn_rows(C.byref(d), BF16)
            part = _nan((rows, cin, 2), torch.float32, cuda)
            e = BnBwdEpilogue()
            e.y, e.mean, e.invstd, e.mask_mode, e.scale, e.shift, e.part = ptr(yb), ptr(zero), ptr(one), 2, ptr(one), \
                ptr(zero), ptr(part)
            pro = BnBwdPrologue(None if rec else ptr(y3), ptr(ca), ptr(cb), ptr(cc), None)
            dx = _dev(c.add, "bf16", cuda) if with_add else _nan((P, cin), torch.bfloat16, cuda)
            dw = _nan((cout, 1, 1, cin), torch.float32, cuda)
            wsw = torch.empty(L.dll.argus_conv_dgrad_wgrad_workspace_bytes(C.byref(d), BF16), dtype=torch.uint8,
                              device=cuda)
            with KernelTimer() as t:
                L.conv_dgrad_wgrad_bn(C.byref(d), BF16, ptr(dm), ptr(wt), ptr(a2), ptr(dx), ptr(dx) if with_add else None,
                                      C.byref(e) if with_bn else None, C.byref(pro), ptr(dw), ptr(wsw), wsw.numel(),
                                      stream())
                torch.cuda.synchronize()
            names = _names(t)
            want = f"argus::dgw1x1_kernel<{'true' if with_bn else 'false'}, {'true' if rec else 'false'}>"
            assert want in names, (what, names)
            _saw("fused dgrad+wgrad", names)
            ref = (dxr + (c.add if with_add else 0)) * (c.mask2 if with_bn else 1.0)
            _same(dx, ref, what, "dx")
            _same(dw, dwr, what, "dW")
            if with_bn:
                _same(part.double().sum(0), X.ConvCase.partials(ref, c.yb), what, "partials")
    _report("fused dgrad+wgrad")


# ---- 7. weight-gradient variants: bf16 operands, fp32 dW, dense integer operands --------------------------------
SPLIT_TARGETS = [None, 4, 2048]


def _split(target):
    return {} if target is None else {6: target, 12: target, 27: target}  # 1x1 / halo / register-staged 3x3


@pytest.mark.parametrize("target", SPLIT_TARGETS)
def test_wgrad_register_staged_exact(cuda, target):
    L = lib()
    for shape in X.IGEMM_CASES:
        c = X.conv_case(shape)
        d = _cdesc(c, {**IGEMM_ONLY, **_split(target)})
        x, dy = _dev(c.x, "bf16", cuda), _dev(c.dy, "bf16", cuda)
        names, dw = _wgrad(L, d, "bf16", c, x, dy, cuda)
        assert any(nm.startswith("argus::wgrad_kernel<__bf16,") for nm in names), (shape, names)
        _saw("wgrad register-staged", names)
        _same(dw, c.dw, "register-staged wgrad", shape, target)
        if c.s == 1 and c.k == 1:  # the apply form (argus_conv_wgrad_apply, non-stem)
            names, dw = _wgrad(L, d, "bf16", c, x, dy, cuda, apply=True)
            assert any(nm.startswith("argus::wgrad_kernel<__bf16,") and nm.endswith(", true>") for nm in names), (shape, names)
            _saw("wgrad register-staged", names)
            _same(dw, c.dw_ap, "register-staged wgrad, apply", shape, target)
    _report("wgrad register-staged")


@pytest.mark.parametrize("target", SPLIT_TARGETS)
def test_wgrad_halo_exact(cuda, target):
    """wgrad3x3_halo_kernel on whole-row tiles, whole images and the 84-, 168- and 21-wide frames, (47, 84) with a
    ragged last row block."""
    L = lib()
    for n, h, w, cin, cout in X.WGRAD_HALO_CASES:
        c = X.wgrad_case(n, h, w, cin, cout, 3, 1)
        d = _cdesc(c, {14: 1 << 20, **_split(target)})
        x, dy = _dev(c.x, "bf16", cuda), _dev(c.dy, "bf16", cuda)
        names, dw = _wgrad(L, d, "bf16", c, x, dy, cuda, kernel="argus::wgrad3x3_halo_kernel")
        assert len(names) == 1, ("halo wgrad not used", c, names)
        _saw("wgrad halo", names)
        _same(dw, c.dw, "halo wgrad", c, target)
    _report("wgrad halo")


@pytest.mark.parametrize("target", SPLIT_TARGETS)
def test_wgrad_dma_ring_exact(cuda, target):
    """wgrad_dma_kernel (key 45: 1 = 128 x 128 tiles, 2 / 3 = 128 x 256 where Cin % 256 == 0 with the apply /
    always), plain and staging the BN-backward apply from dm (argus_conv_wgrad_apply)."""
    L = lib()
    for n, h, w, cin, cout in X.WGRAD_DMA_CASES:
        c = X.wgrad_case(n, h, w, cin, cout)
        x, dy = _dev(c.x, "bf16", cuda), _dev(c.dy, "bf16", cuda)
        for key in (1, 2, 3):
            d = _cdesc(c, {45: key, **({} if target is None else {6: target})})
            for apply in (False, True):
                ap = "true" if apply else "false"
                names, dw = _wgrad(L, d, "bf16", c, x, dy, cuda, apply=apply, kernel=f"argus::wgrad_dma_kernel<{ap}")
                wide = key == 3 or (key == 2 and apply)
                want = 256 if wide and cin % 256 == 0 else 128
                assert names == [f"argus::wgrad_dma_kernel<{ap}, {want}, false, 0>"], (c, key, apply, names)
                _saw("wgrad LDS-DMA ring", names)
                _same(dw, c.dw_ap if apply else c.dw, "LDS-DMA wgrad", c, key, apply, target)
    _report("wgrad LDS-DMA ring")


@pytest.mark.parametrize("target", SPLIT_TARGETS)
def test_wgrad_dma_gather_stride2_exact(cuda, target):
    """The gathering LDS-DMA kernel (key 47 = 1) on the stride-2 1x1 and 3x3 weight gradients: odd and ragged
    frames, rows outside the image."""
    L = lib()
    for shape in X.WGRAD_GATHER_CASES:
        c = X.conv_case(shape)
        d = _cdesc(c, {47: 1, **({} if target is None else {6: target, 27: target})})
        x, dy = _dev(c.x, "bf16", cuda), _dev(c.dy, "bf16", cuda)
        names, dw = _wgrad(L, d, "bf16", c, x, dy, cuda, kernel="argus::wgrad_dma_kernel<false, 128, true, 0>")
        assert len(names) == 1, ("gather kernel not used", shape, names)
        _saw("wgrad gather", names)
        _same(dw, c.dw, "gather wgrad", shape, target)
    _report("wgrad gather")


# ---- 8. MX-fp8 ------------------------------------------------------------------------------------------------
def test_fp8_igemm_exact(cuda):
    """The register-staged MX-fp8 igemm (key 37 = 7: every pass): integers up to 15 are exact in e4m3 under any
    E8M0 block scale, so forward, data gradient with the epilogue and the 1x1 apply-prologue form are held to
    equality, and the fp8 weight copies dequantise to exactly the integer weights."""
    L = lib()
    for shape in X.FP8_EXACT:
        c = X.conv_case(shape)
        d = _cdesc(c, {37: 7, 43: 0})
        what = ("fp8", shape)
        wf, wt = _prep(d, "fp8", _f32(c.wt, cuda), cuda)
        _same(_deq_x8(wf, c.cout, c.k * c.k * c.cin)[0], c.wt.reshape(c.cout, -1), what, "fp8 forward weights")
        x = _dev(c.x, "bf16", cuda)
        names, y, ssum = _fwd(L, d, "fp8", c, x, wf, False, cuda, kernel="argus::igemm_kernel")
        assert any(nm.endswith(", 32>") for nm in names), (what, names)  # the fp8 variant ran
        _saw("fp8 igemm", names)
        _check_fwd(what, c, y, ssum, False)
        # data gradient with the mask-mode-2 epilogue
        rows = L.dll.argus_conv_dgrad_bn_rows(C.byref(d), FP8)
        part = _nan((rows, c.cin, 2), torch.float32, cuda)
        one, zero = _ones_zeros(c.cin, cuda)
        yb, dy = _dev(c.yb, "bf16", cuda), _dev(c.dy, "bf16", cuda)
        e = BnBwdEpilogue()
        e.y, e.mean, e.invstd, e.mask_mode, e.scale, e.shift, e.part = ptr(yb), ptr(zero), ptr(one), 2, ptr(one), \
            ptr(zero), ptr(part)
        dm = _nan(c.x.shape, torch.bfloat16, cuda)
        with KernelTimer("argus::igemm_kernel") as t:
            L.conv_dgrad_bn(C.byref(d), FP8, ptr(dy), ptr(wt), ptr(dm), None, C.byref(e), None, stream())
            torch.cuda.synchronize()
        names = _names(t)
        assert names and all(int(nm.rsplit(", ", 1)[1][:-1]) & 32 for nm in names), (what, names)  # the fp8 variant
        _saw("fp8 igemm", names)
        ref = c.dm(2, False)
        _same(dm, ref, what, "dm")
        _same(part.double().sum(0), X.ConvCase.partials(ref, c.yb), what, "partials")
        if c.k == 1:  # the BN-backward apply staged before the quantisation
            assert L.dll.argus_conv_dgrad_stages_prologue(C.byref(d), FP8) == 1
            ydy, ca, cb, cc = _dev(c.ydy, "bf16", cuda), _f32(c.ca, cuda), _f32(c.cb, cuda), _f32(c.cc, cuda)
            pro = BnBwdPrologue(ptr(ydy), ptr(ca), ptr(cb), ptr(cc), None)
            dx = _nan(c.x.shape, torch.bfloat16, cuda)
            with KernelTimer("argus::igemm_kernel") as t:
                L.conv_dgrad_bn(C.byref(d), FP8, ptr(dy), ptr(wt), ptr(dx), None, None, C.byref(pro), stream())
                torch.cuda.synchronize()
            names = _names(t)
            assert any(nm.endswith(", 48>") for nm in names), (what, names)  # fp8 | apply prologue
            _saw("fp8 igemm", names)
            _same(dx, c.dx_ap, what, "dgrad + apply prologue")
    _report("fp8 igemm")


def test_x8_exact(cuda):
    """MX-fp8 stored operands: argus_bn_apply_x8 / argus_bn_bwd_apply_x8 write an x8 copy that dequantises to
    exactly the integer tensor; argus_conv_fwd_x8 / argus_conv_dgrad_bn_x8 (the halo kernel's F8 variant) and the
    fp8 weight copies are exact."""
    L = lib()
    for shape in X.X8_EXACT:
        c = X.conv_case(shape)
        n, h, w, cin, cout = shape[:5]
        d = _cdesc(c, {37: 10, 13: 1})
        what = ("x8", shape)
        P = n * h * w
        assert L.dll.argus_conv_x8_ok(C.byref(d), 0) == 1
        wf, wd = _prep(d, "fp8", _f32(c.wt, cuda), cuda)
        _same(_deq_x8(wf, cout, 9 * cin)[0], c.wt.reshape(cout, -1), what, "fp8 forward weights")
        # forward: a = relu(x * scale + shift) with its x8 copy
        xin, sc, sh = _dev(c.x, "bf16", cuda), _f32(c.sc, cuda), _f32(c.sh, cuda)
        a = _nan(c.x.shape, torch.bfloat16, cuda)
        a8 = torch.zeros(P * cin * 33 // 32, dtype=torch.uint8, device=cuda)
        L.bn_apply_x8(P, cin, ptr(xin), ptr(sc), ptr(sh), None, None, None, 1, ptr(a), None, ptr(a8), stream())
        _same(a, c.xa, what, "bn_apply_x8 bf16 output")
        _same(_deq_x8(a8, P, cin)[0], c.xa.reshape(P, cin), what, "bn_apply_x8 x8 copy")
        rows = L.dll.argus_conv_fwd_stat_rows(C.byref(d), FP8)
        stats = _nan((rows, cout, 2), torch.float32, cuda)
        y = _nan((n, h, w, cout), torch.bfloat16, cuda)
        with KernelTimer("argus::conv3x3_halo_kernel") as t:
            L.conv_fwd_x8(C.byref(d), ptr(a8), ptr(wf), ptr(y), ptr(stats), stream())
            torch.cuda.synchronize()
        names = _names(t)
        assert any(nm.endswith(", true, false>") for nm in names), (what, names)
        _saw("x8 halo", names)
        _check_fwd(what, c, y, stats[..., 0].double().sum(0), True)
        if cout % 128:
            assert L.dll.argus_conv_x8_ok(C.byref(d), 1) == 0
            continue
        assert L.dll.argus_conv_x8_ok(C.byref(d), 1) == 1
        _same(_deq_x8(wd, cin, 9 * cout)[0].reshape(cin, 3, 3, cout), c.wt.permute(3, 1, 2, 0), what, "fp8 dgrad weights")
        # data gradient: dy = ca*dm + cb*y + cc with its x8 copy, then the mask-mode-2 epilogue
        dmz, ydy = _dev(c.dy, "bf16", cuda), _dev(c.ydy, "bf16", cuda)
        ca, cb, cc = _f32(c.ca, cuda), _f32(c.cb, cuda), _f32(c.cc, cuda)
        dy = _nan(dmz.shape, torch.bfloat16, cuda)
        dy8 = torch.zeros(P * cout * 33 // 32, dtype=torch.uint8, device=cuda)
        L.bn_bwd_apply_x8(P, cout, ptr(dmz), ptr(ydy), ptr(ca), ptr(cb), ptr(cc), ptr(dy), ptr(dy8), stream())
        _same(dy, c.dy_ap, what, "bn_bwd_apply_x8 bf16 output")
        _same(_deq_x8(dy8, P, cout)[0], c.dy_ap.reshape(P, cout), what, "bn_bwd_apply_x8 x8 copy")
        one, zero = _ones_zeros(cin, cuda)
        yb = _dev(c.yb, "bf16", cuda)
        ws = torch.zeros(L.dll.argus_bn_workspace_bytes(2048), dtype=torch.uint8, device=cuda)
        brows = L.dll.argus_conv_dgrad_bn_rows(C.byref(d), FP8)
        # zero-filled, not NaN: the row count is argus_conv_dgrad_bn's, the x8 halo kernel writes fewer rows; the
        # folded finalize below reads exactly the rows the kernel wrote, so an unwritten one shows in dgamma / dbeta
        part = torch.zeros(brows, cin, 2, device=cuda)
        coef = _nan((5, cin), torch.float32, cuda)
        e = BnBwdEpilogue()
        e.y, e.mean, e.invstd, e.mask_mode, e.scale, e.shift, e.part = ptr(yb), ptr(zero), ptr(one), 2, ptr(one), \
            ptr(zero), ptr(part)
        e.workspace, e.gamma, e.dgamma, e.dbeta = ptr(ws), ptr(one), ptr(coef[0]), ptr(coef[1])
        e.ca, e.cb, e.cc = ptr(coef[2]), ptr(coef[3]), ptr(coef[4])
        dm = _nan(c.x.shape, torch.bfloat16, cuda)
        with KernelTimer("argus::conv3x3_halo_kernel") as t:
            L.conv_dgrad_bn_x8(C.byref(d), ptr(dy8), ptr(wd), ptr(dm), C.byref(e), stream())
            torch.cuda.synchronize()
        names = _names(t)
        assert any(nm.endswith(", 2, 2, true, false>") for nm in names), (what, names)
        _saw("x8 halo", names)
        ref = c.dm(2, False, apply=True)
        _same(dm, ref, what, "x8 dm")
        want = X.ConvCase.partials(ref, c.yb)
        _same(part.double().sum(0), want, what, "x8 partials")
        # gamma 1, mean 0, invstd 1: dbeta = sum dm and dgamma = sum dm * y, integers below 2^24
        _same(coef[1], want[:, 0], what, "folded finalize: dbeta")
        _same(coef[0], want[:, 1], what, "folded finalize: dgamma")
        assert int(ws[:16384].count_nonzero()) == 0  # ticket counters left at zero
    _report("x8 halo")


# ---- 9. the frozen kernels --------------------------------------------------------------------------------------
def _only_conv(timer, want, launches):
    got = {n: v["launches"] for n, v in timer.summary().items() if is_frozen_conv(n)}
    assert got == {want: launches}, f"launched {got}, expected {launches} of {want}"


@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", X.INFER_FWD, ids=lambda s: "x".join(map(str, s)))
def test_conv_infer_exact(cuda, dt, shape):
    """argus_conv_infer with splits {1, 2, 3, max, default}, integer bias, with / without the integer residual and
    ReLU; w_fold given directly as the integer weights (the fold itself is pinned bit for bit elsewhere)."""
    L = lib()
    c = X.InferCase(*shape)
    d = _cdesc(c)
    x, wf, bias, res = _dev(c.x, dt, cuda), _dev(c.wt, dt, cuda), _f32(c.bias, cuda), _dev(c.res, dt, cuda)
    mx = L.dll.argus_conv_infer_max_splits(C.byref(d), DT[dt])
    assert mx == c.k * c.k * c.cin // (32 if dt == "fp32" else 64)
    ws = torch.zeros(max(L.dll.argus_conv_infer_workspace_bytes(C.byref(d), DT[dt], mx), 16), dtype=torch.uint8,
                     device=cuda)
    splits = sorted({min(s, mx) for s in (1, 2, 3, mx)}) + [0]
    with KernelTimer() as timer:
        for use_res in (False, True):
            for relu in (0, 1):
                ref = c.out(use_res, relu)
                for sp in splits:
                    out = _nan(ref.shape, TDT[dt], cuda)
                    L.conv_infer(C.byref(d), DT[dt], ptr(x), ptr(wf), ptr(bias), ptr(res) if use_res else None, relu,
                                 ptr(out), sp, ptr(ws), ws.numel(), stream())
                    _same(out, ref, shape, dt, f"res={use_res} relu={relu} splits={sp}")
    want = conv_kernel_name("fwd", dt, shape)
    _only_conv(timer, want, 4 * len(splits))
    print(f"\nexact[frozen fwd] {shape} {dt}: {want}, splits {splits}")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", X.INFER_DGRAD, ids=lambda s: "x".join(map(str, s)))
def test_conv_infer_dgrad_exact(cuda, dt, shape):
    """argus_conv_infer_dgrad (fp32 and bf16: the library serves no fp16 data gradient) with the same split sweep, with / without the addend and the mask (mask > 0; a third
    of the mask is exactly zero); pixels no tap reaches get the (masked) addend or zero."""
    L = lib()
    c = X.InferCase(*shape)
    d = _cdesc(c)
    dy, wfd = _dev(c.dy, dt, cuda), _dev(c.wt_dgrad, dt, cuda)
    addend, mask = _dev(c.add, dt, cuda), _dev(c.mask, dt, cuda)

    def plan(splits_in):
        sp, mx, nb = C.c_int(0), C.c_int(0), C.c_size_t(0)
        L.conv_infer_dgrad_plan(C.byref(d), DT[dt], splits_in, C.byref(sp), C.byref(mx), C.byref(nb))
        return sp.value, mx.value, nb.value

    mx = plan(0)[1]
    assert mx == c.k * c.k * c.cout // (32 if dt == "fp32" else 64)
    ws = torch.zeros(max(plan(mx)[2], 16), dtype=torch.uint8, device=cuda)
    splits = sorted({min(s, mx) for s in (1, 2, 3, mx)}) + [0]
    with KernelTimer() as timer:
        for use_mask in (False, True):
            for use_add in (False, True):
                ref = c.dx_out(use_add, use_mask)
                for sp in splits:
                    dx = _nan(ref.shape, TDT[dt], cuda)
                    L.conv_infer_dgrad(C.byref(d), DT[dt], ptr(dy), ptr(wfd), ptr(addend) if use_add else None,
                                       ptr(mask) if use_mask else None, ptr(dx), sp, ptr(ws), ws.numel(), stream())
                    _same(dx, ref, shape, dt, f"mask={use_mask} addend={use_add} splits={sp}")
    want = conv_kernel_name("dgrad", dt, shape)
    _only_conv(timer, want, 4 * len(splits))
    print(f"\nexact[frozen dgrad] {shape} {dt}: {want}, splits {splits}")


# ---- 10. the stem -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,W,served", [(3, 38, 30, False), (2, 100, 248, True)])
def test_stem_exact(cuda, n, H, W, served):
    """The 7x7 stride-2 stem with activations in {-1, 0, 1} and dense +-1 weights (147 terms): forward on the
    LDS-patch kernel and the implicit GEMM (key 19), weight gradient on the LDS-patch kernel and the register-
    staged kernel (key 34) plain and with the apply, argus_conv_stem_dgrad (fp32 output) with and without the
    apply prologue; 38 x 30 does not tile and keeps the implicit GEMM / wgrad_kernel."""
    L = lib()
    c = X.StemCase(n, H, W)
    ca, cb, cc = _f32(c.ca, cuda), _f32(c.cb, cuda), _f32(c.cc, cuda)
    for dt in ("bf16", "fp32"):
        d0 = _cdesc(c)
        img = _f32(c.x.permute(0, 3, 1, 2), cuda)
        x4 = torch.empty(n, H, W, 4, dtype=TDT[dt], device=cuda)
        L.images_to_nhwc4(DT[dt], n, H, W, ptr(img), ptr(x4), stream())
        wf = torch.empty(64, 256, dtype=TDT[dt], device=cuda)
        wm = _f32(c.wt, cuda)
        L.conv_weight_prep(C.byref(d0), DT[dt], ptr(wm), None, ptr(wf), None, stream())
        dy, ydy = _dev(c.dy, dt, cuda), _dev(c.ydy, dt, cuda)
        for key in ((1, 0) if dt == "bf16" else (0,)):
            d = _cdesc(c, {19: key, 34: key})
            what = ("stem", dt, (n, H, W), key)
            rows = L.dll.argus_conv_fwd_stat_rows(C.byref(d), DT[dt])
            buf = _nan((rows * 128 + rows,), torch.float32, cuda)  # partials (+ counts if ragged)
            y = _nan((n, c.ho, c.wo, 64), TDT[dt], cuda)
            with KernelTimer() as t:
                L.conv_fwd(C.byref(d), DT[dt], ptr(x4), ptr(wf), ptr(y), None, None, ptr(buf), stream())
                torch.cuda.synchronize()
            names = _names(t)
            assert ("argus::stem_fwd_kernel" in names) == (served and key == 1), (what, names)
            assert key == 1 and served or any(nm.startswith("argus::igemm_kernel<") for nm in names), (what, names)
            _saw("stem", names)
            _same(y, c.y, what, "y")
            _same(buf[:rows * 128].view(rows, 64, 2)[..., 0].double().sum(0), c.y.reshape(-1, 64).sum(0), what,
                  "BN partials: sum column")
            for apply in (False, True):
                wsb = L.dll.argus_conv_wgrad_workspace_bytes(C.byref(d), DT[dt])
                ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=cuda)
                dw = _nan((64, 7, 7, 3), torch.float32, cuda)
                with KernelTimer() as t:
                    if apply:
                        ap = BnBwdPrologue(ptr(ydy), ptr(ca), ptr(cb), ptr(cc), None)
                        L.conv_wgrad_apply(C.byref(d), DT[dt], ptr(x4), ptr(dy), C.byref(ap), ptr(dw), ptr(ws), wsb, stream())
                    else:
                        L.conv_wgrad(C.byref(d), DT[dt], ptr(x4), None, None, ptr(dy), ptr(dw), ptr(ws), wsb, stream())
                    torch.cuda.synchronize()
                names = _names(t)
                lds = f"argus::stem_wgrad_kernel<{'true' if apply else 'false'}>"
                assert (lds in names) == (served and key == 1), (what, apply, names)
                assert lds in names or any(nm.startswith("argus::wgrad_kernel<") for nm in names), (what, names)
                _saw("stem", names)
                _same(dw, c.dw_ap if apply else c.dw, what, "dW", "apply" if apply else "plain")
        for apply in (False, True):
            ap = BnBwdPrologue(ptr(ydy), ptr(ca), ptr(cb), ptr(cc), None)
            out = _nan((n, 3, H, W), torch.float32, cuda)
            with KernelTimer() as t:
                L.conv_stem_dgrad(C.byref(d0), DT[dt], ptr(dy), ptr(wf), C.byref(ap) if apply else None, ptr(out), stream())
                torch.cuda.synchronize()
            _saw("stem", _names(t))
            assert any("stem_dgrad" in nm for nm in _names(t)), _names(t)
            _same(out, (c.dx_ap if apply else c.dx).permute(0, 3, 1, 2).contiguous(), ("stem dgrad", dt, (n, H, W)),
                  "apply" if apply else "plain")
    _report("stem")
