"""GPU: the table-driven folds (argus_conv_fold_bn_table, argus_conv_fold_bn_batch, argus_conv_fold_bn_bwd_batch).

Their contract is bit identity with the per-conv entries they stand for (argus_conv_fold_bn, argus_conv_fold_bn_dgrad,
argus_conv_fold_bn_bwd), which have their own accuracy tests (test_gpu_infer.py, test_gpu_frozen_grad.py,
test_gpu_finetune_kernels.py): every comparison here is of bit patterns, no tolerance. One table of four convs: the
two smallest kinds (one tile), a 1x1 with more channels out than in (several tiles, K != C) and the longest filter row
of the network, 3x3 512 -> 512 (4608); OHWI masters (NULL strides) mixed with OIHW-contiguous ones (explicit strides:
the gathered load path, and for the 1x1 convs the same memory as OHWI). Outputs are pre-filled with NaN, so an
element nobody wrote fails the comparison."""
import ctypes as C

import pytest
import torch

from argus_amd._lib import BF16, F32, FOLD_ENTRY_BYTES, ConvDesc, FoldSrc, lib, ptr, stream
from argus_amd.profiling import KernelTimer

pytestmark = pytest.mark.gpu

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
DT = {"fp32": F32, "bf16": BF16}
BITS = {"fp32": torch.int32, "bf16": torch.int16}
CONVS = [(64, 64, 1, "ohwi"), (64, 64, 3, "oihw"), (128, 256, 1, "oihw"), (512, 512, 3, "ohwi")]  # cin, cout, k, master
EPS = 1e-5


class _Conv:
    def __init__(self, cuda, gen, cin, cout, k, layout):
        p = 1 if k == 3 else 0
        self.d = ConvDesc(2, 8, 8, cin, cout, k, k, 1, p, 8, 8, 0)
        w = torch.randn(cout, cin, k, k, generator=gen)
        if layout == "ohwi":
            self.w, self.strides = w.permute(0, 2, 3, 1).contiguous().to(cuda), None
        else:
            self.w = w.to(cuda)
            self.strides = (C.c_int64 * 4)(*self.w.stride())
        self.gamma, self.var = [(0.5 + torch.rand(cout, generator=gen)).to(cuda) for _ in range(2)]
        self.beta, self.mean = [(0.3 * torch.randn(cout, generator=gen)).to(cuda) for _ in range(2)]
        self.dwf = torch.randn(cout, k * k * cin, generator=gen).to(cuda)
        self.db = torch.randn(cout, generator=gen).to(cuda)
        self.cin, self.cout, self.k = cin, cout, k

    def master(self):
        return ptr(self.w), self.strides, ptr(self.gamma), ptr(self.beta), ptr(self.mean), ptr(self.var), \
            C.c_float(EPS)


@pytest.fixture(scope="module")
def convs(cuda):
    gen = torch.Generator().manual_seed(520)
    return [_Conv(cuda, gen, *c) for c in CONVS]


def _bits(t):
    return t.view(BITS["fp32"] if t.dtype == torch.float32 else BITS["bf16"])


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _nan(cuda, *shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=cuda)


def _table(cuda, entries):
    """entries: dicts of FoldSrc fields (desc, strides and tensors). Returns (device table, count, nf, nb)."""
    n = len(entries)
    src = (FoldSrc * n)()
    for e, fields in zip(src, entries):
        for k, v in fields.items():
            if k == "strides":
                v = v if v is None else C.cast(v, C.POINTER(C.c_int64))
            elif k not in ("desc", "eps"):
                v = ptr(v)
            setattr(e, k, v)
    host = torch.zeros(n * FOLD_ENTRY_BYTES, dtype=torch.uint8)
    nf, nb = C.c_int(0), C.c_int(0)
    lib().conv_fold_bn_table(n, src, host.data_ptr(), host.numel(), C.byref(nf), C.byref(nb))
    return host.to(cuda), n, nf.value, nb.value


def _fold_fields(cv, wf, bias, wfd):
    return dict(desc=cv.d, w_master=cv.w, strides=cv.strides, gamma=cv.gamma, beta=cv.beta, running_mean=cv.mean,
                running_var=cv.var, eps=EPS, w_fold=wf, bias=bias, w_fold_dgrad=wfd)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_batched_fold_is_the_per_conv_folds_bit_for_bit(cuda, convs, dt):
    L = lib()
    want, got, entries = [], [], []
    for cv in convs:
        wf, bias = _nan(cuda, cv.cout, cv.k * cv.k * cv.cin, dtype=TDT[dt]), _nan(cuda, cv.cout)
        wfd = _nan(cuda, cv.cin, cv.k * cv.k * cv.cout, dtype=TDT[dt])
        L.conv_fold_bn(C.byref(cv.d), DT[dt], *cv.master(), ptr(wf), ptr(bias), stream())
        L.conv_fold_bn_dgrad(C.byref(cv.d), DT[dt], *cv.master(), ptr(wfd), stream())
        assert not (torch.isnan(wf).any() or torch.isnan(bias).any() or torch.isnan(wfd).any())
        want.append((wf, bias, wfd))
        got.append(tuple(torch.full_like(t, float("nan")) for t in (wf, bias, wfd)))
        entries.append(_fold_fields(cv, *got[-1]))
    entries[2]["w_fold_dgrad"] = None  # the third entry has no second copy: its buffer stays untouched
    table, n, nf, nb = _table(cuda, entries)
    assert nf == sum((cv.cout // 64) * (cv.cin // 64) * cv.k * cv.k for cv in convs) and nb == 0
    with KernelTimer() as timer:
        L.conv_fold_bn_batch(DT[dt], n, ptr(table), nf, stream())
    launches = {k: v["launches"] for k, v in timer.summary().items()}
    assert len(launches) == 1 and list(launches.values()) == [1] and "fold_bn_kernel_batch" in next(iter(launches))
    for i, ((wf, bias, wfd), (gf, gb, gd)) in enumerate(zip(want, got)):
        assert _same(gf, wf), i
        assert _same(gb, bias), i
        if i == 2:
            assert bool(torch.isnan(gd).all())
        else:
            assert _same(gd, wfd), i
    # a sub-table (the last two entries, all copies) from its own table call
    sub = [tuple(torch.full_like(t, float("nan")) for t in w) for w in want[2:]]
    table, n, nf, _ = _table(cuda, [_fold_fields(cv, *g) for cv, g in zip(convs[2:], sub)])
    L.conv_fold_bn_batch(DT[dt], n, ptr(table), nf, stream())
    for w, g in zip(want[2:], sub):
        assert all(_same(a, b) for a, b in zip(g, w))


def _bwd_reference(cv, db):
    """argus_conv_fold_bn_bwd out of place, and in place on a copy of dwf."""
    L, cuda = lib(), cv.dwf.device
    w, st, gamma, _, rm, rv, eps = cv.master()
    out = []
    for in_place in (False, True):
        src = cv.dwf.clone()
        dw = src if in_place else _nan(cuda, *cv.dwf.shape)
        dg, dbe = _nan(cuda, cv.cout), _nan(cuda, cv.cout)
        L.conv_fold_bn_bwd(C.byref(cv.d), w, st, gamma, rm, rv, eps, ptr(src), ptr(db), ptr(dw), ptr(dg), ptr(dbe),
                           stream())
        out.append((dw, dg, dbe))
    assert all(_same(a, b) for a, b in zip(*out))  # (the per-conv entry in place == out of place)
    return out[0]


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_batched_fold_backward_is_the_per_conv_entry_bit_for_bit(cuda, convs, in_place):
    L = lib()
    # entry 1 reads its db from entry 0's dbeta slot, which entry 0 rewrites in place over its own db, as the
    # downsample does under conv3 (both have 64 filters)
    shared = {1: 0}
    bufs, entries = [], []
    for i, cv in enumerate(convs):
        src = cv.dwf.clone()
        dw = src if in_place else _nan(cuda, *cv.dwf.shape)
        dg, dbe = _nan(cuda, cv.cout), (cv.db.clone() if i in shared.values() else _nan(cuda, cv.cout))
        bufs.append((src, dw, dg, dbe))
    for i, cv in enumerate(convs):
        src, dw, dg, dbe = bufs[i]
        db = bufs[shared[i]][3] if i in shared else (dbe if i in shared.values() else cv.db)
        f = _fold_fields(cv, _nan(cuda, 16), _nan(cuda, 16), None)  # (the backward never touches the fold's outputs)
        f.update(dwf=src, dw=dw, db=db, dgamma=dg, dbeta=dbe)
        entries.append(f)
    table, n, nf, nb = _table(cuda, entries)
    assert nb == sum(cv.cout // 4 for cv in convs)
    with KernelTimer() as timer:
        L.conv_fold_bn_bwd_batch(n, ptr(table), nb, stream())
    launches = {k: v["launches"] for k, v in timer.summary().items()}
    assert launches == {"argus::fold_bn_bwd_kernel_batch": 1}, launches
    for i, cv in enumerate(convs):
        want = _bwd_reference(cv, convs[shared[i]].db if i in shared else cv.db)
        _, dw, dg, dbe = bufs[i]
        for name, a, b in zip(("dw", "dgamma", "dbeta"), (dw, dg, dbe), want):
            assert _same(a, b), (i, name)
        assert bool(torch.isnan(entries[i]["w_fold"]).all())


def test_batched_fold_backward_of_a_sub_table(cuda, convs):
    L = lib()
    pick = [convs[3], convs[1]]
    bufs = [(cv.dwf.clone(), _nan(cuda, cv.cout), _nan(cuda, cv.cout)) for cv in pick]
    entries = []
    for cv, (src, dg, dbe) in zip(pick, bufs):
        f = _fold_fields(cv, _nan(cuda, 16), _nan(cuda, 16), None)
        f.update(dwf=src, dw=src, db=cv.db, dgamma=dg, dbeta=dbe)
        entries.append(f)
    table, n, _, nb = _table(cuda, entries)
    assert (n, nb) == (2, 512 // 4 + 64 // 4)
    L.conv_fold_bn_bwd_batch(n, ptr(table), nb, stream())
    for cv, got in zip(pick, bufs):
        assert all(_same(a, b) for a, b in zip(got, _bwd_reference(cv, cv.db)))
