"""CPU: the frozen-gradient additions to the C ABI (argus_conv_fold_bn_dgrad, argus_conv_infer_dgrad,
argus_conv_infer_dgrad_plan, argus_avgpool_bwd_relu) are declared, bound and exported without an ABI bump, the
plan answers the documented shapes, bad calls come back through the error channel before anything could be
launched, and GradientSession refuses what it does not serve before any device use. Nothing here needs a GPU."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
NEW = ["argus_conv_fold_bn_dgrad", "argus_conv_infer_dgrad", "argus_conv_infer_dgrad_plan", "argus_avgpool_bwd_relu"]
F32, BF16, FP8, F16 = 0, 1, 2, 3
ERR_ARG = 1


def _desc(n, h, w, cin, cout, k, s):
    from argus_amd._lib import ConvDesc

    p = 1 if k == 3 else 0
    return ConvDesc(n, h, w, cin, cout, k, k, s, p, (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1, 0)


def _plan(D, d, dtype, splits_in=0):
    sp, mx, nb = C.c_int(-1), C.c_int(-1), C.c_size_t(12345)
    rc = D.argus_conv_infer_dgrad_plan(C.byref(d), dtype, splits_in, C.byref(sp), C.byref(mx), C.byref(nb))
    return rc, sp.value, mx.value, nb.value


def test_symbols_are_declared_bound_and_exported_at_abi_21():
    from argus_amd._lib import LIB_PATH, SIGNATURES, lib

    header = (ROOT / "include" / "argus_hip.h").read_text()
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (argus_[a-z0-9_]+)$", out, re.M))
    for name in NEW:
        assert re.search(rf"^int\s+{name}\(", header, re.M), name
        assert name in SIGNATURES and name in exported, name
    assert lib().dll.argus_abi_version() == 21
    assert "argus/models.py:66-90" in header and "eval" in header  # the reference op the new entries replace


def test_plan():
    from argus_amd._lib import lib

    D = lib().dll
    # the five PARITY shapes of tests/test_gpu_infer.py, then a layer-3 and a layer-4 conv at n = 2
    shapes = [(1, 6, 10, 64, 64, 1, 1), (3, 5, 7, 192, 64, 3, 1), (2, 7, 9, 128, 192, 3, 2), (2, 9, 7, 256, 128, 1, 2),
              (2, 8, 8, 512, 512, 3, 1), (2, 16, 16, 256, 256, 3, 1), (2, 8, 8, 2048, 512, 1, 1)]
    split = 0
    for sh in shapes:
        d = _desc(*sh)
        rsk = sh[5] * sh[5] * sh[4]  # the reduction of a data gradient runs over the forward's output channels
        for dt, bke in ((BF16, 64), (F32, 32)):
            rc, sp, mx, nb = _plan(D, d, dt)
            assert rc == 0 and mx == rsk // bke and 1 <= sp <= mx, (sh, dt, rc, sp, mx)
            assert (nb == 0) == (sp <= 1), (sh, dt, sp, nb)
            split += sp > 1
            assert _plan(D, d, dt, 1) == (0, 1, mx, 0)
            if mx >= 2:
                rc2, sp2, _, nb2 = _plan(D, d, dt, 2)
                rcm, spm, _, nbm = _plan(D, d, dt, mx)
                assert (rc2, sp2, rcm, spm) == (0, 2, 0, mx) and 0 < nb2 <= nbm and nb2 % 16 == 0
            for bad in (-1, mx + 1):
                rc, *_ = _plan(D, d, dt, bad)
                assert rc == ERR_ARG and b"splits" in D.argus_last_error()
    assert split >= 4  # shapes that do split were covered, in both dtypes
    # the split workspace is tickets + splits * slabs, as the forward's
    l4 = _desc(2, 8, 8, 512, 512, 3, 1)
    ws = [_plan(D, l4, BF16, s)[3] for s in (2, 3, 8)]
    assert ws[1] - ws[0] == (ws[2] - ws[1]) // 5 and ws[0] - 2 * (ws[1] - ws[0]) > 0


def test_error_channel():
    from argus_amd._lib import ArgusHipError, lib

    L = lib()
    D = L.dll
    d = _desc(2, 8, 8, 512, 512, 3, 1)
    p = C.c_void_p(16)
    sp, mx, nb = C.c_int(0), C.c_int(0), C.c_size_t(0)
    outs = (C.byref(sp), C.byref(mx), C.byref(nb))

    def refused(rc, *words):
        msg = D.argus_last_error()
        assert rc != 0 and all(w in msg for w in words), (rc, msg)

    # dtypes: F16 through f16_unserved (ARGUS_ERR_ARG, "dtype" and "F16"), FP8 and unknown values by the entry itself
    for dt, words in ((F16, (b"dtype", b"F16")), (FP8, (b"dtype",)), (7, (b"dtype",))):
        refused(D.argus_conv_infer_dgrad(C.byref(d), dt, p, p, None, None, p, 1, None, 0, None), *words)
        refused(D.argus_conv_fold_bn_dgrad(C.byref(d), dt, p, None, p, p, p, p, C.c_float(1e-5), p, None), *words)
        refused(D.argus_conv_infer_dgrad_plan(C.byref(d), dt, 0, *outs), *words)
        refused(D.argus_avgpool_bwd_relu(dt, 2, 4, 2048, p, p, p, None), *words)
    assert D.argus_conv_infer_dgrad(C.byref(d), F16, p, p, None, None, p, 1, None, 0, None) == ERR_ARG
    # NULL pointers
    for args in ((None, BF16, p, p, None, None, p, 1, None, 0, None), (C.byref(d), BF16, None, p, None, None, p, 1, None, 0, None),
                 (C.byref(d), BF16, p, None, None, None, p, 1, None, 0, None), (C.byref(d), BF16, p, p, None, None, None, 1, None, 0, None)):
        refused(D.argus_conv_infer_dgrad(*args), b"null")
    refused(D.argus_conv_fold_bn_dgrad(C.byref(d), BF16, p, None, p, p, p, p, C.c_float(1e-5), None, None), b"null")
    refused(D.argus_conv_infer_dgrad_plan(C.byref(d), BF16, 0, None, C.byref(mx), C.byref(nb)), b"null")
    refused(D.argus_avgpool_bwd_relu(BF16, 2, 4, 2048, p, None, p, None), b"bad arguments")
    # shapes
    stem = _desc(2, 64, 64, 3, 64, 7, 2)
    stem.pad, stem.ho, stem.wo, stem.stem = 3, 32, 32, 1
    for bad, word in ((stem, "stem"), (_desc(2, 8, 8, 48, 64, 3, 1), "multiples of 64"),
                      (_desc(2, 8, 8, 64, 96, 1, 1), "multiples of 64")):
        with pytest.raises(ArgusHipError, match=word):
            L.conv_infer_dgrad(C.byref(bad), BF16, 16, 16, None, None, 16, 1, None, 0, None)
        with pytest.raises(ArgusHipError, match=word):
            L.conv_infer_dgrad_plan(C.byref(bad), BF16, 0, *outs)
        with pytest.raises(ArgusHipError, match=word):
            L.conv_fold_bn_dgrad(C.byref(bad), BF16, 16, None, 16, 16, 16, 16, C.c_float(1e-5), 16, None)
    from argus_amd._lib import ConvDesc

    wrong = ConvDesc(2, 8, 8, 64, 64, 3, 3, 1, 1, 7, 8, 0)  # wrong ho
    with pytest.raises(ArgusHipError, match="ho/wo"):
        L.conv_infer_dgrad(C.byref(wrong), F32, 16, 16, None, None, 16, 1, None, 0, None)
    # splits and workspace
    _, _, mxv, _ = _plan(D, d, BF16)
    for bad in (-1, mxv + 1):
        with pytest.raises(ArgusHipError, match="splits"):
            L.conv_infer_dgrad(C.byref(d), BF16, 16, 16, None, None, 16, bad, 256, 1 << 40, None)
    need = _plan(D, d, BF16, 4)[3]
    with pytest.raises(ArgusHipError, match="workspace"):
        L.conv_infer_dgrad(C.byref(d), BF16, 16, 16, None, None, 16, 4, 256, need - 1, None)  # short
    with pytest.raises(ArgusHipError, match="workspace"):
        L.conv_infer_dgrad(C.byref(d), BF16, 16, 16, None, None, 16, 4, None, 0, None)  # missing
    with pytest.raises(ArgusHipError, match="aligned"):
        L.conv_infer_dgrad(C.byref(d), BF16, 16, 16, None, None, 16, 4, 264, need, None)  # misaligned
    with pytest.raises(ArgusHipError, match="channels"):
        L.avgpool_bwd_relu(BF16, 2, 4, 2044, 16, 16, 16, None)


def test_session_refuses_cpu_models_and_unserved_dtypes():
    from argus_amd.infer import InferenceSession
    from argus_amd.infer_grad import SERVED, GradientSession
    from argus_amd.models import NCameraCNN

    assert SERVED == ("fp32", "bf16") and issubclass(GradientSession, InferenceSession)
    m = NCameraCNN()
    with pytest.raises(RuntimeError, match="HIP"):
        GradientSession(m, 1, (64, 64))
    for dt in ("fp16", "fp8", "bf16x3"):  # decided before any device use
        with pytest.raises(ValueError, match="'fp32' and 'bf16'"):
            GradientSession(m, 1, (64, 64), compute_dtype=dt)
    for dt in ("fp8", "bf16x3"):
        with pytest.raises(ValueError, match="'fp32' and 'bf16'"):
            GradientSession(NCameraCNN(compute_dtype=dt), 1, (64, 64))
    for name in ("vjp", "image_gradient", "refresh"):
        assert callable(getattr(GradientSession, name))
    import inspect

    assert list(inspect.signature(GradientSession.__init__).parameters)[1:] == \
        ["model", "batch", "hw", "compute_dtype", "graph", "debug"]


def test_the_session_module_does_not_import_the_oracle():
    for name in ("infer.py", "infer_grad.py"):
        assert not re.search(r"^\s*(?:from|import)\s+oracle\b", (ROOT / "argus_amd" / name).read_text(), re.M), name
