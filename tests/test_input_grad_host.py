"""CPU: the image-gradient entry point's host side. argus_conv_stem_dgrad is exported and bound, validates
its arguments through the error channel before anything touches a device, the ABI version and the policy
table are unchanged, and the Python seams reject what they do not serve without a GPU."""
import ctypes as C
import inspect

import pytest
import torch

from argus_amd._lib import ABI_VERSION, BF16, F32, FP8, BnBwdPrologue, ConvDesc, lib


def _stem(n=2, h=32, w=32):
    return ConvDesc(n, h, w, 3, 64, 7, 7, 2, 3, (h - 1) // 2 + 1, (w - 1) // 2 + 1, 1)


def _call(d, dtype, dy=16, w=16, ap=None, dx=16):
    L = lib()
    rc = L.dll.argus_conv_stem_dgrad(C.byref(d), dtype, dy, w, C.byref(ap) if ap is not None else None, dx, None)
    return rc, L.dll.argus_last_error().decode()


def test_symbol_abi_and_policy_unchanged():
    from argus_amd._lib import SIGNATURES

    L = lib()
    assert "argus_conv_stem_dgrad" in SIGNATURES
    assert ABI_VERSION == 21 and L.dll.argus_abi_version() == 21
    assert L.dll.argus_conv_policy_default(52) == -1
    assert L.dll.argus_conv_policy_default(54) == -1  # one kernel per dtype: no new policy key


def test_stem_dgrad_rejects_bad_arguments():
    rc, msg = _call(ConvDesc(2, 8, 8, 64, 64, 3, 3, 1, 1, 8, 8, 0), BF16)  # not a stem descriptor
    assert rc != 0 and "stem descriptor" in msg
    rc, msg = _call(ConvDesc(2, 32, 32, 3, 128, 7, 7, 2, 3, 16, 16, 1), BF16)  # a stem of 128 channels
    assert rc != 0 and "stem descriptor" in msg
    rc, msg = _call(ConvDesc(2, 32, 32, 3, 64, 7, 7, 2, 3, 15, 16, 1), BF16)  # wrong ho
    assert rc != 0 and "ho/wo" in msg
    rc, msg = _call(ConvDesc(2, 32, 32, 3, 64, 7, 7, 2, 3, 16, 17, 1), F32)  # wrong wo
    assert rc != 0 and "ho/wo" in msg
    for dtype in (FP8, 7, -1):  # unserved dtypes
        rc, msg = _call(_stem(), dtype)
        assert rc == 1 and "dtype" in msg, dtype
    for kw in ({"dy": None}, {"w": None}, {"dx": None}):
        rc, msg = _call(_stem(), BF16, **kw)
        assert rc == 1 and "null" in msg, kw
    L = lib()
    assert L.dll.argus_conv_stem_dgrad(None, BF16, 16, 16, None, 16, None) == 1
    assert b"null" in L.dll.argus_last_error()
    for ap in (BnBwdPrologue(None, 16, 16, 16, None), BnBwdPrologue(16, None, 16, 16, None),
               BnBwdPrologue(16, 16, None, 16, None), BnBwdPrologue(16, 16, 16, None, None)):
        rc, msg = _call(_stem(), F32, ap=ap)
        assert rc == 1 and "apply" in msg
    rc, msg = _call(_stem().with_tuning({52: 1}), BF16)  # key 52 stays unknown
    assert rc != 0 and "unknown tuning key 52" in msg


def test_python_seams_signatures():
    from argus_amd.engine import ResNetEngine
    from argus_amd.step import FusedTrainer
    from argus_amd.utils import image_gradient

    sig = inspect.signature(ResNetEngine.backward)
    assert list(sig.parameters)[-2:] == ["on_ready", "dx"] and sig.parameters["dx"].default is None
    sig = inspect.signature(FusedTrainer.step)
    assert list(sig.parameters) == ["self", "images", "targets", "image_grad"]
    assert sig.parameters["image_grad"].default is None
    assert list(inspect.signature(image_gradient).parameters) == ["model", "images", "target"]
    doc = image_gradient.__doc__
    assert "Train-mode" in doc and "no eval-mode backward" in doc and "left untouched" in doc


def test_reference_bf16_distance_is_usable():
    """The bar of test_gpu_input_grad.py::test_image_grad_bf16 is 4 x this distance: it must be a number."""
    from tests.input_grad_reference import reference_bf16_distance

    d = reference_bf16_distance()
    print(f"reference x.grad, bf16 autocast vs fp32 (B=2, 64x64): {d:.3e}")
    assert d == d and 0 < d < float("inf")


def test_no_cpu_fallback_for_the_image_gradient():
    from argus_amd.models import NCameraCNN
    from argus_amd.utils import image_gradient

    m = NCameraCNN()
    with pytest.raises(RuntimeError, match="HIP"):
        image_gradient(m, torch.rand(1, 6, 32, 32), torch.zeros(1, 7))
