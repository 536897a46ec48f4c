"""CPU: the frozen pose session's entry points (argus_stem_infer, argus_pool_fc_gelu, argus_pose_tail and the two
workspace queries) are declared, bound and exported, refuse every bad call through the error channel before
anything touches a device, and size their workspaces as include/argus_hip.h documents."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from argus_amd._lib import BF16, F16, F32, FP8, LIB_PATH, SIGNATURES, FrameSrc, lib

ROOT = Path(__file__).resolve().parents[1]
NEW = ["argus_pool_fc_gelu", "argus_pool_fc_gelu_workspace_bytes", "argus_pose_tail", "argus_pose_tail_workspace_bytes",
       "argus_stem_infer"]
P = C.c_void_p(4096)  # a non-null pointer no refused call may dereference
ERR_ARG = 1


def _err():
    return lib().dll.argus_last_error().decode()


def test_symbols_are_declared_bound_and_exported_at_abi_21():
    hdr = (ROOT / "include" / "argus_hip.h").read_text()
    declared = set(re.findall(r"^(?:int|size_t|const char\*)\s+(argus_[a-z0-9_]+)\(", hdr, re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (argus_[a-z0-9_]+)$", out, re.M))
    for name in NEW:
        assert name in declared and name in SIGNATURES and name in exported, name
    assert "argus_frame_src" in hdr
    assert lib().dll.argus_abi_version() == 21  # no bump: the symbol is the detection


def _src(**kw):
    # 2 planar images of 3 x 40 x 48, cropped to 32 x 40 at (4, 4)
    f = dict(base=4096, in_dtype=0, stride_img=3 * 40 * 48, stride_c=40 * 48, stride_y=48, stride_x=1, src_h=40,
             src_w=48, y0=4, x0=4)
    f.update(kw)
    return FrameSrc(*(f[k] for k, _ in FrameSrc._fields_))


def _stem(dtype=BF16, n=2, h=32, w=40, k=64, src=None, ptrs=(P, P, P, P)):
    s = _src() if src is None else src
    return lib().dll.argus_stem_infer(dtype, n, h, w, k, C.byref(s) if s is not False else None, *ptrs, None)


@pytest.mark.parametrize("dtype", [F32, FP8, 99])
def test_stem_infer_refuses_other_dtypes(dtype):
    assert _stem(dtype=dtype) == ERR_ARG and "dtype" in _err()


@pytest.mark.parametrize("kw", [dict(y0=9), dict(x0=9), dict(y0=-1), dict(src_h=35), dict(src_w=43)],
                         ids=["y0", "x0", "negative", "src_h", "src_w"])
def test_stem_infer_refuses_a_crop_outside_the_frame(kw):
    assert _stem(src=_src(**kw)) == ERR_ARG and "crop" in _err()


def test_stem_infer_refuses_bad_geometry_and_nulls():
    for in_dtype in (2, -1):
        assert _stem(src=_src(in_dtype=in_dtype)) == ERR_ARG and "in_dtype" in _err()
    assert _stem(src=False) == ERR_ARG and "null" in _err()
    assert _stem(src=_src(base=None)) == ERR_ARG and "null" in _err()
    for i in range(4):
        ptrs = [P] * 4
        ptrs[i] = None
        assert _stem(ptrs=ptrs) == ERR_ARG and "null" in _err()
    for kw in (dict(n=0), dict(h=7), dict(w=7), dict(k=128)):
        assert _stem(**kw) == ERR_ARG, kw
    # offsets of one image must fit the kernel's 32-bit index; negative strides are not served
    assert _stem(src=_src(stride_y=1 << 27, src_h=40)) == ERR_ARG and "31 bits" in _err()
    assert _stem(src=_src(stride_c=1 << 30)) == ERR_ARG and "31 bits" in _err()
    assert _stem(src=_src(stride_x=-1)) == ERR_ARG and "strides" in _err()


def test_workspace_queries():
    L = lib().dll
    # 256 bytes of tickets, then [column blocks of 128][slices of 64 channels][rows][128] floats
    assert L.argus_pool_fc_gelu_workspace_bytes(4, 2048, 1024) == 256 + 8 * 32 * 4 * 128 * 4
    assert L.argus_pool_fc_gelu_workspace_bytes(16, 2048, 64) == 256 + 1 * 32 * 16 * 128 * 4
    assert L.argus_pool_fc_gelu_workspace_bytes(1, 64, 129) == 256 + 2 * 1 * 1 * 128 * 4
    assert L.argus_pose_tail_workspace_bytes(2, 2048) == 256 + 32 * 2 * 128 * 4
    assert L.argus_pose_tail_workspace_bytes(16, 128) == 256 + 2 * 16 * 128 * 4
    for bad in ((17, 2048, 1024), (0, 2048, 1024), (2, 2000, 1024), (2, 2048, 0)):
        assert L.argus_pool_fc_gelu_workspace_bytes(*bad) == 0, bad
    for bad in ((17, 2048), (0, 2048), (2, 100)):
        assert L.argus_pose_tail_workspace_bytes(*bad) == 0, bad


def test_pool_fc_gelu_refuses_bad_calls():
    L = lib().dll
    need = L.argus_pool_fc_gelu_workspace_bytes(2, 2048, 1024)

    def call(dtype=BF16, n=2, hw=4, c=2048, ptrs=(P, P, P), rdim=1024, g0=P, ws=P, nbytes=need):
        return L.argus_pool_fc_gelu(dtype, n, hw, c, *ptrs, rdim, g0, ws, nbytes, None)

    for dtype in (F32, FP8, 99):
        assert call(dtype=dtype) == ERR_ARG and "dtype" in _err()
    assert call(n=17, nbytes=1 << 30) == ERR_ARG and "16 rows" in _err()
    assert call(n=0) == ERR_ARG
    assert call(nbytes=need - 1) == ERR_ARG and "workspace" in _err()
    assert call(ws=None) == ERR_ARG and "null" in _err()
    assert call(g0=None) == ERR_ARG and "null" in _err()
    for i in range(3):
        ptrs = [P] * 3
        ptrs[i] = None
        assert call(ptrs=ptrs) == ERR_ARG and "null" in _err()
    assert call(hw=0) == ERR_ARG and call(rdim=0) == ERR_ARG
    assert call(c=2000) != 0 and "multiple of 64" in _err()
    assert call(dtype=F16, nbytes=need - 1) == ERR_ARG and "workspace" in _err()  # fp16 is served: the next check fires


def test_pose_tail_refuses_bad_calls():
    L = lib().dll
    need = L.argus_pose_tail_workspace_bytes(2, 2048)

    def call(batch=2, d=2048, ptrs=(P,) * 9, ws=P, nbytes=need):
        return L.argus_pose_tail(batch, d, *ptrs, 0, ws, nbytes, None)

    assert call(batch=17, nbytes=1 << 30) == ERR_ARG and "batch 1..16" in _err()
    assert call(batch=0) == ERR_ARG
    assert call(nbytes=need - 1) == ERR_ARG and "workspace" in _err()
    assert call(ws=None) == ERR_ARG and "null" in _err()
    for i in range(9):
        ptrs = [P] * 9
        ptrs[i] = None
        assert call(ptrs=ptrs) == ERR_ARG and "null" in _err()
    assert call(d=0) == ERR_ARG
    assert call(d=100) != 0 and "multiple of 64" in _err()


def test_pose_session_has_no_cpu_fallback():
    from argus_amd.infer import InferenceSession
    from argus_amd.models import NCameraCNN
    from argus_amd.pose_session import PoseSession

    m = NCameraCNN()
    with pytest.raises(RuntimeError) as parent:
        InferenceSession(m, 1, (64, 64))
    with pytest.raises(RuntimeError) as ours:
        PoseSession(m, 1, (64, 64), compute_dtype="bf16")
    assert str(ours.value) == str(parent.value) and "HIP" in str(ours.value)
