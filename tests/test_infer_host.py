"""CPU: the frozen-inference additions to the C ABI (argus_conv_fold_bn, argus_conv_infer*) are declared,
bound and exported without an ABI bump, their host-side planning answers the documented shapes, bad calls
come back through the error channel, and InferenceSession rejects what it does not serve before any device
use. No compute call needs a GPU here."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
NEW = ["argus_conv_fold_bn", "argus_conv_infer", "argus_conv_infer_max_splits", "argus_conv_infer_splits",
       "argus_conv_infer_workspace_bytes"]
F32, BF16, FP8 = 0, 1, 2


def test_symbols_are_declared_bound_and_exported_at_abi_21():
    from argus_amd._lib import LIB_PATH, SIGNATURES, lib

    header = (ROOT / "include" / "argus_hip.h").read_text()
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (argus_[a-z0-9_]+)$", out, re.M))
    for name in NEW:
        assert re.search(rf"^(?:int|size_t)\s+{name}\(", header, re.M), name
        assert name in SIGNATURES and name in exported, name
    assert lib().dll.argus_abi_version() == 21


def test_split_planning():
    from argus_amd._lib import ConvDesc, lib

    D = lib().dll
    l4 = ConvDesc(2, 8, 8, 512, 512, 3, 3, 1, 1, 8, 8, 0)  # layer-4 3x3 at two images: M = 128
    big = ConvDesc(128, 64, 64, 64, 64, 1, 1, 1, 0, 64, 64, 0)
    stem = ConvDesc(2, 64, 64, 3, 64, 7, 7, 2, 3, 32, 32, 1)
    c48 = ConvDesc(2, 8, 8, 48, 64, 3, 3, 1, 1, 8, 8, 0)
    assert D.argus_conv_infer_splits(C.byref(l4), BF16) > 1
    assert D.argus_conv_infer_splits(C.byref(l4), BF16) <= D.argus_conv_infer_max_splits(C.byref(l4), BF16)
    assert D.argus_conv_infer_splits(C.byref(big), BF16) == 1 and D.argus_conv_infer_splits(C.byref(big), F32) == 1
    for d in (stem, c48):
        assert D.argus_conv_infer_splits(C.byref(d), BF16) == 0
        assert D.argus_conv_infer_splits(C.byref(d), F32) == 0
    # the k-step count: r*s*c over 64 bf16 / 32 fp32 elements
    assert D.argus_conv_infer_max_splits(C.byref(l4), BF16) == 9 * 512 // 64
    assert D.argus_conv_infer_max_splits(C.byref(l4), F32) == 9 * 512 // 32
    assert D.argus_conv_infer_max_splits(C.byref(big), BF16) == 1
    ws = [D.argus_conv_infer_workspace_bytes(C.byref(l4), BF16, s) for s in (0, 1, 2, 3, 8)]
    assert ws[0] == 0 and ws[1] == 0 and 0 < ws[2] < ws[3] < ws[4]
    assert ws[3] - ws[2] == (ws[4] - ws[3]) // 5  # tickets + splits * slabs
    assert ws[2] - 2 * (ws[3] - ws[2]) > 0  # the ticket words


DEPLOYED = [(1, (256, 256)), (2, (256, 256)), (1, (376, 672))]  # the sizes behind the README's latency figures


def test_every_kernel_class_of_a_deployed_session_is_in_the_parity_tables():
    """Every conv of a session plan at the deployed sizes, forward and data gradient, fp32 and 16-bit, classified
    as (direction, dtype group, kernel size, stride, tile rows by the Python mirror of infer_bm(), default splits
    > 1 from the library's own planning): each class must also occur among the kernel-parity shapes of the GPU
    tests, classified the same way. (The GPU tests hold the mirror to the kernel names the library launches.)"""
    import infer_shapes as S
    from argus_amd._lib import BF16, F16, F32, lib

    L = lib()
    code = {"fp32": F32, "bf16": BF16, "fp16": F16}
    served = {"fwd": ("fp32", "bf16", "fp16"), "dgrad": ("fp32", "bf16")}
    tables = {"fwd": S.FWD_PARITY, "dgrad": S.DGRAD_PARITY}
    have = {S.conv_class(L, direction, dt, code[dt], shape)
            for direction in tables for dt in served[direction] for shape in tables[direction]}
    missing, need = {}, set()
    for batch, hw in DEPLOYED:
        for name, shape in S.session_convs(batch, hw).items():
            for direction in tables:
                for dt in served[direction]:
                    cls = S.conv_class(L, direction, dt, code[dt], shape)
                    need.add(cls)
                    if cls not in have:
                        missing.setdefault(cls, f"{name} {shape} at {hw[0]}x{hw[1]}, B = {batch}, {dt}")
    assert len(S.session_convs(1, (256, 256))) == 52
    # what this guards: the deployed sizes do run 64-row tiles, of every kind, in both directions
    assert {c[:5] for c in need if c[4] == 64} == {
        (direction, grp, k, s, 64) for direction in tables for grp in ("fp32", "16-bit")
        for k, s in ((1, 1), (1, 2), (3, 1), (3, 2)) if (direction, k, s) != ("fwd", 3, 2)}
    assert not missing, "kernel classes of a deployed session that no parity shape runs:\n" + "\n".join(
        f"  {c}: e.g. {missing[c]}" for c in sorted(missing))


def test_the_tile_height_mirror_on_the_documented_thresholds():
    """infer_shapes.infer_bm at the two deployed shapes that sit exactly on the rule's threshold, their neighbours
    below, and a whole session: 128 x 128 at B = 2 is the smallest tested session that selects 64-row tiles."""
    import infer_shapes as S

    assert S.infer_bm(*S.gemm_mn("fwd", 2, 32, 32, 128, 512, 1, 1)) == 64   # 32 * 8 = 256
    assert S.infer_bm(*S.gemm_mn("fwd", 2, 32, 31, 128, 512, 1, 1)) == 32   # 31 * 8 = 248
    assert S.infer_bm(*S.gemm_mn("dgrad", 2, 64, 64, 128, 128, 3, 2)) == 64  # 128 * 2 = 256
    assert S.infer_bm(*S.gemm_mn("dgrad", 2, 64, 63, 128, 128, 3, 2)) == 32  # 126 * 2 = 252
    assert S.conv_kernel_name("fwd", "fp16", (2, 32, 32, 128, 512, 1, 1)) == "argus::conv_infer_kernel<_Float16, 64>"
    assert S.conv_kernel_name("dgrad", "bf16", (1, 6, 10, 64, 64, 1, 1)) == "argus::conv_infer_dgrad_kernel<__bf16, 32>"

    def rows(batch, hw):
        return {(direction, S.infer_bm(*S.gemm_mn(direction, *shape)))
                for shape in S.session_convs(batch, hw).values() for direction in ("fwd", "dgrad")}

    assert rows(2, (64, 64)) == rows(2, (72, 104)) == {("fwd", 32), ("dgrad", 32)}
    assert rows(2, (128, 128)) == {("fwd", 32), ("dgrad", 32), ("fwd", 64), ("dgrad", 64)}


def test_error_channel():
    from argus_amd._lib import ArgusHipError, ConvDesc, lib

    L = lib()
    d = ConvDesc(2, 8, 8, 512, 512, 3, 3, 1, 1, 8, 8, 0)
    p = C.c_void_p(16)
    rc = L.dll.argus_conv_infer(C.byref(d), FP8, p, p, p, None, 1, p, 1, None, 0, None)
    assert rc != 0 and b"dtype" in L.dll.argus_last_error()
    rc = L.dll.argus_conv_fold_bn(C.byref(d), 7, p, None, p, p, p, p, C.c_float(1e-5), p, p, None)
    assert rc != 0 and b"dtype" in L.dll.argus_last_error()
    mx = L.dll.argus_conv_infer_max_splits(C.byref(d), BF16)
    with pytest.raises(ArgusHipError, match="splits"):
        L.conv_infer(C.byref(d), BF16, 16, 16, 16, None, 1, 16, mx + 1, 256, 1 << 40, None)
    need = L.dll.argus_conv_infer_workspace_bytes(C.byref(d), BF16, 4)
    with pytest.raises(ArgusHipError, match="workspace"):
        L.conv_infer(C.byref(d), BF16, 16, 16, 16, None, 1, 16, 4, 256, need - 1, None)
    with pytest.raises(ArgusHipError, match="workspace"):
        L.conv_infer(C.byref(d), BF16, 16, 16, 16, None, 1, 16, 4, None, 0, None)
    c48 = ConvDesc(2, 8, 8, 48, 64, 3, 3, 1, 1, 8, 8, 0)
    with pytest.raises(ArgusHipError, match="multiples of 64"):
        L.conv_infer(C.byref(c48), BF16, 16, 16, 16, None, 1, 16, 1, None, 0, None)
    stem = ConvDesc(2, 64, 64, 3, 64, 7, 7, 2, 3, 32, 32, 1)
    with pytest.raises(ArgusHipError, match="stem"):
        L.conv_infer(C.byref(stem), BF16, 16, 16, 16, None, 1, 16, 1, None, 0, None)
    bad = ConvDesc(2, 8, 8, 64, 64, 3, 3, 1, 1, 7, 8, 0)  # wrong ho
    with pytest.raises(ArgusHipError, match="ho/wo"):
        L.conv_infer(C.byref(bad), F32, 16, 16, 16, None, 1, 16, 1, None, 0, None)


def test_session_rejects_cpu_models_and_unserved_dtypes():
    from argus_amd.infer import InferenceSession
    from argus_amd.models import NCameraCNN

    m = NCameraCNN()
    with pytest.raises(RuntimeError, match="HIP"):
        InferenceSession(m, 1, (64, 64))
    for dt in ("fp8", "bf16x3"):  # decided before any device use
        with pytest.raises(ValueError, match="'fp32' and 'bf16'"):
            InferenceSession(m, 1, (64, 64), compute_dtype=dt)
        with pytest.raises(ValueError, match="'fp32' and 'bf16'"):
            InferenceSession(NCameraCNN(compute_dtype=dt), 1, (64, 64))


def test_timing_cli_has_the_frozen_flag():
    import inspect

    from argus_amd import timing

    assert "frozen" in inspect.signature(timing.forward_latency).parameters
    assert '"--frozen"' in inspect.getsource(timing.main)
