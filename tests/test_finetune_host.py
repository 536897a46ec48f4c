"""CPU: the frozen fine-tuning surface without a GPU. The two entry points and the plan entry are declared,
bound and exported at ABI 21; every refusal names its reason before anything is launched (no compute call here
can reach a device: each returns from its argument checks); FineTuneSession's refusals; the two CLI flags."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from argus_amd._lib import BF16, F16, F32, FP8, LIB_PATH, SIGNATURES, ConvDesc, lib
from argus_amd.finetune import FineTuneSession

ROOT = Path(__file__).resolve().parents[1]
NEW = ("argus_bias_grad", "argus_bias_grad_plan", "argus_conv_fold_bn_bwd")
P16 = C.c_void_p(4096)  # an aligned non-NULL pointer no refused call dereferences


def _err():
    return lib().dll.argus_last_error().decode()


def test_symbols_are_declared_bound_and_exported_at_abi_21():
    hdr = (ROOT / "include" / "argus_hip.h").read_text()
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB_PATH)], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(rf"^int {name}\(", hdr, re.M), name
        assert name in SIGNATURES
        assert re.search(rf" T {name}$", out, re.M), name
    assert lib().dll.argus_abi_version() == 21
    assert "straight-through" in hdr and "in place" in hdr


def _plan(dt, P, K, s=0):
    sp, mx, nb = C.c_int(-1), C.c_int(-1), C.c_size_t(99)
    rc = lib().dll.argus_bias_grad_plan(dt, P, K, s, C.byref(sp), C.byref(mx), C.byref(nb))
    return rc, sp.value, mx.value, nb.value


def test_bias_grad_refusals():
    D = lib().dll
    for dt in (F16, FP8, 7, -1):
        assert _plan(dt, 128, 64)[0] != 0 and "dtype" in _err()
        assert D.argus_bias_grad(dt, 128, 64, P16, P16, 1, None, 0, None) != 0 and "dtype" in _err()
    assert D.argus_bias_grad(F32, 128, 64, None, P16, 1, None, 0, None) != 0 and "null" in _err()
    assert D.argus_bias_grad(F32, 128, 64, P16, None, 1, None, 0, None) != 0 and "null" in _err()
    assert D.argus_bias_grad_plan(F32, 128, 64, 0, None, None, None) != 0 and "null" in _err()
    for k in (0, 32, 96, 100):
        assert D.argus_bias_grad(BF16, 128, k, P16, P16, 1, None, 0, None) != 0
        assert ("multiple of 64" in _err()) if k else ("sizes" in _err())
    assert D.argus_bias_grad(BF16, 0, 64, P16, P16, 1, None, 0, None) != 0 and "sizes" in _err()
    for s, P in ((-1, 128), (65, 4096), (61, 60), (2, 1)):
        assert D.argus_bias_grad(F32, P, 64, P16, P16, s, P16, 1 << 20, None) != 0 and "splits" in _err()
        assert _plan(F32, P, 64, s)[0] != 0 and "splits" in _err()
    # a short or missing workspace, only where one is needed
    need = _plan(F32, 4096, 128, 4)[3]
    assert D.argus_bias_grad(F32, 4096, 128, P16, P16, 4, P16, need - 1, None) != 0 and "workspace" in _err()
    assert D.argus_bias_grad(F32, 4096, 128, P16, P16, 4, None, need, None) != 0 and "workspace" in _err()
    assert D.argus_bias_grad(F32, 4096, 128, P16, P16, 4, C.c_void_p(4100), need, None) != 0 and "aligned" in _err()
    assert D.argus_bias_grad(F32, 4096, 128, C.c_void_p(4100), P16, 1, None, 0, None) != 0 and "aligned" in _err()


def test_bias_grad_plan_follows_the_infer_workspace_layout():
    D = lib().dll
    # argus_conv_infer_workspace_bytes: 4096 bytes of tickets (up to 1024 tiles), then the slabs
    d = ConvDesc(2, 8, 8, 64, 64, 1, 1, 1, 0, 8, 8, 0)
    slab = 4 * 32 * 64 * 4  # 4 tiles of 32 rows x 64 columns, fp32
    assert D.argus_conv_infer_workspace_bytes(C.byref(d), F32, 2) == 4096 + 2 * slab
    for dt in (F32, BF16):
        for P, K in ((1, 64), (60, 64), (475, 2048), (4097, 192), (1 << 20, 64), (16384, 256)):
            rc, sp, mx, nb = _plan(dt, P, K)
            assert rc == 0 and mx == min(P, 64) and 1 <= sp <= mx
            assert nb == (0 if sp == 1 else 4096 + sp * K * 8)
            for s in (1, 2, mx):
                if s <= mx:
                    assert _plan(dt, P, K, s)[1:] == (s, mx, 0 if s == 1 else 4096 + s * K * 8)
    assert _plan(F32, 60, 64)[1] == 1 and _plan(F32, 1 << 20, 64)[1] == 64  # few pixels: no split; one column block: 64
    assert _plan(F32, 128, 65536 + 64)[0] != 0  # one ticket per column block in the 4096 bytes


def test_fold_bn_bwd_refusals():
    D = lib().dll
    d = ConvDesc(2, 8, 8, 64, 64, 3, 3, 1, 1, 8, 8, 0)
    args = [P16] * 4 + [C.c_float(1e-5)] + [P16] * 5
    call = lambda dd, a: D.argus_conv_fold_bn_bwd(dd, a[0], None, *a[1:], None)  # noqa: E731
    for i in (0, 1, 2, 3, 5, 6, 7, 8, 9):
        bad = list(args)
        bad[i] = None
        assert call(C.byref(d), bad) != 0 and "null" in _err(), i
    assert call(None, args) != 0 and "null" in _err()
    stem = ConvDesc(2, 8, 8, 3, 64, 7, 7, 2, 3, 4, 4, 1)
    c48 = ConvDesc(2, 8, 8, 48, 64, 1, 1, 1, 0, 8, 8, 0)
    for dd in (stem, c48):
        assert call(C.byref(dd), args) != 0 and _err()
    mis = list(args)
    mis[5] = C.c_void_p(4100)
    assert call(C.byref(d), mis) != 0 and "aligned" in _err()


def test_session_refusals():
    from argus_amd.models import NCameraCNN

    m = NCameraCNN().eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FineTuneSession(m, 2, (64, 64))
    for dt in ("fp16", "fp8", "bf16x3"):
        with pytest.raises(ValueError, match="fp32.*bf16"):
            FineTuneSession(m, 2, (64, 64), compute_dtype=dt)
    with pytest.raises(ValueError, match="bf16x3"):
        FineTuneSession(NCameraCNN(compute_dtype="bf16x3"), 2, (64, 64))
    with pytest.raises(ValueError, match="trainable"):
        FineTuneSession(m, 2, (64, 64), trainable="backbone")
    assert all(p.grad is None for p in m.parameters()) and "_finetune_state" not in m.__dict__  # nothing was touched


def test_cli_flags(tmp_path):
    from argus_amd.data import CameraCubePoseDatasetConfig
    from argus_amd.train import TrainConfig, parse_args

    ds = tmp_path / "ds"
    ds.mkdir()
    (ds / "ds.hdf5").write_bytes(b"")
    (ds / "img").mkdir()
    base = ["--dataset-config.dataset-path", str(ds), "--save-dir", str(tmp_path / "out")]
    cfg = parse_args(base)
    assert cfg.freeze_bn is False and cfg.init_checkpoint is None
    cfg = parse_args(base + ["--freeze-bn", "--init-checkpoint", "some/where.pth"])
    assert cfg.freeze_bn is True and cfg.init_checkpoint == "some/where.pth"
    with pytest.raises(SystemExit):
        parse_args(base + ["--freeze-bn", "--multigpu"])
    with pytest.raises(ValueError, match="single-process"):
        TrainConfig(dataset_config=CameraCubePoseDatasetConfig(dataset_path=str(ds)), save_dir=str(tmp_path / "out"),
                    freeze_bn=True, multigpu=True, num_gpus=2)
