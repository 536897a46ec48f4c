"""CPU: stage-wise frozen fine-tuning and the table-driven fold entries without a GPU. The three entry points are
declared, bound and exported at ABI 21; the table and both batch entries refuse bad arguments before anything is
launched (no call here reaches a device: each returns from its argument checks); FineTuneSession's and the CLI's
handling of ``trainable``."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from argus_amd._lib import BF16, F16, F32, FP8, LIB_PATH, SIGNATURES, ConvDesc, lib
from argus_amd.finetune import FineTuneSession

ROOT = Path(__file__).resolve().parents[1]
NEW = ("argus_conv_fold_bn_table", "argus_conv_fold_bn_batch", "argus_conv_fold_bn_bwd_batch")
P16 = 4096  # an aligned non-NULL pointer no refused call dereferences


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
    from argus_amd._lib import FOLD_ENTRY_BYTES

    assert re.search(rf"^#define ARGUS_CONV_FOLD_ENTRY_BYTES {FOLD_ENTRY_BYTES}$", hdr, re.M)
    # the per-conv entries stay exported
    for name in ("argus_conv_fold_bn", "argus_conv_fold_bn_dgrad", "argus_conv_fold_bn_bwd"):
        assert re.search(rf" T {name}$", out, re.M), name


def _src(descs, **over):
    from argus_amd._lib import FoldSrc

    src = (FoldSrc * len(descs))()
    for e, d in zip(src, descs):
        e.desc = d
        for f, _ in FoldSrc._fields_[1:]:
            if f not in ("strides", "eps"):
                setattr(e, f, P16)
        e.eps = 1e-5
    for k, v in over.items():
        setattr(src[len(descs) - 1], k, v)  # the last entry carries the fault
    return src


def _table(src, count=None, nbytes=None, host=True, nf=True, nb=True):
    from argus_amd._lib import FOLD_ENTRY_BYTES

    n = len(src) if count is None else count
    size = max(n, 1) * FOLD_ENTRY_BYTES if nbytes is None else nbytes
    buf = C.create_string_buffer(max(size, 1))
    a, b = C.c_int(-1), C.c_int(-1)
    rc = lib().dll.argus_conv_fold_bn_table(n, src, buf if host else None, size, C.byref(a) if nf else None,
                                            C.byref(b) if nb else None)
    return rc, a.value, b.value


def test_fold_table_plans_and_refuses():
    from argus_amd._lib import FOLD_ENTRY_BYTES

    d1 = ConvDesc(2, 8, 8, 64, 64, 1, 1, 1, 0, 8, 8, 0)
    d3 = ConvDesc(2, 8, 8, 128, 256, 3, 3, 2, 1, 4, 4, 0)
    rc, nf, nb = _table(_src([d1, d3]))
    # 64 x 64 tiles per tap of the fold, four filter rows per workgroup of the backward
    assert (rc, nf, nb) == (0, 1 + 2 * 4 * 9, 64 // 4 + 256 // 4), _err()
    # no backward operands in any entry: a table for the fold alone
    none = _src([d1, d3])
    for e in none:
        e.dwf = e.dw = e.db = e.dgamma = e.dbeta = None
    assert _table(none) == (0, 73, 0), _err()
    assert _table(_src([d1, d3], w_fold_dgrad=None))[0] == 0, _err()  # the second copy is optional
    # null arguments
    assert _table(_src([d1]), host=False)[0] != 0 and "null" in _err()
    assert _table(_src([d1]), nf=False)[0] != 0 and "null" in _err()
    assert _table(_src([d1]), nb=False)[0] != 0 and "null" in _err()
    assert lib().dll.argus_conv_fold_bn_table(1, None, C.create_string_buffer(256), 256, C.byref(C.c_int()),
                                              C.byref(C.c_int())) != 0 and "null" in _err()
    for f in ("w_master", "gamma", "beta", "running_mean", "running_var", "w_fold", "bias", "dwf", "dw", "db",
              "dgamma", "dbeta"):
        assert _table(_src([d1, d3], **{f: None}))[0] != 0 and "null" in _err(), f
    mixed = _src([d1, d3])
    e = mixed[0]
    e.dwf = e.dw = e.db = e.dgamma = e.dbeta = None  # the backward operands in one entry only
    assert _table(mixed)[0] != 0 and "null" in _err()
    # count, a short table
    for n in (0, -3):
        assert _table(_src([d1]), count=n)[0] != 0 and "count" in _err()
    assert _table(_src([d1, d3]), nbytes=2 * FOLD_ENTRY_BYTES - 1)[0] != 0 and "bytes" in _err()
    # what the fold does not serve: the stem, 48 channels
    stem = ConvDesc(2, 8, 8, 3, 64, 7, 7, 2, 3, 4, 4, 1)
    c48 = ConvDesc(2, 8, 8, 48, 64, 1, 1, 1, 0, 8, 8, 0)
    for bad in (stem, c48):
        assert _table(_src([d1, bad]))[0] != 0 and ("stem" in _err() or "multiples of 64" in _err()), _err()
    # alignment of what is stored in 16-byte pieces
    for f in ("dwf", "dw", "w_fold", "w_fold_dgrad"):
        assert _table(_src([d1, d3], **{f: 4100}))[0] != 0 and "aligned" in _err(), f


def test_fold_batch_refusals():
    D = lib().dll
    for dt in (F16, FP8, 7, -1):
        assert D.argus_conv_fold_bn_batch(dt, 2, P16, 8, None) != 0 and "dtype" in _err()
    for dt in (F32, BF16):
        assert D.argus_conv_fold_bn_batch(dt, 2, None, 8, None) != 0 and "null" in _err()
        assert D.argus_conv_fold_bn_batch(dt, 0, P16, 8, None) != 0 and "count" in _err()
        assert D.argus_conv_fold_bn_batch(dt, 2, P16, 0, None) != 0 and "nblocks" in _err()
    assert D.argus_conv_fold_bn_bwd_batch(2, None, 8, None) != 0 and "null" in _err()
    assert D.argus_conv_fold_bn_bwd_batch(0, P16, 8, None) != 0 and "count" in _err()
    assert D.argus_conv_fold_bn_bwd_batch(2, P16, 0, None) != 0 and "nblocks" in _err()  # a fold-only table's grid


def test_session_trainable_values():
    from argus_amd.finetune import TRAINABLE
    from argus_amd.models import NCameraCNN

    assert TRAINABLE == ("all", "head", "layer1", "layer2", "layer3", "layer4")
    m = NCameraCNN().eval()
    for t in ("layer1", "layer3", "layer4"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # accepted: the next check refuses the device
            FineTuneSession(m, 2, (64, 64), trainable=t)
    for t in ("layer5", "layer0", "backbone", "layer"):
        with pytest.raises(ValueError, match="trainable") as ei:
            FineTuneSession(m, 2, (64, 64), trainable=t)
        assert all(repr(v) in str(ei.value) for v in TRAINABLE)  # the message lists the accepted values
    assert all(p.grad is None for p in m.parameters()) and "_finetune_state" not in m.__dict__
    # a stage and everything behind it is a suffix of the parameters in model order, as the head is
    names = [n for n, _ in m.named_parameters()]
    assert [names.index(f"resnet.layer{k}.0.conv1.weight") for k in (1, 2, 3, 4)] == [3, 33, 72, 129]
    assert names.index("resnet.fc.weight") == 159 and len(names) == 167
    for k in (1, 2, 3, 4):
        i = names.index(f"resnet.layer{k}.0.conv1.weight")
        behind = tuple(f"resnet.layer{j}." for j in range(k, 5)) + ("resnet.fc.", "output_mlp.")
        assert all(n.startswith(behind) for n in names[i:]) and not any(n.startswith(behind) for n in names[:i])


def test_cli_trainable(tmp_path):
    from argus_amd.data import CameraCubePoseDatasetConfig
    from argus_amd.train import TrainConfig, parse_args

    ds = tmp_path / "ds"
    ds.mkdir()
    (ds / "ds.hdf5").write_bytes(b"")
    (ds / "img").mkdir()
    base = ["--dataset-config.dataset-path", str(ds), "--save-dir", str(tmp_path / "out")]
    cfg = parse_args(base)
    assert cfg.trainable == "all" and cfg.freeze_bn is False  # defaults unchanged
    assert parse_args(base + ["--freeze-bn"]).trainable == "all"
    cfg = parse_args(base + ["--freeze-bn", "--trainable", "layer4"])
    assert cfg.freeze_bn is True and cfg.trainable == "layer4"
    assert parse_args(base + ["--freeze-bn", "--trainable", "head"]).trainable == "head"
    assert parse_args(base + ["--trainable", "all"]).trainable == "all"
    with pytest.raises(SystemExit):
        parse_args(base + ["--trainable", "layer4"])  # only with --freeze-bn
    with pytest.raises(SystemExit):
        parse_args(base + ["--freeze-bn", "--trainable", "layer5"])
    dc = CameraCubePoseDatasetConfig(dataset_path=str(ds))
    with pytest.raises(ValueError, match="freeze-bn"):
        TrainConfig(dataset_config=dc, save_dir=str(tmp_path / "out"), trainable="layer2")
    with pytest.raises(ValueError, match="trainable"):
        TrainConfig(dataset_config=dc, save_dir=str(tmp_path / "out"), freeze_bn=True, trainable="stem")
