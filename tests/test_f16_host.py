"""CPU: the fp16 frozen-inference additions. ARGUS_F16 = 3 joins the dtype enum without an ABI bump, the
split planning answers fp16 exactly as bf16, every entry point that does not serve fp16 refuses it before it
could launch anything, and the session / timing / validate plumbing accepts the new choice. Nothing here
needs a GPU; the rejection sweep refuses to run where there is one."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
F32, BF16, FP8, F16 = 0, 1, 2, 3
ERR_ARG = 1

# the entry points a frozen fp16 forward calls (include/argus_hip.h, ARGUS_F16): nothing else serves it
SERVED = {"argus_images_to_nhwc4", "argus_images_u8_to_nhwc4", "argus_conv_weight_prep", "argus_conv_fwd",
          "argus_maxpool_fwd", "argus_avgpool_fwd", "argus_conv_fold_bn", "argus_conv_infer",
          "argus_conv_infer_splits", "argus_conv_infer_max_splits", "argus_conv_infer_workspace_bytes"}
# Planning queries do not return a status: a non-zero return would read as a row count, a byte count or
# "yes". They answer ARGUS_F16 with the value they already give for a conv they do not serve, and set the error.
QUERIES = {"argus_conv_fwd_stat_rows": 0, "argus_conv_fwd_stat_tile": 0, "argus_conv_fwd_stats_only_rows": 0,
           "argus_conv_fwd_stats_only_tile": 0, "argus_conv_fwd_stat_part_bytes": 0, "argus_conv_launch_info": -1,
           "argus_conv_dgrad_bn_rows": -1, "argus_conv_dgrad_stages_prologue": 0, "argus_conv_dgrad_wgrad_ok": 0,
           "argus_conv_dgrad_wgrad_workspace_bytes": 0, "argus_conv_dgrad_wgrad_bn_rows": -1,
           "argus_conv_wgrad_workspace_bytes": 0, "argus_maxpool_bwd_bn_rows": -1}


def _dtype_functions():
    """name -> index of the `int dtype` parameter, for every prototype of the header that has one."""
    header = (ROOT / "include" / "argus_hip.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = {}
    for name, params in re.findall(r"^(?:int|size_t)\s+(argus_\w+)\(([^;]*?)\);", header, re.M | re.S):
        names = [p.strip() for p in params.split(",")]
        for i, p in enumerate(names):
            if re.fullmatch(r"int\s+dtype", p):
                out[name] = i
    return out


def test_constants_and_split_planning():
    from argus_amd import _lib
    from argus_amd._lib import ConvDesc, lib

    assert _lib.F16 == 3 and (_lib.F32, _lib.BF16, _lib.FP8) == (0, 1, 2)
    D = lib().dll
    assert D.argus_abi_version() == 21
    header = (ROOT / "include" / "argus_hip.h").read_text()
    assert re.search(r"ARGUS_F16\s*=\s*3\b", header)

    def desc(n, h, w, cin, cout, k, s):
        p = 1 if k == 3 else 0
        return ConvDesc(n, h, w, cin, cout, k, k, s, p, (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1, 0)

    # the five PARITY shapes of tests/test_gpu_infer.py, then a layer-3 and a layer-4 conv at B = 1, 256 x 256
    # (two cameras: n = 2; 16 x 16 and 8 x 8 feature maps)
    shapes = [(1, 6, 10, 64, 64, 1, 1), (3, 5, 7, 192, 64, 3, 1), (2, 7, 9, 128, 192, 3, 2), (2, 9, 7, 256, 128, 1, 2),
              (2, 8, 8, 512, 512, 3, 1), (2, 16, 16, 256, 256, 3, 1), (2, 8, 8, 2048, 512, 1, 1)]
    split = 0
    for sh in shapes:
        d = desc(*sh)
        sp = D.argus_conv_infer_splits(C.byref(d), BF16)
        mx = D.argus_conv_infer_max_splits(C.byref(d), BF16)
        assert sp >= 1 and mx == sh[5] * sh[5] * sh[3] // 64
        assert D.argus_conv_infer_splits(C.byref(d), F16) == sp
        assert D.argus_conv_infer_max_splits(C.byref(d), F16) == mx
        for s in (0, 1, 2, sp, mx):
            assert (D.argus_conv_infer_workspace_bytes(C.byref(d), F16, s)
                    == D.argus_conv_infer_workspace_bytes(C.byref(d), BF16, s))
        split += sp > 1
        assert D.argus_conv_infer_splits(C.byref(d), FP8) == 0
        assert D.argus_conv_infer_max_splits(C.byref(d), FP8) == 0
        assert D.argus_conv_infer_workspace_bytes(C.byref(d), FP8, 2) == 0
    assert split >= 2  # the comparison covered shapes that do split


def _placeholder(argtype, desc):
    from argus_amd import _lib

    if argtype is _lib._DESC:
        return C.byref(desc)
    if argtype is _lib._P:
        return None  # device pointers: NULL
    if argtype in (_lib._I, _lib._I64):
        return 64
    if argtype is _lib._SZ:
        return 0
    if argtype is _lib._F:
        return C.c_float(1e-5)
    return C.byref(argtype._type_())  # a pointer the host side may dereference: a real zeroed object


def test_every_unserved_entry_point_rejects_f16_before_it_launches():
    """Validation precedes the launch: that needs no device, and with one a missing check would run fp32 kernels
    over 2-byte buffers, so this never runs where a GPU is visible."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("placeholder pointers: never where a launch could reach a GPU")
    from argus_amd._lib import SIGNATURES, ConvDesc, lib

    D = lib().dll
    fns = _dtype_functions()
    assert SERVED <= set(fns) and set(QUERIES) <= set(fns) and len(fns) >= 40
    conv = ConvDesc(2, 8, 8, 64, 64, 3, 3, 1, 1, 8, 8, 0)
    stem = ConvDesc(2, 64, 64, 3, 64, 7, 7, 2, 3, 32, 32, 1)

    def check(name, args, want):
        D.argus_last_error()  # (the channel keeps the last message: each call below must set its own)
        rc = getattr(D, name)(*args)
        msg = D.argus_last_error()
        assert rc == want and b"dtype" in msg and b"F16" in msg, (name, rc, want, msg)

    swept = 0
    for name, at in sorted(fns.items()):
        if name in SERVED:
            continue
        res, argtypes = SIGNATURES[name]
        for d in (conv, stem):
            args = [_placeholder(t, d) for t in argtypes]
            args[at] = F16
            check(name, args, QUERIES.get(name, ERR_ARG))
        swept += 1
    assert swept == len(fns) - len(SERVED) >= 29
    # the two restricted ones outside their restriction; non-NULL placeholders, so the refusal is the dtype's
    p = C.c_void_p(16)
    check("argus_conv_fwd", [C.byref(conv), F16, p, p, p, None, None, None, None], ERR_ARG)
    check("argus_conv_weight_prep", [C.byref(conv), F16, p, None, p, p, None], ERR_ARG)
    check("argus_conv_fwd", [C.byref(stem), F16, p, p, p, None, None, p, None], ERR_ARG)  # stat_part set
    check("argus_conv_fwd", [C.byref(stem), F16, p, p, p, p, p, None, None], ERR_ARG)  # a BN+ReLU prologue
    # unknown values keep failing where they fail today
    rc = D.argus_conv_infer(C.byref(conv), 7, p, p, p, None, 1, p, 1, None, 0, None)
    assert rc != 0 and b"dtype" in D.argus_last_error()


def test_session_accepts_fp16_and_keeps_its_messages():
    from argus_amd.infer import SERVED as served, InferenceSession
    from argus_amd.models import NCameraCNN

    assert served == ("fp32", "bf16", "fp16")
    m = NCameraCNN()
    with pytest.raises(RuntimeError, match="HIP"):  # accepted as a dtype: the CPU model is what is refused
        InferenceSession(m, 1, (64, 64), compute_dtype="fp16")
    with pytest.raises(ValueError, match="'fp32' and 'bf16'.*fp16"):
        InferenceSession(m, 1, (64, 64), compute_dtype="fp8")
    assert hasattr(InferenceSession, "activation_peak")


def test_timing_cli_takes_fp16_only_with_frozen(monkeypatch, capsys):
    from argus_amd import timing

    seen = {}

    def fake(trials, batch, hw, dtype, train_mode, graph, frozen=False):
        seen.update(dtype=dtype, frozen=frozen)
        return {"mean_s": 0.0}

    monkeypatch.setattr(timing, "forward_latency", fake)
    timing.main(["--frozen", "--dtype", "fp16", "--trials", "1"])
    assert seen == {"dtype": "fp16", "frozen": True}
    with pytest.raises(SystemExit):
        timing.main(["--dtype", "fp16"])
    assert "--frozen" in capsys.readouterr().err
    monkeypatch.undo()
    with pytest.raises(ValueError, match="frozen"):  # decided before any device use
        timing.forward_latency(1, 1, (64, 64), "fp16", frozen=False, device="cpu")


def test_validate_has_the_session_dtype(tmp_path, dummy_data_path):
    import dataclasses
    import inspect

    from argus_amd import validate
    from argus_amd.data import CameraCubePoseDatasetConfig

    f = {x.name: x for x in dataclasses.fields(validate.ValConfig)}
    assert f["session_dtype"].default is None
    path = tmp_path / "m.pth"
    path.write_bytes(b"")
    cfg = validate.ValConfig(model_path=str(path), dataset_config=CameraCubePoseDatasetConfig(dummy_data_path),
                             session_dtype="fp16")
    assert cfg.session_dtype == "fp16"
    src = inspect.getsource(validate.main)
    assert '"--session-dtype"' in src and all(f'"{d}"' in src for d in ("fp32", "bf16", "fp16"))
