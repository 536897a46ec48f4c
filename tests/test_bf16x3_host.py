"""CPU: the host surface of the bf16x3 split-precision mode (policy key 53, ABI 21, the CLI field) and the
properties of the split the tests' CPU emulation (tests/x3_reference.py) shares with the kernels."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

from x3_reference import ConvX3, split, use_x3_convs  # noqa: E402


def test_policy_key_and_abi():
    from argus_amd._lib import ABI_VERSION, lib

    L = lib()
    assert L.dll.argus_conv_policy_default(53) == 0  # default off: no existing caller changes
    assert L.dll.argus_conv_policy_default(52) == -1  # 52 stays unknown
    assert L.dll.argus_conv_policy_default(54) == -1
    assert L.dll.argus_abi_version() == ABI_VERSION == 21


def test_cli_float32_matmul_precision(dummy_data_path, tmp_path):
    from argus_amd.train import TrainConfig, parse_args

    base = ["--dataset-config.dataset-path", dummy_data_path, "--save-dir", str(tmp_path)]
    assert parse_args(base).float32_matmul_precision == "highest"
    assert parse_args(base + ["--float32-matmul-precision", "high"]).float32_matmul_precision == "high"
    assert parse_args(base + ["--float32-matmul-precision", "highest"]).float32_matmul_precision == "highest"
    with pytest.raises(SystemExit):
        parse_args(base + ["--float32-matmul-precision", "medium"])
    cfg = parse_args(base)
    with pytest.raises(ValueError):
        TrainConfig(dataset_config=cfg.dataset_config, save_dir=str(tmp_path), float32_matmul_precision="medium")


def test_engine_rejects_unknown_dtype_and_names_bf16x3():
    from argus_amd.engine import ResNetEngine

    with pytest.raises(ValueError, match="bf16x3"):
        ResNetEngine(2, 1024, "tf32", torch.device("cpu"))


def test_split_properties():
    g = torch.Generator().manual_seed(0)
    # magnitudes across the fp32 range the bf16 parts can hold as normal numbers, zeros and exact bf16 values
    x = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-60, 60, (1 << 16,), generator=g).float())
    x[::97] = 0.0
    x[1::97] = -0.0
    x[2::97] = x[2::97].to(torch.bfloat16).float()
    hi, lo = split(x)
    assert hi.dtype == lo.dtype == torch.float32
    # both parts are bf16 values
    assert torch.equal(hi, hi.to(torch.bfloat16).float()) and torch.equal(lo, lo.to(torch.bfloat16).float())
    # x - hi is exactly representable: recomputed in fp64 it is the same number
    assert torch.equal((x.double() - hi.double()).float().double(), x.double() - hi.double())
    assert torch.equal((x - hi).double(), x.double() - hi.double())
    # hi + lo reproduces x to 2^-16 |x| (8 significant bits each; fp64 sum: no further rounding)
    err = (hi.double() + lo.double() - x.double()).abs()
    assert (err <= 2.0 ** -16 * x.double().abs()).all(), (err / x.double().abs().clamp_min(1e-300)).max().item()
    # zeros stay zero in both parts; exact bf16 inputs have no lo part
    z = x == 0
    assert (hi[z] == 0).all() and (lo[z] == 0).all()
    assert (lo[2::97] == 0).all()
    # NaN stays NaN (round to nearest, not the integer trick)
    h, l_ = split(torch.tensor([float("nan"), float("inf"), 3.4e38]))
    assert torch.isnan(h[0]) and torch.isnan(l_[0])
    # documented: an infinite input, or a finite one above the bf16 maximum, gives a NaN product sum
    assert torch.isinf(h[1]) and torch.isnan(l_[1])
    assert torch.isinf(h[2]) and torch.isinf(l_[2]) and torch.isnan(h[2] * 1.0 + l_[2] * 1.0)


def test_conv_x3_autograd_meets_the_error_model():
    """The emulation's three passes meet the kernels' bar, 4 * 2^-16 * (|a| conv |b|) against fp64 (3 for
    the dropped terms, the rest for the fp32 accumulation), and are not the exact fp32 result."""
    torch.manual_seed(1)
    x = torch.randn(2, 64, 9, 9, requires_grad=True)
    w = (torch.randn(64, 64, 3, 3) * 0.05).requires_grad_()
    y = ConvX3.apply(x, w, (2, 2), (1, 1))
    gy = torch.randn_like(y)
    gx, gw = torch.autograd.grad(y, (x, w), gy)
    xd, wd, gyd = x.detach().double(), w.detach().double(), gy.double()
    F = torch.nn.functional
    refs = (F.conv2d(xd, wd, stride=2, padding=1),
            torch.nn.grad.conv2d_input(xd.shape, wd, gyd, stride=2, padding=1),
            torch.nn.grad.conv2d_weight(xd, wd.shape, gyd, stride=2, padding=1))
    mags = (F.conv2d(xd.abs(), wd.abs(), stride=2, padding=1),
            torch.nn.grad.conv2d_input(xd.shape, wd.abs(), gyd.abs(), stride=2, padding=1),
            torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, gyd.abs(), stride=2, padding=1))
    for got, ref, mag in zip((y.detach(), gx, gw), refs, mags):
        assert ((got.double() - ref).abs() <= 4 * 2.0 ** -16 * mag + 1e-30).all()
    assert not torch.equal(y.detach(), F.conv2d(x.detach(), w.detach(), stride=2, padding=1))


def test_use_x3_convs_swaps_every_conv():
    from oracle.ncamera import build_reference_model

    m = use_x3_convs(build_reference_model(42)).train()
    n = sum(isinstance(c, torch.nn.Conv2d) for c in m.modules())
    assert n == 53
    assert all("forward" in c.__dict__ for c in m.modules() if isinstance(c, torch.nn.Conv2d))
