"""bench.py's result head and --dump-outputs (CPU tests of the host-side pieces; the step itself needs a GPU)."""
import argparse
import types

import numpy as np
import torch

import bench


def _fake_trainer(total: int, seed: int = 0):
    g = torch.Generator().manual_seed(seed)
    flat = types.SimpleNamespace(total=total, param=torch.randn(total, generator=g),
                                 grad=torch.randn(total, generator=g, dtype=torch.float64).float())
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 1), torch.nn.BatchNorm2d(4))
    return types.SimpleNamespace(flat=flat, model=model, grad_norm=lambda: torch.tensor([2.5]))


def test_headline_reports_the_timed_steps():
    args = argparse.Namespace(steps=8, warmup=2, dtype="bf16")
    h = bench.headline(args, 1, 64, 256, 256, 0.1)
    assert h["steps"] == 8 and h["warmup"] == 2 and h["dtype"] == "bf16"
    assert h["ms_per_step"] == 12.5  # 100 ms over 8 steps
    assert h["value"] == 10240.0 and h["unit"] == "images/s" and h["higher_is_better"] is True
    assert h["samples_per_s"] == 5120.0
    assert h["metric"] == "train images/sec + val SE(3) geodesic err, 2x256x256 RGB"
    assert bench.headline(args, 2, 64, 256, 256, 0.1)["value"] == 20480.0


def test_step_outputs_small_buffers_are_kept_whole():
    tr = _fake_trainer(1000)
    losses = torch.arange(4.0)
    out = bench.step_outputs(tr, losses)
    assert set(out) == {"losses", "grad_norm", "grad_sample", "param_sample", "running_stats"}
    assert torch.equal(out["losses"], losses) and out["losses"] is not losses
    assert torch.equal(out["grad_sample"], tr.flat.grad) and torch.equal(out["param_sample"], tr.flat.param)
    assert out["running_stats"].tolist() == [0.0] * 4 + [1.0] * 4  # running_mean, running_var; no integer buffer
    assert all(v.dtype == torch.float32 and v.device.type == "cpu" for v in out.values())


def test_step_outputs_sample_is_fixed_and_bounded():
    total = bench.DUMP_SAMPLE + 12345
    tr = _fake_trainer(total)
    a = bench.step_outputs(tr, torch.zeros(2))
    b = bench.step_outputs(tr, torch.zeros(2))
    assert a["grad_sample"].numel() == a["param_sample"].numel() == bench.DUMP_SAMPLE
    assert torch.equal(a["grad_sample"], b["grad_sample"]) and torch.equal(a["param_sample"], b["param_sample"])
    # the same positions of both buffers
    tr.flat.grad = tr.flat.param.clone()
    c = bench.step_outputs(tr, torch.zeros(2))
    assert torch.equal(c["grad_sample"], c["param_sample"])
    assert sum(v.numel() * 4 for v in a.values()) <= 64 * 2**20


def test_dump_outputs_writes_float32_npy(tmp_path):
    out = {"losses": torch.tensor([0.5, 1.5]), "grad_norm": torch.tensor([3.0])}
    d = tmp_path / "nested" / "dump"
    bench.dump_outputs(str(d), out)
    assert sorted(p.name for p in d.iterdir()) == ["grad_norm.npy", "losses.npy"]
    x = np.load(d / "losses.npy")
    assert x.dtype == np.float32 and x.tolist() == [0.5, 1.5]
