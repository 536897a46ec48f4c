"""Latency of one frozen-BatchNorm fine-tuning step (argus_amd.finetune.FineTuneSession) on one MI355X, device events.

    python tools/finetune_latency.py --dtype bf16 --batch 2 --trainable all [--hw 256 256] [--rounds 3] [--trials 50]
    python tools/finetune_latency.py --dtype bf16 --batch 2 --kernels      # per-kernel times of one eager step

One process per (dtype, batch, trainable) cell. Three arms, interleaved within each round (a, b, c, a, b, ...), median /
min / mean per arm and round:

  a step     FineTuneSession.step(images, target): the replayed graph (re-fold, forward, loss, backward, parameter
             gradients, norm), argus_adam_step, the re-fold graph
  b eager    the same launches issued eagerly (graph=False)
  c stock    what the reference does for such a step: the oracle's torch.nn model on the device in eval(), stock
             autograd (fp32; bf16 = torch.autocast(bfloat16)), clip_grad_norm_ and torch.optim.Adam over the trained
             parameters (trainable "head" / "layerK": requires_grad is off on the frozen prefix, so autograd stops
             at the head / at the stage boundary)

Every arm trains its own copy of the weights; the step does not depend on their values. There is no pass/fail on
time. The launches per step() are the session's own count of the entry points it issues (a split weight gradient or
head GEMM is two kernels). --kernels prints the library's per-kernel timer (argus_ktimer) over one eager step.
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def _time(fn, trials: int) -> list:
    """Per-call device time of ``fn`` in ms: one event pair per call, read after the last one."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(trials)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="bf16")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--trainable", choices=["all", "head", "layer1", "layer2", "layer3", "layer4"], default="all")
    ap.add_argument("--hw", type=int, nargs=2, default=[256, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trials", type=int, default=50)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args(argv)

    from argus_amd.finetune import FineTuneSession
    from argus_amd.losses import geometric_loss_fn
    from argus_amd.models import NCameraCNN
    from argus_amd.utils import se3_exp
    from oracle.ncamera import build_reference_model

    dev = torch.device("cuda", 0)
    hw, B = tuple(a.hw), a.batch
    ref = build_reference_model(42)
    g = torch.Generator().manual_seed(7)
    for m in ref.modules():  # non-trivial running statistics
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.data = 0.1 * torch.randn(m.num_features, generator=g)
            m.running_var.data = 0.5 + torch.rand(m.num_features, generator=g)

    def product():
        model = NCameraCNN(compute_dtype=a.dtype)
        model.load_state_dict(ref.state_dict())
        return model.to(dev).eval()

    x = torch.rand(B, 6, *hw, generator=g).to(dev)
    target = se3_exp(0.3 * torch.randn(B, 6, generator=g).to(dev))
    tag = f"{a.dtype} B={B} {a.trainable} {hw[0]}x{hw[1]}"

    if a.kernels:
        from argus_amd.profiling import KernelTimer

        s = FineTuneSession(product(), B, hw, trainable=a.trainable, graph=False)
        s.step(x, target)
        torch.cuda.synchronize()
        with KernelTimer() as t:
            s.step(x, target)
            torch.cuda.synchronize()
        rows = sorted(t.summary().items(), key=lambda kv: -kv[1]["total_ms"])
        total = sum(r["total_ms"] for _, r in rows)
        print(f"# argus_ktimer over one eager step, {tag}: timed kernels {1e3 * total:.1f} us in "
              f"{sum(r['launches'] for _, r in rows)} launches (conv, bias-sum and fold kernels; pools, head and "
              f"optimizer are not timed launches)")
        print("# launches  total_us  avg_us  kernel")
        for name, r in rows:
            print(f"{r['launches']:9d} {1e3 * r['total_ms']:9.1f} {r['avg_us']:7.2f}  {name}")
        return

    sg = FineTuneSession(product(), B, hw, trainable=a.trainable, graph=True)
    se = FineTuneSession(product(), B, hw, trainable=a.trainable, graph=False)
    stock_model = ref.to(dev).eval()
    if a.trainable != "all":  # the head, or resnet.layerK and everything behind it in model order
        names = [n for n, _ in stock_model.named_parameters()]
        first = "resnet.fc.weight" if a.trainable == "head" else f"resnet.{a.trainable}.0.conv1.weight"
        for i, p in enumerate(stock_model.parameters()):
            p.requires_grad_(i >= names.index(first))
    params = [p for p in stock_model.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-4)

    def stock():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=a.dtype == "bf16"):
            pred = stock_model(x)
        losses = geometric_loss_fn(pred.float(), target)
        losses.mean().backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        return losses

    arms = [("step", lambda: sg.step(x, target)), ("eager", lambda: se.step(x, target)), ("stock", stock)]
    print(f"# {tag}, {a.trials} trials per arm and round, ms; launches per step() {sg.launches_per_step} "
          f"(of them re-fold {sg.launches_per_refold}) + re-fold after Adam {sg.launches_per_refold}")
    print("# dtype batch trainable arm    round  median   min      mean")
    med = {n: [] for n, _ in arms}
    for r in range(1, a.rounds + 1):
        for name, fn in arms:
            t = _time(fn, a.trials)
            med[name].append(statistics.median(t))
            print(f"{a.dtype}  {B:5d} {a.trainable:9s} {name:6s} {r:5d} {statistics.median(t):8.4f} {min(t):8.4f} "
                  f"{statistics.fmean(t):8.4f}", flush=True)
    st, eg, sk = (statistics.median(med[n]) for n in ("step", "eager", "stock"))
    print(f"# {tag}: step {st:.4f} | eager {eg:.4f} | stock {sk:.4f} ({sk / st:.2f}x step)")


if __name__ == "__main__":
    main()
