"""Latency of the frozen gradient (argus_amd.infer_grad.GradientSession) on one MI355X, device events.

    python tools/frozen_grad_latency.py --dtype bf16 --batch 1 [--hw 256 256] [--rounds 3] [--trials 100]
    python tools/frozen_grad_latency.py --dtype bf16 --batch 1 --kernels     # per-kernel times of one eager call

One process per (dtype, batch) cell. Four arms, interleaved within each round (a, b, c, d, a, b, ...), median / min /
mean per arm and round:

  a forward    InferenceSession(images), replayed: the frozen forward alone
  b gradient   GradientSession.image_gradient(images, target), replayed: forward + SE(3) loss + backward, one graph
  c eager      the same launches issued eagerly (graph=False)
  d autograd   what a user does today for an eval-mode gradient: the oracle's torch.nn model on the device in
               eval(), stock autograd with images.requires_grad_() (fp32; bf16 = torch.autocast(bfloat16))

There is no pass/fail on time. --kernels prints the library's own per-kernel timer (argus_ktimer) over one eager
image_gradient: where the time of the chain goes.
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
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--hw", type=int, nargs=2, default=[256, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trials", type=int, default=100)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args(argv)

    from argus_amd.infer import InferenceSession
    from argus_amd.infer_grad import GradientSession
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
    model = NCameraCNN(compute_dtype=a.dtype)
    model.load_state_dict(ref.state_dict())
    model = model.to(dev).eval()
    ref = ref.to(dev).eval()
    x = torch.rand(B, 6, *hw, generator=g).to(dev)
    target = se3_exp(0.3 * torch.randn(B, 6, generator=g).to(dev))

    if a.kernels:
        from argus_amd.profiling import KernelTimer

        s = GradientSession(model, B, hw, graph=False)
        s.image_gradient(x, target)
        torch.cuda.synchronize()
        with KernelTimer() as t:
            s.image_gradient(x, target)
            torch.cuda.synchronize()
        rows = sorted(t.summary().items(), key=lambda kv: -kv[1]["total_ms"])
        total = sum(r["total_ms"] for _, r in rows)
        print(f"# argus_ktimer over one eager image_gradient, {a.dtype} B={B} {hw[0]}x{hw[1]}: timed kernels "
              f"{1e3 * total:.1f} us in {sum(r['launches'] for _, r in rows)} launches (the conv kernels; pools, head "
              f"and stem tail are not timed launches)")
        print("# launches  total_us  avg_us  kernel")
        for name, r in rows:
            print(f"{r['launches']:9d} {1e3 * r['total_ms']:9.1f} {r['avg_us']:7.2f}  {name}")
        return

    fwd = InferenceSession(model, B, hw)
    sg, se = GradientSession(model, B, hw, graph=True), GradientSession(model, B, hw, graph=False)

    def autograd():
        xi = x.detach().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=a.dtype == "bf16"):
            pred = ref(xi)
        loss = geometric_loss_fn(pred.float(), target).mean()
        return torch.autograd.grad(loss, xi)[0]

    arms = [("forward", lambda: fwd(x)), ("gradient", lambda: sg.image_gradient(x, target)),
            ("eager", lambda: se.image_gradient(x, target)), ("autograd", autograd)]
    print(f"# {a.dtype} B={B} {hw[0]}x{hw[1]}, {a.trials} trials per arm and round, ms")
    print("# dtype batch arm       round  median   min      mean")
    med = {n: [] for n, _ in arms}
    for r in range(1, a.rounds + 1):
        for name, fn in arms:
            t = _time(fn, a.trials)
            med[name].append(statistics.median(t))
            print(f"{a.dtype}  {B:5d} {name:9s} {r:5d} {statistics.median(t):8.4f} {min(t):8.4f} {statistics.fmean(t):8.4f}",
                  flush=True)
    f, gr = statistics.median(med["forward"]), statistics.median(med["gradient"])
    print(f"# {a.dtype} B={B}: forward {f:.4f} | gradient {gr:.4f} ({gr / f:.2f}x forward) | eager "
          f"{statistics.median(med['eager']):.4f} | autograd {statistics.median(med['autograd']):.4f} "
          f"({statistics.median(med['autograd']) / gr:.2f}x gradient)")


if __name__ == "__main__":
    main()
