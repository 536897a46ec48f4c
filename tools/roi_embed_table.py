"""What conditioning the head on the region of interest costs (profiles/roi_embed.txt), on one MI355X:

    python tools/roi_embed_table.py [--out profiles/roi_embed.txt] [--trials 200] [--steps 30] [--rounds 3]
                                    [--parent PATH]

The method of tools/pose_track_table.py: one process per cell (this script re-run with --cell), the arms
interleaved within every round, medians of event-timed calls (argus_amd.utils.time_torch_fn), compared pair by pair.

(a) pose():  PoseSession(track=...) at 256x256, B=1, bf16, 672x376 planar uint8 frames, two cameras 0.2 from the
             first predicted cube; "plain" is NCameraCNNConfig(), "cond" NCameraCNNConfig(roi_frame_hw=(376, 672))
             with a random roi_embed.weight: argus_pose_tail_roi in place of argus_pose_tail, 56 launches in both.
(b) step():  FusedTrainer.step at B=64, 256x256, bf16 on device-resident uint8 batches; "cond" (step_roi) adds argus_roi_embed
             and the 128 x 8 x 64 weight-gradient GEMM.
--parent PATH: a built checkout of the parent commit; its unconditioned model is measured as a third arm ("parent")
in the same rounds, which separates what the feature costs a plain model (nothing is meant to change) from the
run-to-run spread."""
from __future__ import annotations

import argparse
import json
import math
import statistics
import subprocess
import sys
from pathlib import Path

HW, FHW = (256, 256), (376, 672)
HALF, MARGIN, Z_NEAR = 0.035, 1.5, 0.02


def _look_at(eye, target):
    import numpy as np

    from argus_amd.track import Camera

    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    f = (FHW[0] / 2) / math.tan(math.radians(70.0) / 2)
    return Camera(R.reshape(9), -R @ eye, f, f, FHW[1] / 2, FHW[0] / 2)


def _model(cond: bool, dev):
    import torch

    from argus_amd.models import NCameraCNN, NCameraCNNConfig

    torch.manual_seed(0)
    cfg = NCameraCNNConfig(n_cams=2, roi_frame_hw=FHW) if cond else NCameraCNNConfig(n_cams=2)
    model = NCameraCNN(cfg, compute_dtype="bf16").to(dev)
    if cond:
        with torch.no_grad():
            model.roi_embed.weight.uniform_(-0.5, 0.5)
    return model


def cell_pose(cond: bool, trials: int) -> dict:
    import numpy as np
    import torch

    from argus_amd.pose_session import PoseSession
    from argus_amd.track import TrackConfig
    from argus_amd.utils import time_torch_fn

    dev = "cuda"
    model = _model(cond, dev).eval()
    frames = [torch.randint(0, 256, (1, 6, *FHW), dtype=torch.uint8, device=dev) for _ in range(4)]
    kw = dict(compute_dtype="bf16", frame_hw=FHW)
    center = PoseSession(model, 1, HW, roi=True, **kw).pose(frames[0])[0, :3].double().cpu().numpy()
    off = 0.2 * np.array([0.0, 0.15, 0.13]) / math.hypot(0.15, 0.13)
    cams = [_look_at(center + off * [1, s, 1], center) for s in (1.0, -1.0)]
    s = PoseSession(model, 1, HW, track=TrackConfig(cams, HALF, margin=MARGIN, z_near=Z_NEAR), **kw)
    times = []
    for i in range(trials + 5):
        out, t = time_torch_fn(lambda: s.pose(frames[i % 4]))
        if i >= 5:
            times.append(t * 1e3)
    assert bool(torch.isfinite(out).all()) and tuple(out.shape) == (1, 7)
    return {"median": statistics.median(times), "min": min(times), "mean": statistics.fmean(times),
            "launches": s.launches_per_forward}


def cell_step(cond: bool, steps: int) -> dict:
    import torch

    from argus_amd.step import FusedTrainer
    from argus_amd.utils import time_torch_fn

    dev, B = "cuda", 64
    model = _model(cond, dev).train()
    tr = FusedTrainer(model, lr=1e-4, max_grad_norm=1.0)
    g = torch.Generator().manual_seed(1)
    xs = [torch.randint(0, 256, (B, 6, *HW), generator=g, dtype=torch.uint8).to(dev) for _ in range(2)]
    q = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=-1)
    T = torch.cat([0.1 * torch.randn(B, 3, generator=g), q], -1).to(dev)
    roi = None
    if cond:  # regions of half to full scale somewhere in the frame
        e = torch.empty(B, 2, 1).uniform_(0.5, 1.0, generator=g) * torch.tensor([float(HW[0]), float(HW[1])])
        o = torch.rand(B, 2, 2, generator=g) * (torch.tensor([float(FHW[0]), float(FHW[1])]) - e)
        roi = torch.cat([o, e], -1).to(dev)
    times = []
    for i in range(steps + 5):
        out, t = time_torch_fn(lambda: tr.step_roi(xs[i % 2], T, roi) if cond else tr.step(xs[i % 2], T))
        if i >= 5:
            times.append(t * 1e3)
    assert bool(torch.isfinite(out).all())
    return {"median": statistics.median(times), "min": min(times), "mean": statistics.fmean(times), "launches": 0}


def _spawn(root: Path, *args) -> str:
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--root", str(root), *args],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"cell {args} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout.strip().splitlines()[-1]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="profiles/roi_embed.txt")
    ap.add_argument("--trials", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (third arm)")
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]), help=argparse.SUPPRESS)
    ap.add_argument("--cell", nargs=2, metavar=("WHAT", "ARM"), default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.root)  # the checkout whose argus_amd a cell measures
    if a.cell:
        what, arm = a.cell
        fn, n = (cell_pose, a.trials) if what == "pose" else (cell_step, a.steps)
        print(json.dumps(fn(arm == "cond", n)))
        return
    arms = [("plain", a.root), ("cond", a.root)] + ([("parent", a.parent)] if a.parent else [])
    lines = ["# Conditioning the head on the region of interest, one MI355X, bf16: python tools/roi_embed_table.py",
             f"# one process per cell, arms interleaved within a round; pose: {a.trials} event-timed calls of a tracked "
             f"PoseSession, 256x256, B=1, 672x376 uint8 frames; step: {a.steps} event-timed FusedTrainer.step, B=64, "
             "256x256; ms per call",
             "# what arm    launches round  median    min       mean"]
    summary = []
    for what in ("pose", "step"):
        med = {arm: [] for arm, _ in arms}
        for rnd in range(1, a.rounds + 1):
            for arm, root in arms:
                r = json.loads(_spawn(Path(root), "--cell", what, arm, "--trials", str(a.trials), "--steps",
                                      str(a.steps)))
                med[arm].append(r["median"])
                lines.append(f"{what:4s} {arm:6s} {r['launches']:8d} {rnd:5d} {r['median']:9.4f} {r['min']:9.4f} "
                             f"{r['mean']:9.4f}")
                print(lines[-1], flush=True)
        ratio = [c / p for c, p in zip(med["cond"], med["plain"])]
        spread = max(med["plain"]) / min(med["plain"])
        summary.append(f"{what} cond / plain per pair: " + " ".join(f"{r:.4f}" for r in ratio)
                       + f"; plain's own round-to-round spread {spread:.4f}: the conditioning is "
                       + ("ABOVE" if min(ratio) > spread else "within") + " that spread"
                       + f" (medians {statistics.median(med['plain']):.4f} -> {statistics.median(med['cond']):.4f} ms)")
        if a.parent:
            pr = [p / q for p, q in zip(med["plain"], med["parent"])]
            summary.append(f"{what} plain / parent per pair: " + " ".join(f"{r:.4f}" for r in pr)
                           + f" (parent median {statistics.median(med['parent']):.4f} ms)")
    lines += ["", "# summary"] + summary
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines[-(len(summary) + 2):]))


if __name__ == "__main__":
    main()
