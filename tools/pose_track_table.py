"""The closed-loop tracking measurements of profiles/pose_track.txt, on one MI355X:

    python tools/pose_track_table.py [--out profiles/pose_track.txt] [--trials 200] [--rounds 2]

One process per cell (this script re-run with --cell), the three arms interleaved within every round, medians of
``trials`` event-timed calls (argus_amd.utils.time_torch_fn) from frames on the device to the pose tensor. 256x256,
B=1, bf16 and fp16, 672x376 planar uint8 frames, two cameras placed 0.2 from the first predicted cube.

(a) "roi":   PoseSession(roi=True), the region left where it is: the graph without the new launch (55 launches);
(b) "track": PoseSession(track=...): the graph ends with argus_roi_from_pose (56 launches), nothing else per call;
(c) "host":  the loop written around (a) without the feature: pose(), .cpu(), the region in numpy (the formula of
             argus_roi_from_pose), set_roi (check_roi + H2D copy), and only then the next pose().
(b) / (a) is what the added launch costs; (b) / (c) is what closing the loop on the device saves."""
from __future__ import annotations

import argparse
import json
import math
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
HW, FHW = (256, 256), (376, 672)
HALF, MARGIN, Z_NEAR = 0.035, 1.5, 0.02
ARMS = ("roi", "track", "host")


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


def _host_region(pose, cams):
    """The region of every camera image from a (7,) pose, in numpy: what a caller computes between two replays."""
    import numpy as np

    t, (x, y, z, w) = pose[:3], pose[3:] / np.linalg.norm(pose[3:])
    Rq = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    corners = t + (np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)]) * HALF) @ Rq.T
    out = []
    for c in cams:
        Y = corners @ np.array(c.R).reshape(3, 3).T + np.array(c.t)
        if not np.isfinite(Y).all() or (Y[:, 2] < Z_NEAR).any():
            out.append(((FHW[0] - HW[0]) // 2, (FHW[1] - HW[1]) // 2, *HW))
            continue
        u, v = c.fx * Y[:, 0] / Y[:, 2] + c.cx, c.fy * Y[:, 1] / Y[:, 2] + c.cy
        s = MARGIN * max((v.max() - v.min()) / HW[0], (u.max() - u.min()) / HW[1])
        s = min(max(s, 0.25), 4.0, FHW[0] / HW[0], FHW[1] / HW[1])
        eh, ew = np.float32(s * HW[0]), np.float32(s * HW[1])
        y0 = min(max((v.max() + v.min()) / 2 - eh / 2, 0.0), FHW[0] - eh)
        x0 = min(max((u.max() + u.min()) / 2 - ew / 2, 0.0), FHW[1] - ew)
        out.append((math.floor(y0 * 1024) / 1024, math.floor(x0 * 1024) / 1024, eh, ew))  # o + e <= S after rounding
    return np.array([out], dtype=np.float64)


def cell(arm: str, dtype: str, trials: int) -> dict:
    import numpy as np
    import torch

    from argus_amd.models import NCameraCNN, NCameraCNNConfig
    from argus_amd.pose_session import PoseSession
    from argus_amd.track import TrackConfig
    from argus_amd.utils import time_torch_fn

    torch.manual_seed(0)
    dev = "cuda"
    model = NCameraCNN(NCameraCNNConfig(n_cams=2), compute_dtype="fp32" if dtype == "fp16" else dtype).to(dev).eval()
    frames = [torch.randint(0, 256, (1, 6, *FHW), dtype=torch.uint8, device=dev) for _ in range(4)]
    kw = dict(compute_dtype=dtype, frame_hw=FHW)
    center = PoseSession(model, 1, HW, **kw).pose(frames[0])[0, :3].double().cpu().numpy()
    off = 0.2 * np.array([0.0, 0.15, 0.13]) / math.hypot(0.15, 0.13)
    cams = [_look_at(center + off * [1, s, 1], center) for s in (1.0, -1.0)]
    if arm == "track":
        s = PoseSession(model, 1, HW, track=TrackConfig(cams, HALF, margin=MARGIN, z_near=Z_NEAR), **kw)
        run = s.pose
    else:
        s = PoseSession(model, 1, HW, roi=True, **kw)
        run = s.pose
        if arm == "host":
            def run(x):
                pose = s.pose(x)
                s.set_roi(_host_region(pose[0].cpu().numpy().astype("float64"), cams))  # sync, D2H, numpy, H2D
                return pose
    times = []
    for i in range(trials + 5):
        out, t = time_torch_fn(lambda: run(frames[i % 4]))
        if i >= 5:
            times.append(t * 1e3)
    assert bool(torch.isfinite(out).all()) and tuple(out.shape) == (1, 7)
    moved = bool((s.roi != torch.tensor([60.0, 208.0, 256.0, 256.0])).any())
    return {"median": statistics.median(times), "min": min(times), "mean": statistics.fmean(times),
            "launches": s.launches_per_forward, "moved": moved}


def _spawn(*args) -> str:
    r = subprocess.run([sys.executable, __file__, *args], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"cell {args} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout.strip().splitlines()[-1]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="profiles/pose_track.txt")
    ap.add_argument("--trials", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--cell", nargs=2, metavar=("ARM", "DTYPE"), default=None)
    a = ap.parse_args()
    if a.cell:
        print(json.dumps(cell(*a.cell, a.trials)))
        return
    lines = ["# Closed-loop tracking in the pose session, one MI355X, 256x256, B=1, 672x376 uint8 frames, hipGraph "
             "replay: python tools/pose_track_table.py",
             f"# one process per cell, arms interleaved within a round, {a.trials} event-timed calls; ms per call, "
             "frames on the device -> pose (host: and the next region set)",
             "# dtype arm    launches moved round  median   min      mean"]
    summary = []
    for dtype in ("bf16", "fp16"):
        med = {arm: [] for arm in ARMS}
        for rnd in range(1, a.rounds + 1):
            for arm in ARMS:
                r = json.loads(_spawn("--cell", arm, dtype, "--trials", str(a.trials)))
                med[arm].append(r["median"])
                lines.append(f"{dtype}    {arm:6s} {r['launches']:8d} {str(r['moved']):5s} {rnd:5d} {r['median']:8.4f} "
                             f"{r['min']:8.4f} {r['mean']:8.4f}")
                print(lines[-1], flush=True)
        ba = [b / x for b, x in zip(med["track"], med["roi"])]
        bc = [b / x for b, x in zip(med["track"], med["host"])]
        aa = max(med["roi"]) / min(med["roi"])
        summary.append(f"{dtype} (b)/(a) track / roi per pair: " + " ".join(f"{r:.3f}" for r in ba)
                       + f"; (a)'s own pair-to-pair spread {aa:.3f}: the added launch is "
                       + ("ABOVE" if min(ba) > aa else "within") + " that spread")
        summary.append(f"{dtype} (b)/(c) track / host per pair: " + " ".join(f"{r:.3f}" for r in bc)
                       + f"; {statistics.median(med['host']) / statistics.median(med['track']):.2f}x: "
                       + ("faster in every pair" if max(bc) < 1 else "NOT faster in every pair"))
    lines += ["", "# summary"] + summary
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines[-(len(summary) + 2):]))


if __name__ == "__main__":
    main()
