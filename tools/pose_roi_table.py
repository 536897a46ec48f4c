"""The region-of-interest measurements of profiles/pose_roi.txt, on one MI355X:

    python tools/pose_roi_table.py [--out profiles/pose_roi.txt] [--trials 200] [--rounds 2]

One process per cell (this script re-run with --cell), the arms of a comparison interleaved within every round,
medians of ``trials`` event-timed pose() calls (argus_amd.utils.time_torch_fn) from frames on the device to the
pose tensor. 256x256, B=1, bf16 and fp16.

(a) PoseSession(roi=True) left at its unit-scale center crop against PoseSession(roi=False), 672x376 planar uint8.
(b) PoseSession(roi=True) on (B, n_cams, Hs, Ws, 3) uint8 camera frames of 1280x720 and 1920x1080, the region the
    centered 256 * Hs / 376 square (what the 672x376 pipeline's center crop sees of a camera Hs / 376 times as
    fine), against what there was before: torch on the device, then PoseSession.pose on fp32 planar 256x256 frames:
    "resize+crop": /255, F.interpolate(antialias=True) of the whole frame to 376 rows, center crop (the order of
                   argus/validate_real.py with a resize in front);
    "crop+resize": the cheapest torch form: slice the (integer) region first, /255, F.interpolate to 256x256.
(c) the stem launches alone: device events around 200 back-to-back calls."""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
HW = (256, 256)
CAMERAS = {"720p": (720, 1280), "1080p": (1080, 1920)}


def _region(fhw):
    e = HW[0] * fhw[0] / 376.0
    return ((fhw[0] - e) / 2, (fhw[1] - e) / 2, e, e)


def cell(arm: str, dtype: str, camera: str, trials: int) -> dict:
    import torch
    import torch.nn.functional as F

    from argus_amd.data import center_crop_slices
    from argus_amd.models import NCameraCNN, NCameraCNNConfig
    from argus_amd.pose_session import PoseSession
    from argus_amd.utils import time_torch_fn

    torch.manual_seed(0)
    dev = "cuda"
    model = NCameraCNN(NCameraCNNConfig(n_cams=2), compute_dtype="fp32" if dtype == "fp16" else dtype).to(dev).eval()
    if camera == "sim":  # (a)
        fhw = (376, 672)
        shape = (1, 6, *fhw)
        s = PoseSession(model, 1, HW, compute_dtype=dtype, frame_hw=fhw, roi=arm == "roi")
        run = s.pose
    else:  # (b)
        fhw = CAMERAS[camera]
        shape = (1, 2, *fhw, 3)
        y0, x0, e, _ = _region(fhw)
        if arm == "roi":
            s = PoseSession(model, 1, HW, compute_dtype=dtype, frame_hw=fhw, layout="hwc", roi=True)
            s.set_roi((y0, x0, e, e))
            run = s.pose
        else:
            s = PoseSession(model, 1, HW, compute_dtype=dtype)
            if arm == "resize+crop":
                size = (376, round(fhw[1] * 376 / fhw[0]))
                ys, xs = center_crop_slices(size, HW)

                def run(x):
                    x = x.permute(0, 1, 4, 2, 3).reshape(1, 6, *fhw).float().div_(255.0)
                    x = F.interpolate(x, size=size, mode="bilinear", antialias=True, align_corners=False)
                    return s.pose(x[..., ys, xs])
            else:
                iy, ix, ie = round(y0), round(x0), round(e)

                def run(x):
                    x = x[:, :, iy:iy + ie, ix:ix + ie, :].permute(0, 1, 4, 2, 3).reshape(1, 6, ie, ie).float().div_(255.0)
                    return s.pose(F.interpolate(x, size=HW, mode="bilinear", antialias=True, align_corners=False))
    frames = [torch.randint(0, 256, shape, dtype=torch.uint8, device=dev) for _ in range(4)]
    times = []
    for i in range(trials + 5):
        out, t = time_torch_fn(lambda: run(frames[i % 4]))
        if i >= 5:
            times.append(t * 1e3)
    assert bool(torch.isfinite(out).all()) and tuple(out.shape) == (1, 7)
    return {"median": statistics.median(times), "min": min(times), "mean": statistics.fmean(times)}


def stem_cell(dtype: str) -> list:
    """(c): microseconds per call of the stem launches alone, n_img = 2, 256x256."""
    import ctypes as C

    import torch

    from argus_amd._lib import BF16, F16, FrameSrc, lib, ptr, stream
    from argus_amd.timing import _event_ms

    L, dt, tdt = lib(), {"bf16": BF16, "fp16": F16}[dtype], {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    dev = "cuda"
    wf = (torch.randn(64, 8, 8, 4, device=dev) / 12).to(tdt)
    scale, shift = torch.rand(64, device=dev) + 0.5, torch.randn(64, device=dev) * 0.1
    out = torch.empty(2, 64, 64, 64, dtype=tdt, device=dev)
    x0 = torch.empty(2, 256, 256, 4, dtype=tdt, device=dev)
    rows = []
    for name, fhw in (("sim", (376, 672)), *CAMERAS.items()):
        hwc = torch.randint(0, 256, (2, *fhw, 3), dtype=torch.uint8, device=dev)
        st = (3 * fhw[0] * fhw[1], 1, 3 * fhw[1], 3)
        cy, cx = (fhw[0] - 256) // 2, (fhw[1] - 256) // 2
        crop, whole = FrameSrc(ptr(hwc), 0, *st, *fhw, cy, cx), FrameSrc(ptr(hwc), 0, *st, *fhw, 0, 0)
        unit = torch.tensor([[cy, cx, 256, 256]] * 2, dtype=torch.float32, device=dev)
        reg = torch.tensor([_region(fhw)] * 2, dtype=torch.float32, device=dev)
        calls = {
            "stem_infer crop": lambda: L.stem_infer(dt, 2, 256, 256, 64, C.byref(crop), ptr(wf), ptr(scale), ptr(shift),
                                                    ptr(out), stream()),
            "stem_infer_roi unit": lambda: L.stem_infer_roi(dt, 2, 256, 256, 64, C.byref(whole), ptr(unit), ptr(wf),
                                                            ptr(scale), ptr(shift), ptr(out), stream()),
            f"stem_infer_roi {fhw[0] / 376:.2f}x": lambda: L.stem_infer_roi(dt, 2, 256, 256, 64, C.byref(whole), ptr(reg),
                                                                          ptr(wf), ptr(scale), ptr(shift), ptr(out),
                                                                          stream()),
            f"frames_resample {fhw[0] / 376:.2f}x": lambda: L.frames_resample(dt, 2, 256, 256, C.byref(whole), ptr(reg),
                                                                            ptr(x0), stream()),
        }
        for label, fn in calls.items():
            fn()
            torch.cuda.synchronize()
            us = [1e3 * _event_ms(fn, 200) for _ in range(3)]
            rows.append(f"stem n_img=2 256x256 {dtype} {name:5s} hwc uint8 {label:24s} "
                        + " ".join(f"{u:6.2f}" for u in us) + " us")
    return rows


def _spawn(*args) -> str:
    r = subprocess.run([sys.executable, __file__, *args], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"cell {args} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout.strip().splitlines()[-1]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="profiles/pose_roi.txt")
    ap.add_argument("--trials", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--cell", nargs=3, metavar=("ARM", "DTYPE", "CAMERA"), default=None)
    ap.add_argument("--stem", default=None, metavar="DTYPE")
    a = ap.parse_args()
    if a.cell:
        print(json.dumps(cell(*a.cell, a.trials)))
        return
    if a.stem:
        print(json.dumps(stem_cell(a.stem)))
        return
    lines = ["# Region of interest in the pose session, one MI355X, 256x256, B=1, hipGraph replay: python "
             "tools/pose_roi_table.py", f"# one process per cell, arms interleaved within a round, {a.trials} trials; "
             "ms of pose(), frames on the device -> pose", "# part dtype camera arm          round  median   min      mean"]
    summary = []
    groups = [("a", "sim", ["plain", "roi"])] + [("b", cam, ["roi", "resize+crop", "crop+resize"]) for cam in CAMERAS]
    for part, cam, arms in groups:
        for dtype in ("bf16", "fp16"):
            med = {arm: [] for arm in arms}
            for rnd in range(1, a.rounds + 1):
                for arm in arms:
                    r = json.loads(_spawn("--cell", arm, dtype, cam, "--trials", str(a.trials)))
                    med[arm].append(r["median"])
                    lines.append(f"{part}      {dtype}  {cam:6s} {arm:12s} {rnd:5d} {r['median']:8.4f} {r['min']:8.4f} "
                                 f"{r['mean']:8.4f}")
                    print(lines[-1], flush=True)
            for arm in arms[1:] if part == "b" else arms[:1]:
                num, den = (med["roi"], med[arm])
                ratios = [n / d for n, d in zip(num, den)]
                if part == "a":
                    verdict = "accepted (<= 1.05)" if statistics.median(ratios) <= 1.05 else "NOT accepted (> 1.05)"
                    summary.append(f"(a) {dtype} roi / plain per pair: " + " ".join(f"{r:.3f}" for r in ratios)
                                   + f"; median {statistics.median(ratios):.3f}: {verdict}")
                else:
                    verdict = "faster in every pair" if max(ratios) < 1 else "NOT faster in every pair"
                    summary.append(f"(b) {dtype} {cam} roi / {arm} per pair: " + " ".join(f"{r:.3f}" for r in ratios)
                                   + f"; {statistics.median(den) / statistics.median(num):.2f}x: {verdict}")
    lines += ["", "# summary"] + summary + ["", "# (c) the stem launches alone: device events around 200 back-to-back "
                                            "calls, three rounds"]
    for dtype in ("bf16", "fp16"):
        lines += json.loads(_spawn("--stem", dtype))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines[-(len(summary) + 12):]))


if __name__ == "__main__":
    main()
