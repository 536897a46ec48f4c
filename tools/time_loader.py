#!/usr/bin/env python
"""Time the batches of one epoch for each of the two loaders (no train step):

    python tools/time_loader.py [--arm both|dataloader|resident|roi|roi-track] [--samples 4096] [--batch-size 64]
                                [--workers 16] [--full-frames] [--roi-jitter LO HI SHIFT] [--rounds 3]
                                [--out profiles/resident_loader.txt]

Input: a dataset made by tests/conftest.make_dummy_dataset(..., hw=(376, 672)) (the reference's frame
size) in a temporary directory; its ten training samples are repeated through torch.utils.data.Subset
to ``--samples`` (h5lite cannot write new HDF5 files). 256 x 256 crop, ten spaghetti arcs per image.

  dataloader  DataLoader(CameraCubePoseDataset(uint8=True)) as argus_amd.train.make_loaders builds it
              (spawned persistent workers, pinned memory), each batch copied to the device; the worker
              spawn is timed apart from the epoch
  resident    ResidentDataset (the one-time ingest, timed apart) + ResidentLoader; --full-frames keeps the
              uncropped frames (every image through argus_batch_gather_resample, the center region) and
              --roi-jitter LO HI SHIFT draws a random region per camera image (implies --full-frames)
  roi         four resident loaders interleaved in one run, --rounds epochs each: (a) the cropped store,
              (b) full frames with the center region, (c) --roi-jitter 0.5 2 0.25, (d) --roi-jitter 0.25 4 0.5;
              per arm the samples/s of an epoch, the device span per batch (host-paced) and the device time of
              the batch-building launch alone (100 back-to-back launches on one batch's operands)
  roi-track   the roi arm's (c) against the same loader with roi_track (the regions aimed at the labelled cube by one
              argus_roi_from_pose launch in front of every batch), interleaved, and that launch alone

Each arm prints samples/s of one epoch, measured from the first batch request to a device synchronize
after the last batch. The fused step consumes 4,800 samples/s (13.3 ms per B=64 step).
"""
from __future__ import annotations

import argparse
import dataclasses
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import torch  # noqa: E402
from torch.utils.data import DataLoader, Subset  # noqa: E402


def roi_arms(args, cfg, aug, rep, device, say) -> None:
    """The four resident loaders of the region-of-interest comparison, interleaved epoch by epoch."""
    import numpy as np

    from argus_amd._lib import lib, ptr, stream
    from argus_amd.data import CameraCubePoseDataset
    from argus_amd.resident import ARC_WORDS, ResidentDataset, ResidentLoader

    base = CameraCubePoseDataset(dataclasses.replace(cfg, center_crop=None), None, train=True, uint8=True)
    full = ResidentDataset(cfg, aug, train=True, device=device, num_workers=args.workers, dataset=Subset(base, rep),
                           full_frames=True)
    (y0, x0), (hc, wc) = full.crop_origin, full.crop_hw
    crop = ResidentDataset.__new__(ResidentDataset)  # the same samples, cropped on the device: the parent's store
    crop.__dict__.update(full.__dict__)
    crop.full_frames = False
    crop.images = full.images[:, :, y0:y0 + hc, x0:x0 + wc].contiguous()
    say(f"roi arms: one ingest of the full frames {full.ingest_seconds:.2f} s ({full.images.numel() / 2**20:.0f} MiB; "
        f"the cropped store {crop.images.numel() / 2**20:.0f} MiB is cut from it on the device)")
    B = args.batch_size
    arms = {
        "(a) cropped store": ResidentLoader(crop, B, shuffle=True, seed=0),
        "(b) full frames, center region": ResidentLoader(full, B, shuffle=True, seed=0),
        "(c) full frames, jitter 0.5-2 shift 0.25": ResidentLoader(full, B, shuffle=True, seed=0,
                                                                   roi_jitter=(0.5, 2.0, 0.25)),
        "(d) full frames, jitter 0.25-4 shift 0.5": ResidentLoader(full, B, shuffle=True, seed=0,
                                                                   roi_jitter=(0.25, 4.0, 0.5)),
    }
    rate, span, kern = ({k: [] for k in arms} for _ in range(3))
    for loader in arms.values():  # untimed warm-up pass
        for batch in loader:
            pass
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(args.rounds):
        for name, loader in arms.items():
            loader.set_epoch(1 + r)
            t0 = time.perf_counter()
            ev0.record()
            n = k = 0
            for batch in loader:
                n += batch["images"].shape[0]
                k += 1
            ev1.record()
            torch.cuda.synchronize()
            rate[name].append(n / (time.perf_counter() - t0))
            span[name].append(ev0.elapsed_time(ev1) / k)
            # the launch alone: 100 back-to-back launches on the operands of one batch of this epoch
            ds = loader.ds
            hv = np.zeros(B * (2 + loader._roi_words + ds.n_cams * loader.n_arcs * ARC_WORDS), dtype=np.int32)
            rng, roi_rng = loader.host_generators()
            a_at = loader.fill_slot(hv, loader.indices()[:B], rng, roi_rng)
            dev = torch.from_numpy(hv).to(device)
            out = torch.empty((B, 3 * ds.n_cams, hc, wc), dtype=torch.uint8, device=device)
            arcs = dev.data_ptr() + 4 * a_at if loader.n_arcs else None

            def launch():
                if loader.full_frames:
                    lib().batch_gather_resample(B, ds.n_cams, ds.src_hw[0], ds.src_hw[1], hc, wc, ptr(ds.images), len(ds),
                                                ptr(dev), dev.data_ptr() + 8 * B, arcs, loader.n_arcs, ptr(out), stream())
                else:
                    lib().batch_gather_occlude(B, ds.n_cams, hc, wc, ptr(ds.images), len(ds), ptr(dev), arcs,
                                               loader.n_arcs, y0, x0, ptr(out), stream())

            for _ in range(5):
                launch()
            ev0.record()
            for _ in range(100):
                launch()
            ev1.record()
            torch.cuda.synchronize()
            kern[name].append(ev0.elapsed_time(ev1) / 100)
    step_ms = 13.2  # the fused B=64 step
    for name in arms:
        say(f"{name}: samples/s {' '.join(f'{v:.0f}' for v in rate[name])}; device span per batch (host-paced) "
            f"{' '.join(f'{v:.3f}' for v in span[name])} ms; launch alone {' '.join(f'{v:.3f}' for v in kern[name])} ms "
            f"= {100 * min(kern[name]) / step_ms:.1f} % of the {step_ms} ms step")


def roi_track_arms(args, cfg, aug, rep, device, say) -> None:
    """The jittered loader of the roi arm's (c) against the same loader aimed at the labelled cube
    (roi_track: one argus_roi_from_pose launch in front of every batch), interleaved epoch by epoch."""
    import ctypes as C
    import math

    import numpy as np

    from argus_amd._lib import lib, ptr, stream
    from argus_amd.data import CameraCubePoseDataset
    from argus_amd.resident import ResidentDataset, ResidentLoader
    from argus_amd.track import Camera, TrackConfig

    base = CameraCubePoseDataset(dataclasses.replace(cfg, center_crop=None), None, train=True, uint8=True)
    full = ResidentDataset(cfg, aug, train=True, device=device, num_workers=args.workers, dataset=Subset(base, rep),
                           full_frames=True)
    t = full.poses[:, :3].double().cpu().numpy()
    center, dist = t.mean(0), max(0.2, 3.0 * float(np.abs(t - t.mean(0)).max()))
    cams = []
    for s in (1.0, -1.0):  # two look-at cameras that see every labelled cube
        eye = center + dist * np.array([0.0, s * 0.15, 0.13]) / math.hypot(0.15, 0.13)
        z = (center - eye) / np.linalg.norm(center - eye)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        f = (full.src_hw[0] / 2) / math.tan(math.radians(35.0))
        cams.append(Camera(R.reshape(9), -R @ eye, f, f, full.src_hw[1] / 2, full.src_hw[0] / 2))
    track = TrackConfig(cams, 0.035, z_near=0.02)
    B = args.batch_size
    jitter = (0.5, 2.0, 0.25)
    arms = {
        "(c) full frames, jitter 0.5-2 shift 0.25": ResidentLoader(full, B, shuffle=True, seed=0, roi_jitter=jitter),
        "(e) roi_track, jitter 0.5-2 shift 0.25": ResidentLoader(full, B, shuffle=True, seed=0, roi_jitter=jitter,
                                                                 roi_track=track),
    }
    rate, span = ({k: [] for k in arms} for _ in range(2))
    valid = 0.0
    for loader in arms.values():  # untimed warm-up pass
        for batch in loader:
            if "roi_valid" in batch:
                valid = float(batch["roi_valid"].float().mean())
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(args.rounds):
        for name, loader in arms.items():
            loader.set_epoch(1 + r)
            t0 = time.perf_counter()
            ev0.record()
            n = k = 0
            for batch in loader:
                n += batch["images"].shape[0]
                k += 1
            ev1.record()
            torch.cuda.synchronize()
            rate[name].append(n / (time.perf_counter() - t0))
            span[name].append(ev0.elapsed_time(ev1) / k)
    # the new launch alone: 100 back-to-back launches on one batch's operands
    tl = arms["(e) roi_track, jitter 0.5-2 shift 0.25"]
    index = torch.arange(B, dtype=torch.int64, device=device) % len(full)
    jit = torch.zeros(B * full.n_cams, 3, dtype=torch.float32, device=device)
    roi = torch.empty(B * full.n_cams, 4, dtype=torch.float32, device=device)
    ok = torch.empty(B * full.n_cams, dtype=torch.int32, device=device)

    def launch():
        lib().roi_from_pose(B, full.n_cams, *full.src_hw, *full.crop_hw, ptr(full.poses), len(full), ptr(index),
                            ptr(tl._cameras), C.byref(tl._track_cfg), ptr(jit), ptr(tl._home), ptr(roi), None, ptr(ok),
                            stream())

    kern = []
    for _ in range(args.rounds):
        for _ in range(5):
            launch()
        ev0.record()
        for _ in range(100):
            launch()
        ev1.record()
        torch.cuda.synchronize()
        kern.append(1e3 * ev0.elapsed_time(ev1) / 100)
    for name in arms:
        say(f"{name}: samples/s {' '.join(f'{v:.0f}' for v in rate[name])}; device span per batch (host-paced) "
            f"{' '.join(f'{v:.3f}' for v in span[name])} ms")
    say(f"(e) argus_roi_from_pose alone, B={B} x {full.n_cams} images: {' '.join(f'{v:.2f}' for v in kern)} us; "
        f"{100 * valid:.0f} % of the last warm-up batch's images valid")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arm", choices=("both", "dataloader", "resident", "roi", "roi-track"), default="both")
    ap.add_argument("--full-frames", action="store_true", help="resident arm: keep the uncropped frames")
    ap.add_argument("--roi-jitter", type=float, nargs=3, metavar=("LO", "HI", "SHIFT"), default=None,
                    help="resident arm: a random region of interest per camera image (implies --full-frames)")
    ap.add_argument("--rounds", type=int, default=3, help="roi arm: timed epochs per loader")
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", type=str, default=None, help="append the result lines to this file")
    args = ap.parse_args()

    from conftest import make_dummy_dataset

    from argus_amd.data import AugmentationConfig, CameraCubePoseDataset, CameraCubePoseDatasetConfig
    from argus_amd.resident import ResidentDataset, ResidentLoader

    if not torch.cuda.is_available():
        raise SystemExit("time_loader needs the GPU (both arms end on the device)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as tmp:
        path = make_dummy_dataset(Path(tmp), hw=(376, 672))
        cfg = CameraCubePoseDatasetConfig(dataset_path=path, center_crop=(256, 256))
        aug = AugmentationConfig()
        rep = [i % 10 for i in range(args.samples)]
        say(f"time_loader: {args.samples} samples (10 distinct 376x672 two-camera frames repeated), B={args.batch_size}, "
            f"256x256 crop, {aug.num_spaghetti} arcs per image; {torch.cuda.get_device_name(device)}")

        if args.arm in ("both", "dataloader"):
            ds = Subset(CameraCubePoseDataset(cfg, aug, train=True, uint8=True, device_augmentation=True), rep)
            kw = dict(batch_size=args.batch_size, num_workers=args.workers, pin_memory=True, shuffle=True)
            if args.workers > 0:
                kw.update(multiprocessing_context="spawn", persistent_workers=True)
            loader = DataLoader(ds, **kw)
            t0 = time.perf_counter()
            it = iter(loader)  # spawns the workers
            first = next(it)
            t_spawn = time.perf_counter() - t0
            del first, it
            t0 = time.perf_counter()
            n = 0
            for batch in loader:
                images = batch["images"].to(device, non_blocking=True)
                batch["cube_pose"].to(device, non_blocking=True)
                n += images.shape[0]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            say(f"dataloader arm ({args.workers} workers): {n} samples in {dt:.3f} s = {n / dt:.0f} samples/s "
                f"({1e3 * dt * args.batch_size / n:.2f} ms per batch); worker spawn + first batch {t_spawn:.2f} s")
            del loader

        if args.arm in ("both", "resident"):
            full = args.full_frames or args.roi_jitter is not None
            base = CameraCubePoseDataset(dataclasses.replace(cfg, center_crop=None) if full else cfg, None, train=True,
                                         uint8=True)
            rds = ResidentDataset(cfg, aug, train=True, device=device, num_workers=args.workers,
                                  dataset=Subset(base, rep), full_frames=full)
            loader = ResidentLoader(rds, args.batch_size, shuffle=True, seed=0,
                                    roi_jitter=None if args.roi_jitter is None else tuple(args.roi_jitter))
            if full:
                say(f"resident arm: full frames {rds.src_hw[0]}x{rds.src_hw[1]}, regions "
                    f"{'the center crop' if args.roi_jitter is None else 'jitter ' + str(tuple(args.roi_jitter))}")
            for batch in loader:  # untimed warm-up pass: first-launch and allocator costs
                pass
            torch.cuda.synchronize()
            loader.set_epoch(1)
            t0 = time.perf_counter()
            n = 0
            for batch in loader:
                n += batch["images"].shape[0]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            say(f"resident arm: {n} samples in {dt:.3f} s = {n / dt:.0f} samples/s "
                f"({1e3 * dt * args.batch_size / n:.2f} ms per batch); one-time ingest {rds.ingest_seconds:.2f} s "
                f"({rds.images.numel() / 2**20:.0f} MiB on the device)")
            # where a batch's time goes: the host draw of the arc records against the launch
            import numpy as np

            from argus_amd.resident import arc_records, sample_arcs

            rng = np.random.RandomState(0)
            t0 = time.perf_counter()
            for _ in range(50):
                arc_records(sample_arcs(rng, args.batch_size * rds.n_cams, rds.num_spaghetti, rds.src_hw))
            t_host = (time.perf_counter() - t0) / 50
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            loader.set_epoch(2)
            ev0.record()
            k = 0
            for batch in loader:
                k += 1
            ev1.record()
            torch.cuda.synchronize()
            say(f"resident arm detail: host arc draw {1e3 * t_host:.3f} ms per batch; device span of an epoch "
                f"{ev0.elapsed_time(ev1) / k:.3f} ms per batch (copy + gather/arc kernel + pose gather, host-paced)")

        if args.arm == "roi":
            roi_arms(args, cfg, aug, rep, device, say)
        if args.arm == "roi-track":
            roi_track_arms(args, cfg, aug, rep, device, say)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
