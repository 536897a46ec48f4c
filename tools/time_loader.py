#!/usr/bin/env python
"""Time the batches of one epoch for each of the two loaders (no train step):

    python tools/time_loader.py [--arm both|dataloader|resident] [--samples 4096] [--batch-size 64]
                                [--workers 16] [--out profiles/resident_loader.txt]

Input: a dataset made by tests/conftest.make_dummy_dataset(..., hw=(376, 672)) (the reference's frame
size) in a temporary directory; its ten training samples are repeated through torch.utils.data.Subset
to ``--samples`` (h5lite cannot write new HDF5 files). 256 x 256 crop, ten spaghetti arcs per image.

  dataloader  DataLoader(CameraCubePoseDataset(uint8=True)) as argus_amd.train.make_loaders builds it
              (spawned persistent workers, pinned memory), each batch copied to the device; the worker
              spawn is timed apart from the epoch
  resident    ResidentDataset (the one-time ingest, timed apart) + ResidentLoader

Each arm prints samples/s of one epoch, measured from the first batch request to a device synchronize
after the last batch. The fused step consumes 4,800 samples/s (13.3 ms per B=64 step).
"""
from __future__ import annotations

import argparse
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import torch  # noqa: E402
from torch.utils.data import DataLoader, Subset  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arm", choices=("both", "dataloader", "resident"), default="both")
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
            base = CameraCubePoseDataset(cfg, None, train=True, uint8=True)
            rds = ResidentDataset(cfg, aug, train=True, device=device, num_workers=args.workers,
                                  dataset=Subset(base, rep))
            loader = ResidentLoader(rds, args.batch_size, shuffle=True, seed=0)
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
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
