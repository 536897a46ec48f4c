#!/usr/bin/env python
"""Benchmark of the argus training hot path on MI355X (BASELINE.json metric / configs[1]).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch 64] [--hw 256 256] [--dtype bf16]
                    [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N

A plain run does only what the headline figure needs: set up, W warm-up steps, K timed steps, the
result line (metric, value, unit, higher_is_better, dtype, ms_per_step and the workload's description).
--full adds everything listed under "With --full also reported" below, each with runs of its own
outside the timed region. --dump-outputs DIR writes what the last timed step handed its caller
(DIR/<name>.npy, float32; see dump_outputs) so that two builds can be compared output for output: with
the same arguments the inputs and the initial weights are the same from run to run.

A step = one fused native train step (argus/train.py:298-320) on a device-resident synthetic batch:
images (B, 6, H, W) fp32 in [0,1] (uint8-uniform pixels / 255, seed 1000+rank) and SE(3) targets
Exp(xi), xi ~ N(0, 0.5^2) (seed 2000+rank) -> NCameraCNN forward (bf16 HIP kernels) -> SE(3) loss ->
backward -> [RCCL SUM all-reduce, bucketed, overlapped] -> clip_grad_norm_(1.0) -> Adam(1e-4).
Weights: seeded random init (torch.manual_seed(42)) of the reference architecture.
value = images/s over all ranks (one sample = 2 camera images); weak scaling (B per rank fixed).

With --full also reported:
  roofline     - the dominant kernel instantiation (conv GEMM or BN pass; largest total time in one
                 probe step),
                 timed live over the timed region by the library's kernel timer (start/stop HIP
                 events carried by each of its dispatch packets, on its launch stream). bound =
                 "mfma" if its algorithmic FLOP/byte is above the ridge (peak FLOP/s / 8 TB/s), else
                 "hbm"; achieved = algorithmic FLOPs (or bytes) per launch / average launch time;
                 peak = dense bf16 MFMA (or HBM); traffic = measured HBM bytes per launch from the
                 committed PMC summary of this workload (tools/pmc_traffic.py).
  cpu_baseline - the CPU oracle (the reference's torch.nn ops on CPU, fp32, B=8) train step timed on
                 this host (rank 0, N=1), a bounded sample of ~15 s.
  val_loss     - mean SE(3) loss (argus/train.py:342) of the trained model in eval mode on a
                 synthetic held-out batch; val_se3_log_rms = sqrt(val_loss) (the RMS norm of the
                 full se(3) log, translation included); val_rot_err_deg = mean rotation-angle
                 component |phi| of the geodesic. The data is synthetic, so the value
                 itself says nothing about accuracy; val_vs_oracle is the same validation by the CPU
                 fp32 oracle with the same trained weights (rank 0, first 16 samples): the gap between
                 the two is the metric's error half (north_star: pose error within 1e-4 at fp32).
Batch: 64 samples per rank (configs[1]) at every N, so the driver's N = 1, 2, 4, 8 lines form one
weak-scaling series (per-GPU work fixed); --batch 256 gives configs[2]'s per-rank batch
(cube_unity_data_medium-shaped), --batch overrides in general.
"""
from __future__ import annotations

import argparse
import json
import sys
import math
import os
import time
from pathlib import Path

import torch
import torch.distributed as dist

BF16_DENSE_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: ~2.5 PF dense bf16 MFMA
F32_MFMA_PEAK_TFLOPS = 157.3
FP8_DENSE_PEAK_TFLOPS = 5000.0  # MI355X_MICROARCH.md: ~5 PF dense fp8 MFMA
HBM_PEAK_GBS = 8000.0


def synthetic_batch(B, H, W, seed, device):
    from argus_amd.utils import se3_exp

    g = torch.Generator(device=device).manual_seed(seed)
    images = torch.randint(0, 256, (B, 6, H, W), generator=g, device=device, dtype=torch.uint8).float() / 255.0
    xi = torch.randn(B, 6, generator=g, device=device) * 0.5
    targets = se3_exp(xi, canonical_w=True)
    return images, targets


def _config_name(B: int, H: int, W: int, world: int) -> str:
    """Which BASELINE.json config this run's shape is (configs[1] is the default bench line)."""
    if (H, W) == (376, 672):
        return "configs[3] cube_unity_data_large-shaped (2-cam 376x672)"
    if (H, W) == (256, 256) and B == 512:
        return "configs[4] fp8-shaped (B=512 per rank)"
    if (H, W) == (256, 256) and B == 256:
        return "configs[2] cube_unity_data_medium-shaped"
    if (H, W) == (256, 256) and B == 64:
        return "configs[1] cube_unity_data_small-shaped"
    return f"custom ({H}x{W}, batch {B} per rank)"


def _newest_summary(pattern: str, B: int, H: int, W: int, dtype: str):
    """The newest committed PMC summary (profiles/<pattern>) of this exact workload, or None. Only the
    newest one (by name: rNN<tag>_..., later rounds and tags sort later) is consulted: an older summary
    is of older code, so a kernel missing from the newest reads None, not an older profile's figure."""
    for p in sorted(Path(__file__).resolve().parent.glob(f"profiles/{pattern}"), key=lambda p: p.name)[::-1]:
        d = json.loads(p.read_text())
        if d.get("meta", {}).get("workload") == [B, H, W, dtype]:
            return p, d
    return None, None


def pmc_traffic(kernel: str, B: int, H: int, W: int, dtype: str):
    """HBM bytes per launch of ``kernel`` (its exact demangled name, which the kernel timer's labels use)
    from the newest committed PMC summary of this exact workload (profiles/*_pmc_traffic.json, written
    by tools/pmc_traffic.py from separate FETCH_SIZE and WRITE_SIZE rocprofv3 passes of this bench
    command). None when that summary lacks the kernel."""
    _, d = _newest_summary("*_pmc_traffic.json", B, H, W, dtype)
    v = (d or {}).get("kernels", {}).get(kernel)
    return round(v["traffic_bytes_per_launch"]) if v else None


def pmc_mfma(kernel: str, B: int, H: int, W: int, dtype: str):
    """MFMA-pipe busy fraction of ``kernel`` (SQ_VALU_MFMA_BUSY_CYCLES over 4 SIMD x 256 CU x kernel
    cycles) and its wave-state split, from the newest committed PMC summary of this workload
    (profiles/*_pmc_mfma_summary.json, tools/prof_pmc.sh). None when that summary lacks the kernel."""
    p, d = _newest_summary("*_pmc_mfma_summary.json", B, H, W, dtype)
    v = (d or {}).get("kernels", {}).get(kernel)
    if not v or "mfma_busy" not in v:
        return None
    return {"mfma_busy": round(v["mfma_busy"], 4), "wait_frac": round(v.get("wait_frac", 0), 3),
            "issue_stall_frac": round(v.get("issue_stall_frac", 0), 3),
            "active_frac": round(v.get("active_frac", 0), 3), "source": p.name}


def cpu_model() -> str:
    """The host CPU's model name (/proc/cpuinfo), as BASELINE.md asks the CPU baseline to state."""
    try:
        for line in Path("/proc/cpuinfo").read_text().splitlines():
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def oracle_validation(model, vimg: torch.Tensor, vtgt: torch.Tensor) -> dict:
    """The validation pass of argus/train.py:327-348 (eval mode, running BN statistics, mean SE(3) loss)
    on the held-out batch, by the CPU oracle carrying this model's trained weights and buffers: fp32
    (the reference's numbers for the same weights), under the reference's real --amp mode (fp16 autocast,
    argus/train.py:298-299,334-335) and under bf16 autocast (the dtype of our path; a yardstick this
    project chose, not a mode the reference runs)."""
    from oracle import se3
    from oracle.ncamera import build_reference_model

    ref = build_reference_model(42)
    ref.load_state_dict({k: v.detach().float().cpu() for k, v in model.state_dict().items()})
    ref.eval()
    out = {}
    with torch.no_grad():
        x = vimg.cpu().float()
        for mode, dt in (("fp32", None), ("fp16_autocast", torch.float16), ("bf16_autocast", torch.bfloat16)):
            with torch.autocast("cpu", dtype=dt or torch.bfloat16, enabled=dt is not None):
                pred = ref(x)
            pred = pred.float()
            out[mode] = {"pred": pred, "loss": se3.geometric_loss(pred.double(), vtgt.cpu().double())}
    return out


# the stated eval-mode tolerances of the val_vs_oracle check: fp32 within north_star's
# 1e-4; the reduced-precision paths within 2x (bf16) / 4x (fp8: e4m3 keeps 3 mantissa bits to bf16's 7)
# the distance of the reference model under CPU bf16 autocast from fp32 - a yardstick chosen by this
# project for a bf16 path (the same bars as tests/test_gpu_parity.py::test_lowp_eval_predictions_at_trained_point),
# both on max |pred diff| and on max |per-sample loss diff|. The reference's own --amp mode is fp16
# autocast (argus/train.py:298-299): its distance is reported beside it, with our ratio to it, and an
# absolute bound VAL_LOWP_ABS caps the relative bar so it cannot only loosen
VAL_FP32_TOL = 1e-4
VAL_LOWP_FACTOR = {"bf16": 2.0, "fp8": 4.0}
VAL_LOWP_ABS = {"bf16": {"pred": 0.25, "per_sample_loss": 0.5}, "fp8": {"pred": 0.5, "per_sample_loss": 1.0}}


def cpu_share() -> int:
    """Threads for the CPU legs: the host's CPU share for one GPU, not the whole machine. The GPU box
    runs one job per GPU on a shared many-core host (os.cpu_count() reports all of its cores, e.g. 64 on
    an EPYC 9575F, shared by 8 GPUs' jobs) and exports OMP_NUM_THREADS=16 as this job's share; more
    threads than the share would time CPU cores other jobs hold."""
    try:
        share = int(os.environ.get("OMP_NUM_THREADS", "16"))
    except ValueError:
        share = 16
    return max(1, min(share, 16, os.cpu_count() or 1))


def cpu_baseline(batch: int, H: int, W: int, budget_s: float = 15.0) -> dict:
    """Oracle (CPU restatement of the reference model, same torch CPU ops) fwd+loss+bwd+clip+Adam."""
    from oracle import se3
    from oracle.ncamera import build_reference_model

    threads = cpu_share()
    torch.set_num_threads(threads)
    model = build_reference_model(42)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(1000)
    x = torch.randint(0, 256, (batch, 6, H, W), generator=g, dtype=torch.uint8).float() / 255.0
    T = se3.random_targets(batch, generator=g)

    def step():
        losses = se3.geometric_loss(model(x), T)
        opt.zero_grad()
        losses.mean().backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()

    step()  # warm-up
    n, t0 = 0, time.perf_counter()
    while n < 2 or (time.perf_counter() - t0 < budget_s and n < 24):
        step()
        n += 1
    dt = time.perf_counter() - t0
    return {"value": round(2 * batch * n / dt, 3), "unit": "images/s", "cores": threads, "kind": "port",
            "cpu_model": cpu_model(), "host_cpus": os.cpu_count(),
            "cores_note": "the job's CPU share for one GPU (OMP_NUM_THREADS, 16 on the GPU box), not the "
                          "whole host: the other cores belong to the other GPUs' jobs",
            "sample": f"oracle (reference torch.nn ops on CPU) fp32 train step, batch {batch} samples "
                      f"({2 * batch} images) of {H}x{W}, {n} timed steps after 1 warm-up, {dt:.1f} s"}


def needs_launch(gpus: int, env) -> bool:
    """True when this process is the user-facing ``bench.py --gpus N`` (N > 1) and no launcher has set
    up the ranks (WORLD_SIZE unset): it must start the N rank processes itself. The reference's own
    multi-GPU entry does the same (mp.spawn(..., nprocs=cfg.num_gpus), argus/train.py:373-376)."""
    return gpus > 1 and "WORLD_SIZE" not in env


def launcher_argv(gpus: int, port: int, argv: list[str], script: str | None = None) -> list[str]:
    """Child command that runs N ranks of this bench, one process per GPU: torch.distributed.run on one
    node with a 127.0.0.1 rendezvous (the container hostname may not resolve); ``argv`` is this
    process's own argument list (``--gpus N`` included), passed to every rank unchanged."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
            "--master-addr=127.0.0.1", f"--master-port={port}", script or str(Path(__file__).resolve()), *argv]


def check_world(gpus: int, world: int) -> None:
    """Each rank asserts that it runs in a world of exactly ``--gpus`` ranks (a launcher with another
    --nproc-per-node must not produce a line labelled with the wrong GPU count)."""
    if world != gpus:
        raise SystemExit(f"bench.py: --gpus {gpus} but WORLD_SIZE={world}; launch N ranks with --gpus N")


def _free_port() -> int:
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(gpus: int, argv: list[str], script: str | None = None) -> int:
    """Start the N rank processes (before this process touches the GPU: it only imported torch) and
    return their launcher's exit status; rank 0 prints the JSON line to the shared stdout."""
    import subprocess

    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this host driver (RCCL)
    return subprocess.call(launcher_argv(gpus, _free_port(), argv, script), env=env)


def timed_steps(trainer, images, targets, steps: int, world: int):
    """The timed region: ``steps`` fused train steps between two device synchronisations (and two
    barriers when there are several ranks). Returns (seconds, the last step's per-sample losses)."""
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    losses = None
    t0 = time.perf_counter()
    for _ in range(steps):
        losses = trainer.step(images, targets)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    return time.perf_counter() - t0, losses


DUMP_SAMPLE = 1 << 20  # elements kept of each flat buffer (4 MiB as float32)


def step_outputs(trainer, losses: torch.Tensor) -> dict:
    """What the caller of FusedTrainer.step holds after a step, as float32 CPU tensors: the per-sample
    losses it returns, the gradient norm, and the state it leaves behind - the gradients, the updated
    parameters (a fixed, seeded sample of DUMP_SAMPLE elements of each flat buffer, in index order) and
    the model's floating-point buffers (the BN running statistics) in named_buffers() order."""
    flat = trainer.flat
    if flat.total > DUMP_SAMPLE:
        g = torch.Generator().manual_seed(20240)
        idx = torch.randint(0, flat.total, (DUMP_SAMPLE,), generator=g).sort().values.to(flat.param.device)
        grad, param = flat.grad[idx], flat.param[idx]
    else:
        grad, param = flat.grad, flat.param
    bufs = [b.detach().flatten().float() for _, b in trainer.model.named_buffers() if b.is_floating_point()]
    out = {"losses": losses, "grad_norm": trainer.grad_norm(), "grad_sample": grad, "param_sample": param}
    if bufs:
        out["running_stats"] = torch.cat(bufs)
    return {k: v.detach().float().cpu().clone() for k, v in out.items()}


def dump_outputs(directory: str, outputs: dict) -> None:
    """Write each array of ``outputs`` as <directory>/<name>.npy (float32)."""
    import numpy as np

    d = Path(directory)
    d.mkdir(parents=True, exist_ok=True)
    for name, t in outputs.items():
        np.save(d / f"{name}.npy", t.numpy().astype(np.float32, copy=False))


def headline(args, world: int, B: int, H: int, W: int, elapsed: float) -> dict:
    """The head of the result line: the throughput figure, the time of one timed step and the
    description of the workload."""
    images_per_s = world * B * 2 * args.steps / elapsed
    return {
        "metric": f"train images/sec + val SE(3) geodesic err, 2x{H}x{W} RGB",
        "value": round(images_per_s, 2),
        "unit": "images/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": args.dtype,
        "dtype_detail": ("OCP MX-fp8 (e4m3 + E8M0 scale per 32 K-elements) operands for the 3x3 conv forward "
                         "(stride 1) and data-gradient GEMMs with >= 128 reduction channels (policy key 37); the "
                         "stride-1 ones read MX-fp8 copies of their inputs that the BN apply passes store beside "
                         "the bf16 tensors; bf16 tensors, BN, 1x1 convs, weight gradients and the 64-channel "
                         "convs; fp32 accumulation, statistics, head, optimizer"
                         if args.dtype == "fp8" else None),
        "data": "synthetic (uint8-uniform images, Exp(N(0,0.5^2)) SE(3) targets, seeded random-init weights)",
        "config": {
            "workload": f"{_config_name(B, H, W, world)}: fused train step, {B} samples "
                        f"({2 * B} images) of {H}x{W} per rank, 2 cams, ResNet-50 + MLP head, {args.dtype}",
            "batch_per_rank": B, "global_batch": B * world, "image_hw": [H, W], "parallelism": f"dp{world}",
            "baseline_config": _config_name(B, H, W, world).split(" ")[0],
            "scaling_series": ("weak: the same per-rank batch at every N (the default 64 is configs[1]'s; configs[2], "
                               "the 8-GPU B=256-per-rank line, is --batch 256)"),
        },
        "samples_per_s": round(images_per_s / 2, 2),
    }


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None,
                    help="samples (camera pairs) per rank (default 64 = configs[1] at every N: weak scaling; "
                         "256 = configs[2]'s per-rank batch)")
    ap.add_argument("--hw", type=int, nargs=2, default=(256, 256))
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp8"])
    ap.add_argument("--full", action="store_true",
                    help="also measure and report everything beside the headline figure (roofline and critical-"
                         "path kernel timers, validation against the CPU oracle, CPU baseline); the options below "
                         "shape those legs and need --full")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step handed its caller as DIR/<name>.npy (rank 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--kernels", action="store_true", help="print the probe step's per-kernel table to stderr (implies --full)")
    ap.add_argument("--no-isolated", action="store_true",
                    help="skip the two untimed no-overlap steps that measure the dominant kernel alone")
    ap.add_argument("--no-val-oracle", action="store_true", help="skip the CPU oracle validation check")
    ap.add_argument("--val-oracle-batch", type=int, default=16,
                    help="held-out samples the CPU fp32 oracle validates (rank 0)")
    ap.add_argument("--tune", nargs="*", default=[],
                    help="dev: kernel-selection overrides key=value (argus_conv_policy_default keys)")
    args = ap.parse_args()
    args.full = args.full or args.kernels  # the table is of the probe steps, which only a full run takes
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if needs_launch(args.gpus, os.environ):
        sys.exit(launch(args.gpus, sys.argv[1:]))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    check_world(args.gpus, world)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # rehearsal knob (dev only): ARGUS_BENCH_REHEARSE=1 puts every rank on cuda:0 and exchanges over
    # gloo, so the N>1 code path can be exercised on a one-GPU box (RCCL refuses two ranks per device)
    rehearse = os.environ.get("ARGUS_BENCH_REHEARSE", "0") == "1"
    if rehearse:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if rehearse:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    from argus_amd.models import NCameraCNN
    from argus_amd.profiling import KernelTimer
    from argus_amd.step import FusedTrainer
    from argus_amd.losses import geometric_loss_fn

    tuning = {int(k): int(v) for k, v in (kv.split("=") for kv in args.tune)}
    B, (H, W) = (args.batch or 64), args.hw
    torch.manual_seed(42)
    model = NCameraCNN(compute_dtype=args.dtype, kernel_tuning=tuning or None).to(dev)
    model.train()
    trainer = FusedTrainer(model, lr=1e-4, max_grad_norm=1.0)
    images, targets = synthetic_batch(B, H, W, 1000 + rank, dev)

    for _ in range(args.warmup):
        trainer.step(images, targets)
    if not args.full:  # the plain run: the timed steps, their outputs, the headline
        elapsed, losses = timed_steps(trainer, images, targets, args.steps, world)
        el = torch.tensor([elapsed], device=dev)
        if world > 1:
            dist.all_reduce(el, op=dist.ReduceOp.MAX)
        if rank == 0:
            out = headline(args, world, B, H, W, el.item())
            out["train_loss"] = round(losses.mean().item(), 6)
            out["max_memory_allocated_gb"] = round(torch.cuda.max_memory_allocated(dev) / 2**30, 3)
            if args.dump_outputs:
                dump_outputs(args.dump_outputs, step_outputs(trainer, losses))
            print(json.dumps(out), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return
    # find the dominant kernel instantiation (largest total time) over three instrumented steps (the
    # two 128x128 weight-gradient instantiations are within ~10 % of each other: one step's noise
    # could pick either)
    probe = KernelTimer()
    probe.start()
    nprobe = 3
    for _ in range(nprobe):
        trainer.step(images, targets)
    summ = probe.summary()
    probe.stop()
    dom = max(summ, key=lambda k: summ[k]["total_ms"])
    # the critical path: the main stream (the dgrad / BN chain; weight gradients run beside it on a
    # side stream) - its kernel instantiation with the largest total time
    main_stream = torch.cuda.current_stream().cuda_stream
    mprobe = KernelTimer(stream=main_stream)
    mprobe.start()
    for _ in range(nprobe):
        trainer.step(images, targets)
    msumm = mprobe.summary()
    mprobe.stop()
    crit = max(msumm, key=lambda k: msumm[k]["total_ms"])
    if args.kernels and rank == 0:
        for k, v in sorted(summ.items(), key=lambda kv: -kv[1]["total_ms"]):
            us = v["avg_us"]
            print(f"{v['total_ms'] / nprobe:7.3f} ms {v['launches'] // nprobe:4d}x {us:8.1f} us {v['tflops']:7.1f} TF "
                  f"{v['bytes_per_launch'] / us / 1e3:7.0f} GB/s  {k}", file=sys.stderr)
    timer = KernelTimer(dom)  # exact-name prefix: only this instantiation is timed

    torch.cuda.synchronize()
    if trainer.distributed:
        trainer.tail_events = []
    timer.start()
    elapsed, losses = timed_steps(trainer, images, targets, args.steps, world)
    timer.stop()
    if rank == 0 and args.dump_outputs:  # before the untimed steps below change them
        dump_outputs(args.dump_outputs, step_outputs(trainer, losses))
    tail_ms = None
    if trainer.tail_events:
        tail_ms = sum(a.elapsed_time(b) for a, b in trainer.tail_events) / len(trainer.tail_events)
        trainer.tail_events = None
    el = torch.tensor([elapsed], device=dev)
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = el.item()
    train_loss = losses.mean().item()

    ks = timer.summary()[dom]  # read before the next timer starts (the native timer is per process)

    # the same kernel without the side-stream overlap (untimed, after the timed region): its duration
    # when it has the GPU to itself, reported beside the concurrent figure
    eng = model._engine(dev)
    iso_s = None
    if not args.no_isolated:
        iso = KernelTimer(dom)
        eng.wgrad_overlap = False
        iso.start()
        for _ in range(2):
            trainer.step(images, targets)
        iso_s = iso.summary().get(dom)
        iso.stop()
        eng.wgrad_overlap = True

    # the critical-path kernel, timed live (overlap on) over a few more steps after the timed region
    ncrit = 5
    ctimer = KernelTimer(crit, stream=main_stream)
    ctimer.start()
    for _ in range(ncrit):
        trainer.step(images, targets)
    cs = ctimer.summary()[crit]
    ctimer.stop()
    main_busy_ms = sum(v["total_ms"] for v in msumm.values()) / nprobe

    # validation SE(3) error (eval mode, running BN statistics) of the trained weights on a synthetic
    # held-out batch (seed 5000 + rank, never trained on), and the same validation by the CPU fp32 oracle
    # with the same weights and buffers (rank 0): the metric's error half against the reference
    model.eval()
    vimg, vtgt = synthetic_batch(B, H, W, 5000 + rank, dev)
    from argus_amd.utils import rotation_angle_error

    with torch.no_grad():
        vpred = model(vimg)
        vloss = geometric_loss_fn(vpred, vtgt)
        vrot = rotation_angle_error(vpred, vtgt)
    vsum = torch.stack([vloss.sum(), vrot.sum(), torch.tensor(float(vloss.numel()), device=dev)])
    if world > 1:
        dist.all_reduce(vsum)
    val_loss = (vsum[0] / vsum[2]).item()
    val_rot = (vsum[1] / vsum[2]).item()
    val_oracle = None
    if rank == 0 and not args.no_val_oracle:
        nv = min(B, args.val_oracle_batch)
        torch.set_num_threads(cpu_share())
        o = oracle_validation(model, vimg[:nv], vtgt[:nv])
        o32, o16, oh = o["fp32"], o["bf16_autocast"], o["fp16_autocast"]
        ours = geometric_loss_fn(vpred[:nv], vtgt[:nv]).double().cpu()
        d_pred = (vpred[:nv].float().cpu() - o32["pred"]).abs().max().item()
        d_loss = (ours - o32["loss"]).abs().max().item()
        r_pred = (o16["pred"] - o32["pred"]).abs().max().item()
        r_loss = (o16["loss"] - o32["loss"]).abs().max().item()
        h_pred = (oh["pred"] - o32["pred"]).abs().max().item()
        h_loss = (oh["loss"] - o32["loss"]).abs().max().item()
        if args.dtype == "fp32":
            bar_pred = bar_loss = VAL_FP32_TOL
            bar = f"fp32: |pred diff| and |per-sample loss diff| <= {VAL_FP32_TOL:g} (north_star)"
        else:
            fac, cap = VAL_LOWP_FACTOR[args.dtype], VAL_LOWP_ABS[args.dtype]
            bar_pred, bar_loss = min(fac * r_pred, cap["pred"]), min(fac * r_loss, cap["per_sample_loss"])
            bar = (f"{args.dtype}: <= {fac:g}x the distance of the reference model under CPU bf16 autocast from "
                   f"fp32 (a yardstick chosen by this project for a bf16 path; the reference's own --amp is fp16 "
                   f"autocast, argus/train.py:298-299, reported beside it), capped at {cap['pred']:g} (pred) / "
                   f"{cap['per_sample_loss']:g} (per-sample loss), on the same weights and samples")
        val_oracle = {
            "samples": nv,
            "val_loss_gpu": round(ours.mean().item(), 6),
            "val_loss_oracle_fp32": round(o32["loss"].mean().item(), 6),
            "val_loss_oracle_fp16_autocast": round(oh["loss"].mean().item(), 6),
            "val_loss_oracle_bf16_autocast": round(o16["loss"].mean().item(), 6),
            "val_loss_abs_diff": float(f"{abs(ours.mean().item() - o32['loss'].mean().item()):.3e}"),
            "pred_max_abs_diff": float(f"{d_pred:.3e}"),
            "per_sample_loss_max_abs_diff": float(f"{d_loss:.3e}"),
            "ref_fp16_autocast_pred_max_abs_diff": float(f"{h_pred:.3e}"),
            "ref_fp16_autocast_per_sample_loss_max_abs_diff": float(f"{h_loss:.3e}"),
            "ratio_to_ref_fp16_autocast": {"pred": float(f"{d_pred / max(h_pred, 1e-30):.3g}"),
                                           "per_sample_loss": float(f"{d_loss / max(h_loss, 1e-30):.3g}")},
            "ref_bf16_autocast_pred_max_abs_diff": float(f"{r_pred:.3e}"),
            "ref_bf16_autocast_per_sample_loss_max_abs_diff": float(f"{r_loss:.3e}"),
            "tolerance": {"pred": float(f"{bar_pred:.3e}"), "per_sample_loss": float(f"{bar_loss:.3e}"), "rule": bar},
            "within_tolerance": bool(d_pred <= bar_pred and d_loss <= bar_loss),
            "note": f"eval-mode validation (argus/train.py:327-348) of the trained weights on the first {nv} "
                    f"held-out samples: the {args.dtype} HIP path, and the reference model under CPU fp16 autocast "
                    f"(its --amp mode) and bf16 autocast, each vs the CPU fp32 oracle with the same weights",
        }

    # the dominant kernel's own MFMA roof: MX-fp8 igemm variants (template flag 32) and the fp8 halo
    # kernel (its fourth template argument, F8, true) run at the dense fp8 rate; in an "fp8" run the weight
    # gradients and the 64-channel convs stay bf16
    f8_kernel = ((dom.startswith("argus::igemm_kernel<") and int(dom.rstrip(">").split(",")[-1]) >= 32) or
                 (dom.startswith("argus::conv3x3_halo_kernel<") and dom.rstrip(">").split(", ")[3] == "true"))
    peak_flops = (FP8_DENSE_PEAK_TFLOPS if f8_kernel else
                  BF16_DENSE_PEAK_TFLOPS if args.dtype in ("bf16", "fp8") else F32_MFMA_PEAK_TFLOPS)
    tflops = ks["flops_per_launch"] / (ks["avg_us"] * 1e-6) / 1e12
    gbs = ks["bytes_per_launch"] / (ks["avg_us"] * 1e-6) / 1e9
    # the roof that binds: MFMA if the kernel's algorithmic intensity is above the ridge, else HBM
    compute_bound = ks["flops_per_launch"] / ks["bytes_per_launch"] > peak_flops * 1e12 / (HBM_PEAK_GBS * 1e9)
    ms = 1e3 * elapsed / args.steps

    def roof_of(k):  # {bound, achieved, peak, unit, frac} of one kernel timer record
        tf = k["flops_per_launch"] / (k["avg_us"] * 1e-6) / 1e12
        gb = k["bytes_per_launch"] / (k["avg_us"] * 1e-6) / 1e9
        mf = k["flops_per_launch"] / max(k["bytes_per_launch"], 1.0) > peak_flops * 1e12 / (HBM_PEAK_GBS * 1e9)
        return {"bound": "mfma" if mf else "hbm", "achieved": round(tf, 2) if mf else round(gb, 1),
                "peak": peak_flops if mf else HBM_PEAK_GBS, "unit": "TFLOP/s" if mf else "GB/s",
                "frac": round(tf / peak_flops if mf else gb / HBM_PEAK_GBS, 4),
                "achieved_tflops": round(tf, 2), "achieved_gbs": round(gb, 1)}
    # algorithmic conv FLOPs per step: fwd + dgrad + wgrad (the stem has no dgrad)
    step_flops = sum((2 if n == "resnet.conv1" else 3) * c.flops for n, c in eng.convs.items())
    out = {
        **headline(args, world, B, H, W, elapsed),
        "rccl_world_size": dist.get_world_size() if world > 1 else 1,
        "collective_backend": (dist.get_backend() if world > 1 else None),
        "allreduce_tail_ms_per_step": round(tail_ms, 4) if tail_ms is not None else None,
        "allreduce_bytes_per_step": (trainer.flat.total * 4 if world > 1 else 0),
        "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated(dev) / 2**30, 3),
        "roofline": {
            "bound": "mfma" if compute_bound else "hbm", "kernel": dom, "launches": ks["launches"],
            "flops_per_launch": round(ks["flops_per_launch"]), "algorithmic_bytes_per_launch": round(ks["bytes_per_launch"]),
            "avg_launch_us": round(ks["avg_us"], 3),
            "achieved": round(tflops, 2) if compute_bound else round(gbs, 1),
            "peak": peak_flops if compute_bound else HBM_PEAK_GBS,
            "unit": "TFLOP/s" if compute_bound else "GB/s",
            "frac": round(tflops / peak_flops if compute_bound else gbs / HBM_PEAK_GBS, 4),
            "intensity_flop_per_byte": round(ks["flops_per_launch"] / ks["bytes_per_launch"], 1),
            "achieved_tflops": round(tflops, 2), "frac_of_mfma_peak": round(tflops / peak_flops, 4),
            "achieved_gbs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
            "traffic": pmc_traffic(dom, B, H, W, args.dtype),
            "mfma_counters": pmc_mfma(dom, B, H, W, args.dtype),
            "concurrency": "weight-gradient kernels run on a side stream, overlapped with the main-stream "
                           "dgrad/BN chain; avg_launch_us is measured while sharing the GPU",
            "isolated_avg_launch_us": round(iso_s["avg_us"], 3) if iso_s else None,
            "isolated_launches": iso_s["launches"] if iso_s else None,
            "isolated_flops_per_launch": round(iso_s["flops_per_launch"]) if iso_s else None,
            "isolated_frac": (round((iso_s["flops_per_launch"] / (iso_s["avg_us"] * 1e-6) / 1e12) / peak_flops
                                    if compute_bound else
                                    iso_s["bytes_per_launch"] / (iso_s["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
                              if iso_s else None),
        },
        "critical_path": {
            "kernel": crit, "stream": "main (dgrad / BN chain)", "launches_per_step": msumm[crit]["launches"] // nprobe,
            "ms_per_step": round(msumm[crit]["total_ms"] / nprobe, 3),
            "flops_per_launch": round(cs["flops_per_launch"]), "algorithmic_bytes_per_launch": round(cs["bytes_per_launch"]),
            "avg_launch_us": round(cs["avg_us"], 3), "timed_steps": ncrit, **roof_of(cs),
            "traffic": pmc_traffic(crit, B, H, W, args.dtype),
            "mfma_counters": pmc_mfma(crit, B, H, W, args.dtype),
            "main_stream_busy_ms_per_step": round(main_busy_ms, 3),
        },
        "step_conv_tflops_per_gpu": round(step_flops / (ms * 1e-3) / 1e12, 2),
        "step_conv_frac_of_bf16_peak": round(step_flops / (ms * 1e-3) / 1e12 / BF16_DENSE_PEAK_TFLOPS, 4),
        "train_loss": round(train_loss, 6),
        "val_loss": round(val_loss, 6),
        "val_se3_log_rms": round(math.sqrt(max(val_loss, 0.0)), 6),
        "val_rot_err_deg": round(math.degrees(val_rot), 4),
        "val_vs_oracle": val_oracle,
    }
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(8, H, W, args.cpu_seconds)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
