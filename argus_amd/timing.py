"""Forward-latency benchmark — the MI355X counterpart of the reference's ``scripts/timing.py``.

    python -m argus_amd.timing [--trials 100] [--batch 2] [--hw 256 256] [--dtype fp32|bf16x3|bf16]
                               [--eval] [--no-graph] [--frozen [--dtype fp16]]
    python -m argus_amd.timing --frozen --pose [--layout hwc --frame-hw Hs Ws] [--parent] [--roi Y X H W] [--track CALIB.json]
    python -m argus_amd.timing --input-grad [--out profiles/input_grad.txt]

Reference semantics (scripts/timing.py:10-48): ``NCameraCNN(n_cams=2)`` in fp32 on the GPU, left in
its default (train) mode — BatchNorm uses batch statistics — a fresh ``torch.rand((2, 6, 256, 256))``
batch per trial, ``torch.no_grad()``, 100 timed trials after one untimed first call, each trial timed
with device events by ``time_torch_fn`` (argus/utils.py:153-171).

The reference compiles the model with ``torch.compile(mode="reduce-overhead")``, i.e. it replays a
captured device graph. The equivalent here is a hipGraph of the whole native forward (every HIP
launch of ``ResNetEngine.forward`` on one captured stream), replayed per trial after the new batch is
copied into the graph's static input buffer; ``--no-graph`` times eager launches instead.

``--frozen`` times an ``argus_amd.infer.InferenceSession`` built from the model in eval mode instead (BN
folded into the conv weights, one launch per conv, its own captured graph): the deployment path.
``--dtype fp16`` exists only with ``--frozen``: the session runs in fp16 on an fp32 model.

``--input-grad`` measures the image gradient instead (``input_grad_table``): the stem data-gradient kernel
alone against MIOpen's, and the train step with and without ``image_grad``.

One deliberate difference: the reference prints ``np.mean(runtime)`` — the last trial only
(scripts/timing.py:48); this prints the mean (and median, min) over all timed trials.
"""
from __future__ import annotations

import argparse
import json
import statistics

import torch

from argus_amd.models import NCameraCNN, NCameraCNNConfig
from argus_amd.utils import time_torch_fn


def forward_latency(trials: int = 100, batch: int = 2, hw=(256, 256), dtype: str = "fp32", train_mode: bool = True,
                    graph: bool = True, device: str = "cuda", frozen: bool = False) -> dict:
    """Mean / median / min seconds of one NCameraCNN forward (no_grad) over ``trials`` timed trials.
    ``frozen``: the forward of an InferenceSession of the model in eval mode, in compute dtype ``dtype``
    ("fp16" is a session dtype only: the model behind it is fp32)."""
    if dtype == "fp16" and not frozen:
        raise ValueError("dtype 'fp16' is served by the frozen session only (frozen=True)")
    torch.manual_seed(0)
    cfg = NCameraCNNConfig(n_cams=2)
    model = NCameraCNN(cfg, compute_dtype="fp32" if dtype == "fp16" else dtype).to(device)
    model.train(train_mode)
    H, W = hw
    static_x = torch.rand((batch, cfg.n_cams * 3, H, W), device=device)
    first = None
    if frozen:
        from argus_amd.infer import InferenceSession

        session = InferenceSession(model.eval(), batch, (H, W), compute_dtype=dtype, graph=graph)
        train_mode = False

        def run(x):
            return session(x)
    elif graph:
        # untimed warm-up (workspaces, weight-prep table), then capture on a side stream
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(2):
                model(static_x)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(g):
            static_out = model(static_x)

        def run(x):
            static_x.copy_(x)
            g.replay()
            return static_out
    else:
        def run(x):
            with torch.no_grad():
                return model(x)

    times = []
    for i in range(trials + 1):
        x = torch.rand((batch, cfg.n_cams * 3, H, W), device=device)
        out, t = time_torch_fn(lambda: run(x))
        if i == 0:
            first = t
        else:
            times.append(t)
    assert torch.isfinite(out).all()
    r = {"mean_s": statistics.fmean(times), "median_s": statistics.median(times), "min_s": min(times),
         "first_call_s": first, "trials": trials, "batch": batch, "hw": list(hw), "dtype": dtype,
         "mode": "train" if train_mode else "eval", "graph": graph}
    if frozen:
        r["frozen"] = True
    return r


def pose_latency(trials: int = 200, batch: int = 1, hw=(256, 256), dtype: str = "bf16", graph: bool = True,
                 layout: str = "chw", frame_hw=None, fused_stem: bool = True, fused_head: bool = True,
                 parent: bool = False, device: str = "cuda", roi=None, track=None) -> dict:
    """Mean / median / min seconds of one ``pose()`` call, from uint8 frames on the device to the (batch, 7) pose
    tensor, over ``trials`` timed trials. ``parent``: the yardstick arm, ``InferenceSession.pose()`` on the same
    frames (an "hwc" layout or a crop is brought to the planar cropped tensor it needs with torch ops first, as
    argus/validate_real.py:58-75 does); else a ``PoseSession`` with the given switches. ``track``: a
    ``TrackConfig``: the session aims its own region from every pose (one more launch in the graph)."""
    from argus_amd.data import center_crop_slices
    from argus_amd.infer import InferenceSession
    from argus_amd.pose_session import PoseSession

    torch.manual_seed(0)
    cfg = NCameraCNNConfig(n_cams=2)
    model = NCameraCNN(cfg, compute_dtype="fp32" if dtype == "fp16" else dtype).to(device).eval()
    H, W = hw
    Hs, Ws = (H, W) if frame_hw is None else frame_hw
    shape = (batch, 3 * cfg.n_cams, Hs, Ws) if layout == "chw" else (batch, cfg.n_cams, Hs, Ws, 3)
    if parent:
        session = InferenceSession(model, batch, (H, W), compute_dtype=dtype, graph=graph)
        ys, xs = center_crop_slices((Hs, Ws), (H, W))

        def run(x):
            if layout == "hwc":
                x = x.permute(0, 1, 4, 2, 3).reshape(batch, 3 * cfg.n_cams, Hs, Ws)
            if (Hs, Ws) != (H, W):
                x = x[..., ys, xs]
            return session.pose(x)
    else:
        session = PoseSession(model, batch, (H, W), compute_dtype=dtype, graph=graph, frame_hw=(Hs, Ws), layout=layout,
                              fused_stem=fused_stem, fused_head=fused_head, roi=roi is not None, track=track)
        if roi is not None:
            session.set_roi(roi)  # once: the replays read it from the device
        run = session.pose
    times, first = [], None
    for i in range(trials + 1):
        x = torch.randint(0, 256, shape, dtype=torch.uint8, device=device)
        out, t = time_torch_fn(lambda: run(x))
        if i == 0:
            first = t
        else:
            times.append(t)
    assert torch.isfinite(out).all() and tuple(out.shape) == (batch, 7)
    return {"mean_s": statistics.fmean(times), "median_s": statistics.median(times), "min_s": min(times),
            "first_call_s": first, "trials": trials, "batch": batch, "hw": list(hw), "frame_hw": [Hs, Ws],
            "layout": layout, "dtype": dtype, "graph": graph, "pose": True,
            "arm": "InferenceSession" if parent else f"PoseSession(stem={int(fused_stem)},head={int(fused_head)})",
            "launches_per_forward": session.launches_per_forward, "roi": None if roi is None else list(roi), "track": track is not None}


def _event_ms(fn, reps: int) -> float:
    """Milliseconds per call of ``fn`` over ``reps`` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def input_grad_table(rounds: int = 3, samples: int = 20, device: str = "cuda") -> list:
    """The image-gradient measurement (``--input-grad``), as the lines of profiles/input_grad.txt.

    (a) argus_conv_stem_dgrad alone at N=128 and N=2, 256x256, bf16 and fp32: with the apply prologue (the
        call the fused schedule makes) and on a materialised dy, against ``torch.nn.grad.conv2d_input``
        (MIOpen) on the same materialised dy and weights, given as the NHWC memory the kernel reads
        (channels_last) and as NCHW. The yardstick does less: no apply, no planar fp32 output.
    (b) ``FusedTrainer.step`` at B=64, bf16, 256x256, with and without ``image_grad``.
    Device events, the arms interleaved, ``rounds`` rounds; every cell is the median over ``samples`` samples
    (kernel arms: 10 back-to-back calls a sample)."""
    import ctypes as C

    from argus_amd._lib import BF16, F32, BnBwdPrologue, ConvDesc, lib, ptr, stream
    from argus_amd.step import FusedTrainer

    L = lib()
    lines = ["# Image gradient (argus_conv_stem_dgrad), one MI355X, 256x256, python -m argus_amd.timing --input-grad",
             "# device events, arms interleaved, %d rounds, median / min over %d samples a cell; ms" % (rounds, samples),
             "# (a) kernel alone, 10 back-to-back calls a sample. apply = dy formed from dm, y, ca/cb/cc while staging",
             "#     (what the fused backward launches); plain = a materialised dy; miopen_* = torch.nn.grad.conv2d_input",
             "#     on that materialised dy (no apply; output in the compute dtype, not planar fp32), dy as the",
             "#     kernel's NHWC memory (channels_last) or NCHW-contiguous. N=2 operands stay cache-resident.",
             "# part dtype     N arm          round   median      min"]
    med = {}
    for dtype, tdt, dt in (("bf16", torch.bfloat16, BF16), ("fp32", torch.float32, F32)):
        for N in (128, 2):
            torch.manual_seed(0)
            d = ConvDesc(N, 256, 256, 3, 64, 7, 7, 2, 3, 128, 128, 1)
            w = torch.randn(64, 7, 7, 3, device=device) * 0.1
            wf = torch.empty(64, 256, dtype=tdt, device=device)
            L.conv_weight_prep(C.byref(d), dt, ptr(w), None, ptr(wf), None, stream())
            dm = torch.randn(N, 128, 128, 64, device=device).to(tdt)
            y = torch.randn(N, 128, 128, 64, device=device).to(tdt)
            ca, cb, cc = (torch.randn(64, device=device) * 0.5 for _ in range(3))
            dy = torch.empty_like(dm)
            L.bn_bwd_apply(dt, N * 128 * 128, 64, ptr(dm), 0, None, ptr(y), None, None, ptr(ca), ptr(cb), ptr(cc),
                           ptr(dy), None, None, None, None, None, None, stream())
            dx = torch.empty(N, 3, 256, 256, device=device)
            pro = BnBwdPrologue(ptr(y), ptr(ca), ptr(cb), ptr(cc), None)
            w_oihw = w.permute(0, 3, 1, 2).contiguous().to(tdt)
            dy_cl = dy.permute(0, 3, 1, 2)  # (N, 64, 128, 128) over the NHWC memory
            dy_nchw = dy_cl.contiguous()
            arms = {
                "apply": lambda: L.conv_stem_dgrad(C.byref(d), dt, ptr(dm), ptr(wf), C.byref(pro), ptr(dx), stream()),
                "plain": lambda: L.conv_stem_dgrad(C.byref(d), dt, ptr(dy), ptr(wf), None, ptr(dx), stream()),
                "miopen_nhwc": lambda: torch.nn.grad.conv2d_input((N, 3, 256, 256), w_oihw, dy_cl, stride=2, padding=3),
                "miopen_nchw": lambda: torch.nn.grad.conv2d_input((N, 3, 256, 256), w_oihw, dy_nchw, stride=2,
                                                                  padding=3),
            }
            for name in list(arms):  # warm-up (code objects, MIOpen's solver choice); an arm that fails is reported
                try:
                    _event_ms(arms[name], 3)
                except Exception as e:  # noqa: BLE001
                    lines.append(f"a    {dtype:5s} {N:5d} {name:12s} failed: {type(e).__name__}: {str(e)[:80]}")
                    del arms[name]
            for rnd in range(1, rounds + 1):
                for name, fn in arms.items():
                    ts = [_event_ms(fn, 10) for _ in range(samples)]
                    m = statistics.median(ts)
                    med.setdefault((dtype, N, name), []).append(m)
                    lines.append(f"a    {dtype:5s} {N:5d} {name:12s} {rnd:5d} {m:8.4f} {min(ts):8.4f}")
            del dm, y, dy, dx, dy_nchw
            torch.cuda.empty_cache()
    lines.append("# (b) FusedTrainer.step, B=64, bf16: one step a sample")
    trainers = {}
    x = torch.rand(64, 6, 256, 256, device=device)
    from oracle import se3

    T = se3.random_targets(64, generator=torch.Generator().manual_seed(0)).float().to(device)
    buf = torch.empty_like(x)
    for name in ("step", "step+image_grad"):
        torch.manual_seed(0)
        model = NCameraCNN(NCameraCNNConfig(n_cams=2), compute_dtype="bf16").to(device).train()
        trainers[name] = FusedTrainer(model, lr=1e-5, max_grad_norm=1.0)
    steps = {"step": lambda: trainers["step"].step(x, T),
             "step+image_grad": lambda: trainers["step+image_grad"].step(x, T, image_grad=buf)}
    for fn in steps.values():
        _event_ms(fn, 3)
    for rnd in range(1, rounds + 1):
        for name, fn in steps.items():
            ts = [_event_ms(fn, 1) for _ in range(samples)]
            m = statistics.median(ts)
            med.setdefault(("bf16", 64, name), []).append(m)
            lines.append(f"b    bf16  {64:5d} {name:15s} {rnd:2d} {m:8.4f} {min(ts):8.4f}")
    lines += ["", "# summary: median of the round medians"]
    mm = {k: statistics.median(v) for k, v in med.items()}
    for dtype in ("bf16", "fp32"):
        for N in (128, 2):
            ours = mm.get((dtype, N, "apply"))
            yard = [v for k, v in mm.items() if k[:2] == (dtype, N) and k[2].startswith("miopen")]
            if ours is None or not yard:
                continue
            best = min(yard)
            lines.append(f"{dtype} N={N:<3d} kernel+apply {ours:8.4f} | plain {mm[(dtype, N, 'plain')]:8.4f} | "
                         f"miopen best {best:8.4f} | ours/miopen {ours / best:5.2f}x "
                         f"({'faster' if ours < best else 'slower'} than the yardstick)")
    extra = mm[("bf16", 64, "step+image_grad")] - mm[("bf16", 64, "step")]
    lines.append(f"step B=64 bf16: {mm[('bf16', 64, 'step')]:8.4f} -> {mm[('bf16', 64, 'step+image_grad')]:8.4f} with "
                 f"image_grad: +{extra:.4f} ms; the kernel alone at N=128 bf16 (apply): {mm[('bf16', 128, 'apply')]:.4f} ms")
    return lines


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--input-grad", action="store_true",
                    help="measure the image-gradient kernel and the step with image_grad (writes --out)")
    ap.add_argument("--out", default="profiles/input_grad.txt", help="where --input-grad writes its table")
    ap.add_argument("--trials", type=int, default=100)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--hw", type=int, nargs=2, default=(256, 256))
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16x3", "bf16", "fp16"],
                    help="fp16: with --frozen only")
    ap.add_argument("--eval", action="store_true", help="eval-mode BN (running statistics)")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of a replayed hipGraph")
    ap.add_argument("--frozen", action="store_true",
                    help="time an InferenceSession of the eval-mode model (fp32 / bf16 / fp16)")
    ap.add_argument("--pose", action="store_true",
                    help="with --frozen: time PoseSession.pose() end to end (uint8 frames in, pose out)")
    ap.add_argument("--layout", default="chw", choices=["chw", "hwc"], help="--pose: the frames' layout")
    ap.add_argument("--frame-hw", type=int, nargs=2, default=None, help="--pose: frame size, center-cropped to --hw")
    ap.add_argument("--unfused-stem", action="store_true", help="--pose: the parent session's three stem launches")
    ap.add_argument("--unfused-head", action="store_true", help="--pose: the parent session's head launches")
    ap.add_argument("--parent", action="store_true", help="--pose: time InferenceSession.pose() instead (yardstick)")
    ap.add_argument("--roi", type=float, nargs=4, default=None, metavar=("Y", "X", "H", "W"),
                    help="--pose: PoseSession(roi=True) with this region of every frame (source pixels, fractional "
                         "allowed) resampled to --hw inside the stem launch")
    ap.add_argument("--track", default=None, metavar="CALIB.json",
                    help="--pose: PoseSession(track=load_calibration(CALIB.json)): every replay aims the next region "
                         "from its own pose")
    a = ap.parse_args(argv)
    if a.pose:
        if not a.frozen:
            ap.error("--pose times a frozen session: pass --frozen")
        track = None
        if a.track:
            if a.parent or a.unfused_head:
                ap.error("--track needs PoseSession's fused head: not with --parent or --unfused-head")
            from argus_amd.track import load_calibration

            try:
                track = load_calibration(a.track)
            except (OSError, ValueError) as e:
                ap.error(f"--track {a.track}: {e}")
        if a.roi and a.parent:
            ap.error("--roi is PoseSession's: InferenceSession (--parent) has no region of interest")
        r = pose_latency(a.trials, a.batch, tuple(a.hw), a.dtype, not a.no_graph, a.layout,
                         tuple(a.frame_hw) if a.frame_hw else None, not a.unfused_stem, not a.unfused_head, a.parent,
                         roi=a.roi, track=track)
        print(f"pose() took {r['mean_s']} seconds on average.")
        print(json.dumps(r))
        return
    if a.dtype == "fp16" and not a.frozen:
        ap.error("--dtype fp16 is served by --frozen only")
    if a.input_grad:
        lines = input_grad_table()
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    r = forward_latency(a.trials, a.batch, tuple(a.hw), a.dtype, not a.eval, not a.no_graph, frozen=a.frozen)
    print(f"Forward pass took {r['mean_s']} seconds on average.")
    print(json.dumps(r))


if __name__ == "__main__":
    main()
