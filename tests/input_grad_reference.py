"""The reduced-precision yardstick of the image-gradient tests (CPU only): how far the reference model's
x.grad moves under bf16 autocast, on the small batch the bf16 engine test uses."""
import torch

from oracle import se3
from oracle.ncamera import build_reference_model


def small_batch():
    g = torch.Generator().manual_seed(1234)
    x = torch.randint(0, 256, (2, 6, 64, 64), generator=g, dtype=torch.uint8).float() / 255.0
    return x, se3.random_targets(2, generator=g).float()


def reference_bf16_distance():
    """Global relative distance of the CPU reference's x.grad under bf16 autocast from its fp32 self, on
    the B=2 64x64 batch of test_image_grad_bf16."""
    x, T = small_batch()
    grads = []
    for low in (False, True):
        rm = build_reference_model(42).train()
        xr = x.clone().requires_grad_()
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=low):
            pred = rm(xr)
        se3.geometric_loss(pred.float(), T).mean().backward()
        grads.append(xr.grad)
    return ((grads[1].double() - grads[0].double()).norm() / grads[0].double().norm()).item()
