"""dev: is the bf16x3 mode's distance from the oracle at a trained point the split arithmetic itself?

    python tools/x3_trained_point.py

25 fused steps (B=64, 256 x 256, compute_dtype="bf16x3") from the seeded init, then the eval-mode prediction
on 16 held-out samples by the bf16x3 kernels, by the exact fp32 kernels with the same weights and by the CPU
emulation of the split (tests/x3_reference.py), each against the CPU oracle in fp32 and fp64."""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from argus_amd.models import NCameraCNN  # noqa: E402
from argus_amd.step import FusedTrainer  # noqa: E402
from oracle import se3  # noqa: E402
from oracle.ncamera import build_reference_model  # noqa: E402
from x3_reference import use_x3_convs  # noqa: E402

torch.set_num_threads(16)
dev = torch.device("cuda", 0)
B = 64
g = torch.Generator().manual_seed(0)
x = (torch.randint(0, 256, (B, 6, 256, 256), generator=g, dtype=torch.uint8).float() / 255.0).to(dev)
T = se3.random_targets(B, generator=g).to(dev)
vx = torch.randint(0, 256, (16, 6, 256, 256), generator=g, dtype=torch.uint8).float() / 255.0
torch.manual_seed(42)
m = NCameraCNN(compute_dtype="bf16x3").to(dev).train()
tr = FusedTrainer(m, lr=1e-4, max_grad_norm=1.0)
for _ in range(25):
    tr.step(x, T)
torch.cuda.synchronize()
m.eval()
with torch.no_grad():
    ours = m(vx.to(dev)).cpu()
sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
e = NCameraCNN(compute_dtype="fp32")
e.load_state_dict(sd)
e = e.to(dev).eval()
with torch.no_grad():
    exact = e(vx.to(dev)).cpu()
outs = {}
for name, emu, dt in (("fp32", False, torch.float32), ("emulation", True, torch.float32), ("fp64", False, torch.float64)):
    r = build_reference_model(42)
    r.load_state_dict(sd)
    r = r.to(dt).eval()
    if emu:
        use_x3_convs(r)
    with torch.no_grad():
        outs[name] = r(vx.to(dt)).double()
    print(name, "done", flush=True)
for ref in ("fp32", "fp64"):
    print(f"vs oracle {ref}: bf16x3 GPU {(ours.double() - outs[ref]).abs().max():.3e}  exact GPU "
          f"{(exact.double() - outs[ref]).abs().max():.3e}  CPU emulation {(outs['emulation'] - outs[ref]).abs().max():.3e}"
          f"  oracle fp32 {(outs['fp32'] - outs[ref]).abs().max():.3e}")
print(f"bf16x3 GPU vs CPU emulation {(ours.double() - outs['emulation']).abs().max():.3e}; |pred| max {outs['fp64'].abs().max():.3f}")
