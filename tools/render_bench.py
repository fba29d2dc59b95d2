"""render.overlay and evaluate.heatmaps beside the same expressions composed from torch ops, same GPU, same run,
alternating.  Writes bench_out/render_timing.txt."""
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import avtubes  # noqa: E402,F401
from avt_amd import evaluate as ev  # noqa: E402
from avt_amd import render  # noqa: E402

dev = torch.device("cuda")
torch.manual_seed(0)
N, H, W = 128, 224, 224
frames = torch.randn(N, 3, H, W, device=dev)
pred = (torch.rand(N, H, W, device=dev) < 0.5).float()
gt = (torch.rand(N, H, W, device=dev) < 0.3).float()
jet = render.JET.to(dev)
A = torch.randn(N, 1, 14, 14, device=dev)


def torch_overlay():
    f = frames.flatten(1)
    mn, mx = f.min(1).values.view(N, 1, 1, 1), f.max(1).values.view(N, 1, 1, 1)
    a = ((frames - mn) / (mx - mn) * 255).permute(0, 2, 3, 1) * 0.4
    c0 = jet[(gt * 128).to(torch.uint8).long()].double()
    c1 = jet[(pred * 255).to(torch.uint8).long()].double()
    return (a.double() + (c0 * 0.5 + c1 * 0.5) * 0.6).clamp(0, 255).to(torch.uint8)


def torch_heatmaps():
    r = F.interpolate(A, size=(224, 224), mode="bilinear", align_corners=False)[:, 0]
    f = r.flatten(1)
    mn, mx = f.min(1).values.view(N, 1, 1), f.max(1).values.view(N, 1, 1)
    return (r - mn) / (mx - mn)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


cases = [("render.overlay (avt_render_overlay)", lambda: render.overlay(frames, pred=pred, gt=gt)),
         ("torch ops, same expression", torch_overlay),
         ("evaluate.heatmaps mode=norm (avt_heatmap_upsample)", lambda: ev.heatmaps(A, mode="norm")),
         ("F.interpolate + min/max normalise", torch_heatmaps)]
same = torch.equal(render.overlay(frames, pred=pred, gt=gt), torch_overlay())
hd = (ev.heatmaps(A, mode="norm") - torch_heatmaps()).abs().max().item()
for _, fn in cases:
    for _ in range(5):
        fn()
torch.cuda.synchronize()
rounds = {name: [] for name, _ in cases}
for _ in range(5):  # alternate
    for name, fn in cases:
        rounds[name].append(timed(fn, 50))
lines = [f"{torch.cuda.get_device_name(0)}; {N} frames of {H}x{W}; {N} maps 14x14 -> 224x224; 5 rounds x 50 calls, "
         f"alternating, device events; us per call: median (min .. max)",
         f"overlay bytes equal to the torch composition: {same}; heatmaps max |diff| to F.interpolate form: {hd:.3e}"]
for name, _ in cases:
    v = sorted(rounds[name])
    lines.append(f"{name:55s} {v[2]:9.1f} ({v[0]:.1f} .. {v[-1]:.1f})")
ov_bytes = N * H * W * (12 * 2 + 3 + 8)  # frame read twice, 3 B out, two 4 B maps
lines.append(f"overlay traffic model {ov_bytes / 1e6:.1f} MB per call (frame read twice, second from L2 at best)")
os.makedirs(os.path.join(REPO, "bench_out"), exist_ok=True)
with open(os.path.join(REPO, "bench_out", "render_timing.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
