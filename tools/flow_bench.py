#!/usr/bin/env python
"""Times the flow entries (avt_amd.flow, losses.FlowLoss) at the reference's sizes against the same expressions from
torch ops on the same GPU.  Device events around `iters` back-to-back calls after `warmup` calls; the median of
`repeats` such windows, the two sides alternating.

    python tools/flow_bench.py [--out profiles/flow_bench.txt]

Sizes (flow.py: batch 20, 16 frames -> 15 pairs per clip): 20 x 15 pairs of 224 x 224 maps for the warp and the
consistency, 20 x 15 pairs of 14 x 14 heat maps for the loss (forward and gradient), 300 fields of 224 x 224 for the
colour picture.
"""
import argparse
import math
import os
import sys

import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import avtubes  # noqa: E402,F401
from avt_amd import flow  # noqa: E402
from avt_amd.losses import FlowLoss  # noqa: E402

DEV = torch.device("cuda")


def timed(fn, warmup, iters, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / iters)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def grid_of(field):
    """pixel displacements [N,H,W,2] -> grid_sample coordinates (align_corners=False)"""
    N, H, W, _ = field.shape
    y, x = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float32),
                          torch.arange(W, device=DEV, dtype=torch.float32), indexing="ij")
    return torch.stack([(x + field[..., 0] + 0.5) * 2 / W - 1, (y + field[..., 1] + 0.5) * 2 / H - 1], dim=-1)


def torch_consistency(pred, grid):
    """grid_sample + the compare + the three masked sums of cal_CIOU, per pair"""
    T = pred.shape[0]
    warped = TF.grid_sample(pred[:-1, None].float(), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    infer = (warped[:, 0] >= 0.5).double()
    gt = pred[1:].double()
    inter = (infer * gt).sum(dim=(1, 2))
    denom = gt.sum(dim=(1, 2)) + (infer * (gt == 0)).sum(dim=(1, 2))
    return torch.stack([inter / denom, inter, denom], dim=1)


def make_wheel():
    return flow.WHEEL.to(DEV).double()


def torch_flow2img(field, wheel):
    """utils.flow2img / compute_color transcribed to torch ops, fp64, batched over fields (per-field maximum)"""
    f = field.double()
    u, v = f[..., 0].clone(), f[..., 1].clone()
    unknown = (u.abs() > 1e7) | (v.abs() > 1e7)
    u[unknown] = 0
    v[unknown] = 0
    rad = torch.sqrt(u ** 2 + v ** 2)
    maxrad = rad.amax(dim=(1, 2), keepdim=True).clamp_min(-1)
    eps = 2.0 ** -52
    u = u / maxrad + eps
    v = v / maxrad + eps
    nan = torch.isnan(u) | torch.isnan(v)
    u[nan] = 0
    v[nan] = 0
    ncols = wheel.shape[0]
    rad = torch.sqrt(u ** 2 + v ** 2)
    a = torch.atan2(-v, -u) / math.pi
    fk = (a + 1) / 2 * (ncols - 1) + 1
    k0 = torch.floor(fk).long()
    k1 = k0 + 1
    k1[k1 == ncols + 1] = 1
    fr = (fk - k0)[..., None]
    col = (1 - fr) * (wheel[k0 - 1] / 255) + fr * (wheel[k1 - 1] / 255)
    small = (rad <= 1)[..., None]
    col = torch.where(small, 1 - rad[..., None] * (1 - col), col * 0.75)
    img = torch.floor(255 * col * (~nan)[..., None]).to(torch.uint8)
    img[unknown] = 0
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flow_bench needs the GPU")
    g = torch.Generator(device="cpu").manual_seed(0)
    clips, pairs, S, hm = 20, 15, 224, 14
    N = clips * pairs
    # one prediction sequence per clip, as evaluate_tube sees it, and all of them stacked for the batched calls
    pred = (torch.rand(N + 1, S, S, generator=g) < 0.5).to(torch.uint8).to(DEV)
    field = (torch.randn(N, S, S, 2, generator=g) * 3).to(DEV)
    grid = grid_of(field)
    x = torch.randn(clips, pairs + 1, hm, hm, generator=g).to(DEV)
    lfield = (torch.randn(clips, pairs, hm, hm, 2, generator=g)).to(DEV)
    lgrid = grid_of(lfield.reshape(N, hm, hm, 2))
    wheel = make_wheel()
    crit = FlowLoss()

    def ours_loss():
        xx = x.clone().requires_grad_(True)
        crit(xx, lfield).backward()

    def torch_loss():
        xx = x.clone().requires_grad_(True)
        warped = TF.grid_sample(xx[:, :-1].reshape(N, 1, hm, hm), lgrid, mode="bilinear", padding_mode="zeros",
                                align_corners=False)
        (warped.reshape(clips, pairs, hm, hm) - xx[:, 1:]).abs().mean().backward()

    rows = [
        ("warp 300 x 224^2 (fp32 maps)", lambda: flow.warp(pred[:N].float(), field, "pixels"),
         lambda: TF.grid_sample(pred[:N, None].float(), grid, mode="bilinear", padding_mode="zeros",
                                align_corners=False)),
        ("consistency 300 pairs x 224^2", lambda: flow.consistency(pred, field, "pixels"),
         lambda: torch_consistency(pred, grid)),
        ("consistency 15 pairs x 224^2 (one video)", lambda: flow.consistency(pred[:16], field[:15], "pixels"),
         lambda: torch_consistency(pred[:16], grid[:15])),
        ("loss + gradient 20 x 15 pairs x 14^2", ours_loss, torch_loss),
        ("colour 300 x 224^2", lambda: flow.flow_to_image(field), lambda: torch_flow2img(field, wheel)),
        ("colour 1 x 224^2", lambda: flow.flow_to_image(field[:1]), lambda: torch_flow2img(field[:1], wheel)),
    ]
    lines = [f"# tools/flow_bench.py on {torch.cuda.get_device_name(0)}: device events, warmup {args.warmup}, "
             f"{args.iters} calls per window, median (min .. max) of {args.repeats} windows, us per call",
             "# the torch side holds its inputs ready (grid_sample coordinates precomputed); the warp row's .float() "
             "of the maps is in both sides"]
    for name, ours, theirs in rows:
        a = timed(ours, args.warmup, args.iters, args.repeats)
        b = timed(theirs, args.warmup, args.iters, args.repeats)
        a2 = timed(ours, 2, args.iters, args.repeats)
        lines.append(f"{name:44s} libavt {a[0]:9.1f} ({a[1]:.1f} .. {a[2]:.1f})   torch {b[0]:9.1f} ({b[1]:.1f} .. "
                     f"{b[2]:.1f})   libavt again {a2[0]:9.1f}   torch / libavt {b[0] / a[0]:6.2f}")
        print(lines[-1], flush=True)
    # the two sides compute the same thing (the colour bytes may differ by 1 where 255 col is an integer up to rounding)
    ours_c, theirs_c = flow.consistency(pred[:16], field[:15], "pixels"), torch_consistency(pred[:16], grid[:15])
    lines.append(f"# check: consistency max |libavt - torch| = {(ours_c - theirs_c).abs().max().item():.3e}; colour "
                 f"bytes differing = {(flow.flow_to_image(field[:2]) != torch_flow2img(field[:2], wheel)).sum().item()}"
                 f" of {2 * S * S * 3}")
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
