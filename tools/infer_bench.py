"""Eval forward of one seeded AVENet, folded (enable_folded_inference) against unfolded, in one process.

    timeout -k 10 600 python tools/infer_bench.py [--batches 128,1] [--pairs 3] [--iters N] [--warmup W]

Per batch size: both paths warmed up, then `--pairs` alternating (unfolded, folded) pairs; each timed region is
`--iters` forwards between two HIP events on the current stream (the engine's side stream joins it at the end of
every forward).  Prints ms per forward of every region, the launch counts of one forward of each path (libavt
calls by entry point, counted at the Python binding, plus the torch element-wise launches of the unfolded path's
per-call BN arithmetic, which the count lists as `torch BN arithmetic`), and the largest difference of the
outputs.  Reads nothing outside the repository: seeded weights, seeded inputs, running statistics moved by two
train-mode forwards."""
import argparse
import collections
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))

import torch  # noqa: E402

import avtubes  # noqa: E402,F401
import avenet_oracle as orc  # noqa: E402
from avt_amd import _lib, trunk  # noqa: E402
from avt_amd.model import AVENet, HardWayArgs  # noqa: E402


def build(folded, sd, dev):
    m = AVENet(HardWayArgs(), False)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    return m.enable_folded_inference() if folded else m


def count_launches(model, img, aud):
    """libavt calls of one forward by entry point (+ the eval branch of trunk._bn_finalize: 5 torch launches each)."""
    counts = collections.Counter()
    real_call, real_fin = _lib.call, trunk._bn_finalize

    def call(name, *a):
        counts[name] += 1
        return real_call(name, *a)

    def fin(*a, **k):
        counts["torch BN arithmetic (5 launches each)"] += 1
        return real_fin(*a, **k)

    mods = [sys.modules[n] for n in ("avt_amd.trunk", "avt_amd.engine")]
    for mod in mods:
        mod.call = call
    trunk._bn_finalize = fin
    try:
        with torch.no_grad():
            model(img, aud)
        torch.cuda.synchronize()
    finally:
        for mod in mods:
            mod.call = real_call
        trunk._bn_finalize = real_fin
    return counts


def timed(model, img, aud, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        a.record()
        for _ in range(iters):
            model(img, aud)
        b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,1")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=0, help="forwards per timed region (0: 20 at B >= 32, else 100)")
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "infer_bench needs a GPU"
    dev = torch.device("cuda:0")
    sd = orc.make_state(0)
    seed_model = build(False, sd, dev).train()
    with torch.no_grad():  # move the running statistics off (0, 1)
        for s in (1, 2):
            seed_model(orc.make_image(8, 224, seed=s).to(dev), orc.make_spectrogram(8, 257, 300, seed=s + 10).to(dev))
    sd = {k: v.detach().cpu().clone() for k, v in seed_model.state_dict().items()}
    del seed_model
    models = {"unfolded": build(False, sd, dev), "folded": build(True, sd, dev)}
    print(f"device: {torch.cuda.get_device_name(0)}")
    for B in (int(b) for b in args.batches.split(",")):
        img, aud = orc.make_image(B, 224).to(dev), orc.make_spectrogram(B, 257, 300).to(dev)
        iters = args.iters or (20 if B >= 32 else 100)
        outs = {}
        for name, m in models.items():
            with torch.no_grad():
                for _ in range(args.warmup):
                    outs[name] = m(img, aud)
            torch.cuda.synchronize()
        dA = (outs["folded"][0] - outs["unfolded"][0]).abs().max().item()
        print(f"\nB = {B}: {iters} forwards per region, {args.pairs} alternating pairs; max |A folded - A unfolded| = {dA:.3e}")
        ms = {"unfolded": [], "folded": []}
        for p in range(args.pairs):
            for name in ("unfolded", "folded"):
                ms[name].append(timed(models[name], img, aud, iters))
            print(f"  pair {p}: unfolded {ms['unfolded'][-1]:.3f} ms  folded {ms['folded'][-1]:.3f} ms  "
                  f"ratio {ms['unfolded'][-1] / ms['folded'][-1]:.3f}")
        for name in ms:
            print(f"  {name}: min {min(ms[name]):.3f} max {max(ms[name]):.3f} ms "
                  f"(spread {100 * (max(ms[name]) - min(ms[name])) / min(ms[name]):.1f} %)")
        faster = all(f < u for f, u in zip(ms["folded"], ms["unfolded"]))
        gap = min(ms["unfolded"]) - max(ms["folded"])
        spread = max(max(v) - min(v) for v in ms.values())
        print(f"  folded faster in every pair: {faster}; slowest folded vs fastest unfolded: {gap:+.3f} ms "
              f"(largest same-path spread {spread:.3f} ms)")
        for name, m in models.items():
            c = count_launches(m, img, aud)
            print(f"  launches per forward, {name}: {sum(c.values())} calls: " +
                  ", ".join(f"{k} x{v}" for k, v in sorted(c.items())))


if __name__ == "__main__":
    main()
