"""Eval forward of one seeded model, folded (enable_folded_inference) against unfolded, in one process.

    timeout -k 10 600 python tools/infer_bench.py [--model avenet|tube|r3d] [--batches 128,1] [--pairs 3]
                                                  [--iters N] [--warmup W]

--model avenet (default): AVENet at B 224^2 frames + 257 x 300 spectrograms.  --model tube: FullModel (R3D-18 video
trunk + audio ResNet-18 + head) at b clips of 16 x 224^2 frames + b 257 x 300 spectrograms (one per clip); --model
r3d: the standalone R3D-18 trunk (no max-pool) on the same clips (default --batches 8,1 for both).

Per batch size: both paths warmed up, then `--pairs` alternating (unfolded, folded) pairs; each timed region is
`--iters` forwards between two HIP events on the current stream (the engine's side stream joins it at the end of
every forward).  Prints ms per forward of every region, the launch counts of one forward of each path (libavt
calls by entry point, counted at the Python binding, plus the torch element-wise launches of the unfolded path's
per-call BN arithmetic, which the count lists as `torch BN arithmetic`), and the largest difference of the
outputs; for tube / r3d also the peak allocated memory of one forward of each path.  Reads nothing outside the
repository: seeded weights, seeded inputs, running statistics moved by two train-mode forwards."""
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
from avt_amd import _lib, trunk, tube  # noqa: E402
from avt_amd.model import AVENet, HardWayArgs  # noqa: E402


def build(folded, sd, dev, kind="avenet"):
    if kind == "avenet":
        m = AVENet(HardWayArgs(), False)
    elif kind == "tube":
        from avt_amd.model import FullModel

        m = FullModel(orc.Args())
    else:
        from avt_amd.resnet3D import generate_model

        m = generate_model(18, no_max_pool=True, n_classes=1039)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    return m.enable_folded_inference() if folded else m


def make_inputs(kind, B, dev, seed=None):
    """The inputs of one forward: (image, spectrogram) / (spectrogram per clip, video) / (video,)."""
    if kind == "avenet":
        if seed is None:
            return orc.make_image(B, 224).to(dev), orc.make_spectrogram(B, 257, 300).to(dev)
        return orc.make_image(B, 224, seed=seed).to(dev), orc.make_spectrogram(B, 257, 300, seed=seed + 10).to(dev)
    import tube_oracle as tor

    video = tor.make_video(B, 16, 224) if seed is None else tor.make_video(B, 16, 224, seed=seed)
    if kind == "r3d":
        return (video.to(dev),)
    spec = orc.make_spectrogram(B, 257, 300) if seed is None else orc.make_spectrogram(B, 257, 300, seed=seed + 10)
    return spec.to(dev), video.to(dev)


def seed_state(kind):
    if kind == "avenet":
        return orc.make_state(0)
    import tube_oracle as tor

    sd = tor.make_tube_state(0)
    if kind == "r3d":
        sd = {k[len("vidnet."):]: v for k, v in sd.items() if k.startswith("vidnet.")}
    return sd


def count_launches(model, *inputs):
    """libavt calls of one forward by entry point (+ the eval branch of trunk._bn_finalize: 5 torch launches each)."""
    counts = collections.Counter()
    real_call, real_fin = _lib.call, trunk._bn_finalize

    def call(name, *a):
        counts[name] += 1
        return real_call(name, *a)

    def fin(*a, **k):
        counts["torch BN arithmetic (5 launches each)"] += 1
        return real_fin(*a, **k)

    mods = [sys.modules[n] for n in ("avt_amd.trunk", "avt_amd.engine", "avt_amd.tube")]
    for mod in mods:
        mod.call = call
    trunk._bn_finalize = tube._bn_finalize = fin
    try:
        with torch.no_grad():
            model(*inputs)
        torch.cuda.synchronize()
    finally:
        for mod in mods:
            mod.call = real_call
        trunk._bn_finalize = tube._bn_finalize = real_fin
    return counts


def timed(model, inputs, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        a.record()
        for _ in range(iters):
            model(*inputs)
        b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def peak_mib(model, inputs):
    """torch.cuda.max_memory_allocated over one forward, less what was allocated before it (weights, inputs)."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        model(*inputs)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20, (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="avenet", choices=["avenet", "tube", "r3d"])
    ap.add_argument("--batches", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=0, help="forwards per timed region (0: by model and batch size)")
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "infer_bench needs a GPU"
    dev = torch.device("cuda:0")
    kind = args.model
    batches = args.batches or ("128,1" if kind == "avenet" else "8,1")
    sd = seed_state(kind)
    seed_model = build(False, sd, dev, kind).train()
    with torch.no_grad():  # move the running statistics off (0, 1)
        for s in (1, 2):
            seed_model(*make_inputs(kind, 8 if kind == "avenet" else 1, dev, seed=s))
    sd = {k: v.detach().cpu().clone() for k, v in seed_model.state_dict().items()}
    del seed_model
    models = {"unfolded": build(False, sd, dev, kind), "folded": build(True, sd, dev, kind)}
    print(f"device: {torch.cuda.get_device_name(0)}")
    what = "logits" if kind == "r3d" else "A"
    unit = "B" if kind == "avenet" else "b (clips of 16 frames)"
    for B in (int(b) for b in batches.split(",")):
        inputs = make_inputs(kind, B, dev)
        if kind == "avenet":
            iters = args.iters or (20 if B >= 32 else 100)
        else:
            iters = args.iters or (10 if B >= 4 else 50)
        outs = {}
        for name, m in models.items():
            with torch.no_grad():
                for _ in range(args.warmup):
                    outs[name] = m(*inputs)
            torch.cuda.synchronize()
        first = {n: (o if torch.is_tensor(o) else o[0]) for n, o in outs.items()}
        dA = (first["folded"] - first["unfolded"]).abs().max().item()
        print(f"\n{unit} = {B}: {iters} forwards per region, {args.pairs} alternating pairs; "
              f"max |{what} folded - {what} unfolded| = {dA:.3e}")
        ms = {"unfolded": [], "folded": []}
        for p in range(args.pairs):
            for name in ("unfolded", "folded"):
                ms[name].append(timed(models[name], inputs, iters))
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
            c = count_launches(m, *inputs)
            print(f"  launches per forward, {name}: {sum(c.values())} calls: " +
                  ", ".join(f"{k} x{v}" for k, v in sorted(c.items())))
        if kind != "avenet":
            del outs, first
            for name, m in models.items():
                tot, fwd = peak_mib(m, inputs)
                print(f"  peak allocated, {name}: {tot:.0f} MiB in all, {fwd:.0f} MiB above what was allocated "
                      f"before the forward (torch.cuda.max_memory_allocated)")


if __name__ == "__main__":
    main()
