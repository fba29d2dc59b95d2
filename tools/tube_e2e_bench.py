"""Cost of training the video trunk end to end (FullModel.enable_video_backward): the captured tube step
at bench.py's tube size (b clips of 16 x 224 x 224 frames, one 257 x 300 spectrogram per clip), once detached (the
default, bench.py --workload tube) and once with the opt-in, in the same process on the same GPU, the two timed in
alternating blocks of graph replays; then one eager one-stream step of the opt-in model under the conv profiler for the
per-kind conv TFLOP/s, and the algorithmic expectation of the ratio from the profiler's own FLOP counts.
usage: python tools/tube_e2e_bench.py [--batch 8] [--frames 16] [--rounds 5] [--steps 10] [--out profiles/tube_e2e_step.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5, help="alternations detached / opt-in")
    ap.add_argument("--steps", type=int, default=10, help="graph replays per timed block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import bench
    import avtubes  # noqa: F401
    from avt_amd.model import FullModel, HardWayArgs
    from avt_amd.train import HardWayTrainStep
    from avt_amd.trunk import ConvProfiler

    dev = torch.device("cuda", 0)
    video, spec = bench.synthetic_inputs(args.batch, dev, seed=1000, frames=args.frames)
    steps = {}
    for name in ("detached", "opt-in"):
        torch.manual_seed(0)
        model = FullModel(HardWayArgs()).to(dev).train()
        if name == "opt-in":
            model.enable_video_backward()
        step = HardWayTrainStep(model, lr=1e-6, weight_decay=1e-4)
        for i in range(max(args.warmup, 1)):
            step.step(spec, video)
            if i == 0:
                step.capture(spec, video)
        torch.cuda.synchronize()
        steps[name] = step

    def block(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = step.step(spec, video)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps, float(loss)

    ms = {"detached": [], "opt-in": []}
    losses = {}
    for _ in range(args.rounds):  # A B A B ...: drift and clock state hit both alike
        for name in ("detached", "opt-in"):
            t, losses[name] = block(steps[name])
            ms[name].append(t)
    med = {k: statistics.median(v) for k, v in ms.items()}
    # conv family of one eager, one-stream step of each model (per-kernel durations, not overlapped pairs)
    conv = {}
    for name in ("detached", "opt-in"):
        eager = bench.eager_copy(steps[name])
        conc = eager.engine.concurrent
        eager.engine.concurrent = False
        with ConvProfiler() as prof:
            eager.step(spec, video)
            torch.cuda.synchronize()
        eager.engine.concurrent = conc
        conv[name] = prof.summary()
    fl = {k: sum(v[1] for v in c.values()) for k, c in conv.items()}
    vid_bwd = sum(v[1] for k, v in conv["opt-in"].items() if k in ("dgrad3d", "wgrad3d"))
    lines = [
        f"tube step, b={args.batch} clips of {args.frames}x224x224 frames + one 257x300 spectrogram per clip, captured "
        f"(hip-graph replay), {args.rounds} alternating blocks of {args.steps} replays each, {torch.cuda.get_device_name(0)}",
        f"detached (default): {med['detached']:.3f} ms/step (blocks: {' '.join(f'{x:.3f}' for x in ms['detached'])}) "
        f"loss {losses['detached']:.4f}",
        f"opt-in (enable_video_backward): {med['opt-in']:.3f} ms/step (blocks: "
        f"{' '.join(f'{x:.3f}' for x in ms['opt-in'])}) loss {losses['opt-in']:.4f}",
        f"measured ratio opt-in / detached: {med['opt-in'] / med['detached']:.3f}",
        f"algorithmic conv FLOPs per step: detached {fl['detached'] / 1e12:.3f} TFLOP, opt-in {fl['opt-in'] / 1e12:.3f} "
        f"TFLOP (the video trunk's dgrad3d + wgrad3d: {vid_bwd / 1e12:.3f} TFLOP; the stem's folded 2-D wgrad and the "
        f"1x1x1 downsamples' in-place 2-D dgrad are not bracketed)",
        f"algorithmic expectation of the ratio (conv FLOPs opt-in / detached): {fl['opt-in'] / fl['detached']:.3f}",
        "conv kinds of one eager one-stream opt-in step (launches, algorithmic TFLOP, ms, TFLOP/s):",
    ]
    for kind, (n, f, t, _) in sorted(conv["opt-in"].items()):
        lines.append(f"  {kind}: {n} launches, {f / 1e12:.3f} TFLOP, {t:.3f} ms, {f / 1e9 / max(t, 1e-9):.1f} TFLOP/s")
    report = "\n".join(lines)
    print(report, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
