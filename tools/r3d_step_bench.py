"""Fine-tuning step of the stand-alone R3D-18, three forms on the same seeded clips and labels:

  parent    loss = F.cross_entropy(net(video), labels); loss.backward(); torch.optim.SGD.step()  (the autograd bridge:
            libavt trunk, torch head, torch's foreach optimizer over the parameter views)
  fused     train.R3DTrainStep.step, eager (libavt head and flat SGD, one flat gradient, no autograd)
  captured  the same step replayed from its HIP graph

The three are built from the same weights in ONE process and timed in alternating blocks (A B C A B C ...: drift and
clock state hit all alike); every block ends in a device synchronise and the median block is reported with all blocks
listed.  One batch size per process: without --batch the tool starts one fresh child per size of --sizes, each under
its own ``timeout``, stops at the first child that fails, and writes the children's reports to --out.
usage: python tools/r3d_step_bench.py [--sizes 8,1] [--frames 16] [--size 224] [--classes 400] [--max-pool]
                                      [--rounds 5] [--steps 10] [--warmup 3] [--out profiles/r3d_step.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_size(args):
    import torch
    import torch.nn.functional as F

    import avtubes  # noqa: F401
    from avt_amd.resnet3D import generate_model
    from avt_amd.train import R3DTrainStep

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1000)
    video = torch.randn(args.batch, 3, args.frames, args.size, args.size, generator=g).to(dev)
    labels = torch.randint(0, args.classes, (args.batch,), generator=g).to(dev)
    hyper = dict(lr=1e-3, momentum=0.9, weight_decay=1e-3)

    def net():
        torch.manual_seed(0)
        return generate_model(18, n_classes=args.classes, no_max_pool=not args.max_pool).to(dev).train()

    parent_net = net().enable_backward()
    parent_opt = torch.optim.SGD(parent_net.parameters(), **hyper)

    def parent_step():
        parent_opt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(parent_net(video), labels)
        loss.backward()
        parent_opt.step()
        return loss

    fused = R3DTrainStep(net(), "sgd", **hyper)
    captured = R3DTrainStep(net(), "sgd", **hyper)
    forms = {"parent": parent_step, "fused": lambda: fused.step(video, labels),
             "captured": lambda: captured.step(video, labels)}
    first = {}
    for i in range(max(args.warmup, 1)):  # every form warms up at the timed shape; the capture follows the first step
        for name, fn in forms.items():
            loss = fn()
            if i == 0:
                first[name] = float(loss)
        if i == 0:
            captured.capture(video, labels)
    torch.cuda.synchronize()

    def block(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps, float(loss)

    ms = {k: [] for k in forms}
    last = {}
    for _ in range(args.rounds):
        for name, fn in forms.items():
            t, last[name] = block(fn)
            ms[name].append(t)
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines = [f"R3D-18 fine-tuning step, b={args.batch} clips of {args.frames}x{args.size}x{args.size}, "
             f"{args.classes} classes, stem max-pool {'on' if args.max_pool else 'off'}, SGD momentum 0.9; "
             f"{args.rounds} alternating blocks of {args.steps} steps after {max(args.warmup, 1)} warm-up steps each, "
             f"{torch.cuda.get_device_name(0)}"]
    for name in forms:
        lines.append(f"  {name:9s} {med[name]:9.3f} ms/step  (blocks: {' '.join(f'{x:.3f}' for x in ms[name])})  "
                     f"first loss {first[name]:.6f}  last loss {last[name]:.6f}")
    lines.append(f"  ratio parent / fused {med['parent'] / med['fused']:.3f}, parent / captured "
                 f"{med['parent'] / med['captured']:.3f}, fused / captured {med['fused'] / med['captured']:.3f}")
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=None, help="time this one size in this process")
    ap.add_argument("--sizes", default="8,1", help="batch sizes, one child process each")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--classes", type=int, default=400)
    ap.add_argument("--max-pool", action="store_true", help="keep the stem's MaxPool3d (no_max_pool=False)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=280, help="seconds per size")
    ap.add_argument("--out", default=None, help="write the reports to this file")
    args = ap.parse_args()
    if args.batch is not None:
        return one_size(args)
    reports = []
    for b in [int(x) for x in args.sizes.split(",") if x]:
        cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--batch",
               str(b), "--frames", str(args.frames), "--size", str(args.size), "--classes", str(args.classes),
               "--rounds", str(args.rounds), "--steps", str(args.steps), "--warmup", str(args.warmup)]
        if args.max_pool:
            cmd.append("--max-pool")
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:  # nothing more is started on the GPU after a failure
            print(f"r3d_step_bench: size {b} ended with status {r.returncode}; stopping", flush=True)
            sys.exit(r.returncode)
        reports.append("\n".join(ln for ln in r.stdout.splitlines() if ln.startswith(("R3D-18", "  "))))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(reports) + "\n")


if __name__ == "__main__":
    main()
