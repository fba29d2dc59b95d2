"""Time of the two-view clip front end (avt_clip_transform, datasets/dataloader.py:155-181) at b = 8 clips of
t = 16 decoded 360x640 RGB frames, image_size 224: the five launches alone on frames already packed in HBM
(HIP events, after a warm-up), the whole ClipTransform call from host arrays (descriptor build + host-to-device
copy of the frames + the launches), and the same work done with Pillow on the host, frame by frame, one thread.
Prints one JSON line.

    python tools/clip_bench.py [b] [t]
"""
import ctypes
import json
import os
import random
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import avtubes  # noqa: E402,F401
import clip_oracle as co  # noqa: E402  (the Pillow pipeline)
from avt_amd import frames as fr  # noqa: E402
from avt_amd._lib import call, query  # noqa: E402
from avt_amd.frames import ClipTransform  # noqa: E402
from avt_amd.trunk import P, stream_ptr  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16
H, W, S = 360, 640, 224
dev = torch.device("cuda")
rng = np.random.default_rng(7)
clips = [[rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(T)] for _ in range(B)]
tf = ClipTransform(S, "train")
rnd = random.Random(8)
params = [tf.params(W, H, rnd) for _ in range(B)]

# the kernels alone: tables and frames on the device, buffers allocated once
n = B * T
desc = np.array([(i * H * W * 3, H, W, p.rh, p.rw, p.crop_top, p.crop_left, int(p.flip))
                 for i, p in enumerate(p for p in params for _ in range(T))], dtype=np.int64)
view2 = np.zeros(B, dtype=fr._VIEW2)
for v, p in zip(view2, params):
    v["crop_top"], v["crop_left"], v["flip"], v["nops"] = p.crop2_top, p.crop2_left, int(p.flip2), len(p.ops)
    for o, (kind, f) in enumerate(p.ops):
        v["ops"][o]["kind"], v["ops"][o]["factor"] = kind, f
src = torch.from_numpy(np.stack([f for c in clips for f in c]).reshape(-1)).to(dev)
d_desc, d_view2 = torch.from_numpy(desc).to(dev), torch.from_numpy(view2.view(np.uint8)).to(dev)
ws_bytes = int(query("avt_clip_workspace_bytes", B, T, S, H, 1))
ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
frames, augmented = (torch.empty(B, 3, T, S, S, device=dev) for _ in range(2))
mean, std = (ctypes.c_float * 3)(*fr.MEAN), (ctypes.c_float * 3)(*fr.STD)


def kernels():
    call("avt_clip_transform", P(src), P(d_desc), P(d_view2), B, T, S, H, P(ws), ws_bytes,
         ctypes.cast(mean, ctypes.c_void_p), ctypes.cast(std, ctypes.c_void_p), P(frames), P(augmented), stream_ptr())


def timed(fn, reps=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


ms_k = timed(kernels)
ms_call = timed(lambda: tf(clips, params=params), reps=5, warmup=2)
got = tf(clips, params=params)
assert torch.equal(got[0], frames) and torch.equal(got[1], augmented)
t0 = time.perf_counter()
ref_f, ref_a = co.pil_clips(clips, params, S)
ms_pil = (time.perf_counter() - t0) * 1e3
assert np.array_equal(ref_f, frames.cpu().numpy()) and np.array_equal(ref_a, augmented.cpu().numpy())
print(json.dumps({"kernel": "avt_clip_transform", "clips": B, "frames_per_clip": T, "src": f"{H}x{W}", "image_size": S,
                  "launches": 5, "kernels_ms": round(ms_k, 4), "kernels_clips_per_s": round(B / ms_k * 1e3, 1),
                  "call_ms": round(ms_call, 3), "call_clips_per_s": round(B / ms_call * 1e3, 1),
                  "pillow_host_ms": round(ms_pil, 1), "pillow_clips_per_s": round(B / ms_pil * 1e3, 2),
                  "bitwise_equal_to_pillow": True}))
