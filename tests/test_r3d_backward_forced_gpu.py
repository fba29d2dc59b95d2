"""R3DTrunk.backward as a whole against fp64 autograd on the GPU's OWN forward state (the "teacher-forced" oracle
tube_oracle.r3d18_forward_forced).  For a fixed forward state the backward is a linear map of the upstream gradient,
so forcing the oracle's conv outputs, ReLU masks and outputs to the tape's takes the forward's rounding noise (flipped
ReLU masks, shifted batch statistics, amplified by 17 layers: test_r3d_backward_end_to_end's 0.2-0.45 yardstick) out
of the comparison and leaves what only the composition can get wrong: the residual gradient through ``add=gm``, gm
shared by bn2 / downsample.1 / the identity branch, the in-place 2-D dgrad of the 1x1x1 downsample on top of conv1's
dgrad, downsample.1's mask-less BN backward, the max-pool backward reading h0, the stem's unfold, and which tape
tensor feeds which wgrad.  tests/test_r3d_forced_oracle_cpu.py shows on the CPU that the oracle is sound, that its
yardstick meets the cap below and that four such wiring faults fall out of bound."""
import numpy as np
import pytest
import torch

import tube_oracle as tor
from gradcheck import rule_full

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
E_REF_CAP, MAX_OVER_CAP = 0.1, 6


def _engine(max_pool):
    """A standalone trainable generate_model(18, ...) on the seeded weights (as test_r3d_backward_gpu._standalone) and
    an R3DEngine with the backward on its flat store."""
    from avt_amd.resnet3D import generate_model
    from avt_amd.tube import R3DEngine

    sd = tor.make_tube_state(0)
    net = generate_model(18, no_max_pool=not max_pool, n_classes=1039)
    net.load_state_dict({k[len("vidnet."):]: v for k, v in sd.items() if k.startswith("vidnet.")})
    net.enable_backward()
    net = net.to(DEV).train()
    return net, R3DEngine(net._flat_store(), "", max_pool=max_pool, with_backward=True), sd


def _ncdhw(t, b):
    """'(b t) h w c' bf16 on the GPU -> [b, c, t, h, w] on the CPU."""
    n, h, w, c = t.shape
    return t.view(b, n // b, h, w, c).permute(0, 4, 1, 2, 3).float().cpu()


@pytest.mark.parametrize("max_pool", [False, True])
def test_r3d_backward_forced_tape(max_pool):
    """engine.forward(make_video(2, 4, 64), tape=True), then engine.backward(tape, glogits) for a fixed dense standard
    normal glogits [2, 1039] (loss = (logits * glogits).sum(); no cross-entropy), against the forced oracle fed the
    tape (c0, h0, per block c1, h1, c2, cd, out).  Without the max-pool layer4's frames are 4 x 4; with it T goes
    4 -> 2, layer4's frames are 2 x 2 and layer4.0.conv1 is a stride-2 conv into frames of fewer than 32 positions.

    Yardstick: the same forced oracle with every activation gradient the GPU stores in bf16 rounded to bf16 (autograd
    hooks on c0, h0, the max-pool output, c1, h1, c2, cd and each block's output, which covers gm; weight gradients
    stay full sums).  Every one of the 62 parameter gradients, on the whole tensor, by gradcheck's rule: error vector
    <= max(5e-2, 3 e_ref), cosine >= min(0.999, 1 - 3 (1 - cos_ref)), norm deviation <= max(5e-2, 3 d_ref, e_ref).
    Condition: the yardstick's own e_ref is at most 0.1 for all but at most 6 tensors (printed; still checked).

    Measured on one MI355X: the forced yardstick's e_ref is 0 (fc) to 9.1e-3, median 5.7e-3, without the max-pool and
    0 to 9.6e-3, median 5.7e-3, with it -- no tensor above the cap, so every bound is the 5e-2 floor; this build's
    largest error is 0.19 of its bound without the max-pool (layer1.1.bn1.bias) and 0.23 with it (bn1.bias, e 1.15e-2
    against e_ref 9.6e-3; conv1.weight e 9.1e-3 against e_ref 8.5e-3).  The extended kernel cases of
    test_r3d_backward_gpu.py measured at worst 4.9e-3 (dgrad, bound 8e-3) and 2.2e-7 (wgrad, bound 2e-4)."""
    video = tor.make_video(2, 4, 64)
    b = video.shape[0]
    glogits = tor.make_glogits(b)
    net, engine, sd = _engine(max_pool)
    flat = engine.flat
    logits, tp = engine.forward(video.to(DEV), True, tape=True)
    gflat = torch.zeros(flat.n_train, device=DEV, dtype=torch.float32)
    engine.backward(tp, glogits.float().to(DEV), gflat)
    torch.cuda.synchronize()
    grads = {n: g.detach().double().cpu() for n, g in flat.param_grad_views(gflat).items()}
    tape = {"c0": _ncdhw(tp["c0"], b), "h0": _ncdhw(tp["h0"], b), "blocks": []}
    for tb in tp["blocks"]:
        tape["blocks"].append({k: _ncdhw(tb[k], b) for k in ("c1", "h1", "c2", "cd", "out") if k in tb})
    assert len(tape["blocks"]) == 8 and tape["blocks"][7]["out"].shape[-2:] == ((2, 2) if max_pool else (4, 4))
    ref = tor.r3d18_forced_grads(sd, video, tape, glogits, max_pool)
    yard = tor.r3d18_forced_grads(sd, video, tape, glogits, max_pool, round_grads=True)
    assert len(ref) == 62 and sorted(ref) == sorted(grads)
    bad, over, e_refs, worst = [], [], [], (None, 0.0)
    for n, r in ref.items():
        assert tuple(grads[n].shape) == tuple(r.shape), n
        viol, e, e_ref, ratio = rule_full(grads[n], r, yard[n])
        print(f"  {n}: e {e:.3e} e_ref {e_ref:.3e} ({ratio:.2f} of its bound)")
        e_refs.append(e_ref)
        if e_ref > E_REF_CAP:
            over.append((n, round(e_ref, 4)))
        if ratio > worst[1]:
            worst = (n, ratio)
        bad += [(n,) + v for v in viol]
    e_refs = np.array(e_refs)
    print(f"max_pool={max_pool}: forced yardstick e_ref max {e_refs.max():.3e} median {np.median(e_refs):.3e}; above "
          f"{E_REF_CAP}: {over}; largest error {worst[1]:.2f} of its bound ({worst[0]})")
    for x in bad:
        print("OUT OF BOUND", x)
    assert len(over) <= MAX_OVER_CAP, over
    assert not bad, bad
