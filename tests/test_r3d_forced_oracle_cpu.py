"""tube_oracle.r3d18_forward_forced -- the "teacher-forced" fp64 reference of the R3D-18 trunk's backward that
test_r3d_backward_forced_gpu.py holds R3DTrunk.backward against -- checked on the CPU, with a tape simulated by the fp64
oracle: forcing is sound (it reproduces plain autograd), its bf16-storage yardstick stays under that test's cap, and it
tells each of four mis-wired backward graphs from the right one."""
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tube_oracle as tor
from gradcheck import rule_full

E_REF_CAP, MAX_OVER_CAP = 0.1, 6  # test_r3d_backward_forced_gpu.py's condition on the yardstick
_CACHE = {}


def _bf16(t):
    return t.to(torch.bfloat16).double()


def _recorded_forward(s, video, max_pool):
    """r3d18_forward with every conv and ReLU output rounded to bf16 where it is made (straight-through for the
    gradient) and recorded, in call order, under the tape's names."""
    convs, relus = [], []
    conv3d, relu = F.conv3d, F.relu

    def stored(fn, seq):
        def f(*a, **k):
            y = fn(*a, **k)
            y = y + (_bf16(y) - y).detach()
            seq.append(y.detach().clone())
            return y
        return f

    with mock.patch.object(tor.F, "conv3d", stored(conv3d, convs)), \
            mock.patch.object(tor.F, "relu", stored(relu, relus)):
        feat = tor.r3d18_forward(s, "vidnet.", video, training=True, max_pool=max_pool)
    ci, ri = iter(convs), iter(relus)
    tape = {"c0": next(ci), "h0": next(ri), "blocks": []}
    for li in range(1, 5):
        for bi in range(2):
            tb = {"c1": next(ci), "h1": next(ri), "c2": next(ci)}
            if li > 1 and bi == 0:
                tb["cd"] = next(ci)
            tb["out"] = next(ri)
            tape["blocks"].append(tb)
    assert next(ci, None) is None and next(ri, None) is None
    return feat, tape


def _simulated(max_pool):
    """A tape as R3DTrunk.forward(tape=True) names it, from r3d18_forward in fp64 on the bf16-rounded conv weights and
    video with every stored tensor rounded to bf16 where it is made (the later layers read the rounded values, as on
    the GPU; the rounding passes the gradient straight through), plain fp64 autograd's gradients of that network and
    loss, and the forced oracle's on the tape with and without bf16-stored gradients.  Once per configuration."""
    if max_pool not in _CACHE:
        sd = tor.make_tube_state(0)
        video = tor.make_video(2, 4, 64)
        glogits = tor.make_glogits(2)
        names = [k for k, v in sd.items() if k.startswith("vidnet.") and v.is_floating_point()
                 and not k.endswith(("running_mean", "running_var"))]
        s = {k: (v.double().clone() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
        for n in names:
            s[n] = (_bf16(s[n]) if s[n].dim() == 5 else s[n]).requires_grad_(True)
        feat, tape = _recorded_forward(s, _bf16(video), max_pool)
        logits = F.linear(feat.mean(dim=(2, 3, 4)), s["vidnet.fc.weight"], s["vidnet.fc.bias"])
        (logits * glogits).sum().backward()
        plain = {n[len("vidnet."):]: s[n].grad for n in names}
        assert all(torch.equal(t, _bf16(t)) for t in (tape["h0"], tape["blocks"][7]["c2"]))  # bf16 values
        assert sorted(tape) == ["blocks", "c0", "h0"] and len(tape["blocks"]) == 8
        assert all(sorted(rb) in (["c1", "c2", "cd", "h1", "out"], ["c1", "c2", "h1", "out"]) for rb in tape["blocks"])
        forced = tor.r3d18_forced_grads(sd, video, tape, glogits, max_pool)
        yard = tor.r3d18_forced_grads(sd, video, tape, glogits, max_pool, round_grads=True)
        _CACHE[max_pool] = dict(sd=sd, video=video, glogits=glogits, tape=tape, plain=plain, forced=forced, yard=yard)
    return _CACHE[max_pool]


@pytest.mark.parametrize("max_pool", [False, True])
def test_forcing_is_sound(max_pool):
    """The forced oracle on the simulated tape against plain fp64 autograd of the same rounded-weights network, every
    one of the 62 gradients inside the rule (the yardstick's error taken against the forced gradients, as the GPU test
    takes it).  On a tape the network itself made, forcing adds zeros: the two agree to fp64 rounding."""
    d = _simulated(max_pool)
    assert len(d["plain"]) == 62
    bad, worst = [], 0.0
    for n, ref in d["plain"].items():
        # the yardstick's deviation from the forced gradients, carried over to the plain ones
        b, e, _, _ = rule_full(d["forced"][n], ref, ref + (d["yard"][n] - d["forced"][n]))
        worst = max(worst, e)
        bad += [(n,) + x for x in b]
    print(f"max_pool={max_pool}: forced vs plain fp64 autograd, largest error vector {worst:.3e}")
    assert not bad, bad


@pytest.mark.parametrize("max_pool", [False, True])
def test_forced_yardstick_within_cap(max_pool):
    """The bf16-hook yardstick's own error vector against the forced fp64 gradients: at most MAX_OVER_CAP of the 62
    tensors above E_REF_CAP."""
    d = _simulated(max_pool)
    e_ref = {n: rule_full(d["yard"][n], ref, d["yard"][n])[2] for n, ref in d["forced"].items()}
    v = np.array(list(e_ref.values()))
    over = [(n, round(e, 4)) for n, e in e_ref.items() if e > E_REF_CAP]
    print(f"max_pool={max_pool}: forced yardstick e_ref max {v.max():.3e} median {np.median(v):.3e} min {v.min():.3e}; "
          f"above {E_REF_CAP}: {over}")
    assert len(over) <= MAX_OVER_CAP, over


def _upstream(fault):
    """Parameters whose gradient the fault changes (all of them lie upstream of it).  pool_last: the stem's weight
    only -- bn1.bias' gradient, a sum over positions, is exactly the same whichever of a window's equal maxima
    receives the gradient, and bn1.weight's nearly so (equal stored h0 values have equal normalised values up to the
    bf16 rounding of c0; measured 4e-4)."""
    names = [n[len("vidnet."):] for n, _, kind in tor.r3d18_entries("vidnet.") if kind in ("conv", "bn_w", "bn_b")]
    stem = ["conv1.weight", "bn1.weight", "bn1.bias"]
    if fault == "drop_identity":
        return stem + [n for n in names if n.startswith("layer1.0.")]
    if fault == "drop_downsample":
        return stem + [n for n in names if n.startswith("layer1.")]
    if fault == "pool_last":
        return stem[:1]
    return names  # mask_c2: every block's output mask


@pytest.mark.parametrize("fault", tor.FORCED_FAULTS)
def test_forced_oracle_sees_miswiring(fault):
    """A forced oracle with one wiring fault, held against the right one as a GPU result would be: every parameter
    upstream of the fault is out of bound (so the GPU test cannot pass with that fault in R3DTrunk.backward).  On the
    max-pool configuration, which has all four places."""
    d = _simulated(True)
    wrong = tor.r3d18_forced_grads(d["sd"], d["video"], d["tape"], d["glogits"], True, fault=fault)
    up = _upstream(fault)
    assert up and all(n in d["forced"] for n in up)
    inside, least = [], None
    for n in up:
        b, e, e_ref, ratio = rule_full(wrong[n], d["forced"][n], d["yard"][n])
        if not b:
            inside.append((n, round(e, 4), round(e_ref, 4)))
        if least is None or ratio < least[1]:
            least = (n, ratio)
    print(f"{fault}: {len(up)} upstream gradients, {len(up) - len(inside)} out of bound; smallest error "
          f"{least[1]:.2f} of its bound ({least[0]})")
    assert not inside, inside
