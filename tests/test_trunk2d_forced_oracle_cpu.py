"""avenet_oracle.resnet18_forward_forced -- the "teacher-forced" fp64 reference of the 2-D ResNet-18 trunk's backward
that test_trunk2d_backward_forced_gpu.py holds Trunk.backward against -- checked on the CPU, with a tape simulated by
the fp64 oracle at that test's shapes (make_image(3, 64), make_spectrogram(2, 65, 76); batch not raised): forcing is
sound (it reproduces plain autograd), its bf16-storage yardstick stays under that test's cap, and it tells each of
five mis-wired backward graphs from the right one.

Measured on the simulated tapes: the yardstick's e_ref is 0 (layer4.1.bn2.bias) to 1.15e-2, median 5.8e-3, for
vision and 0 to 1.51e-2, median 5.9e-3, for audio -- no tensor above the cap at N = 3 / N = 2, so every bound is the
5e-2 floor.  The faults' smallest error over their upstream gradients: drop_identity 11.9, drop_downsample 9.2, mask_c2
7.6, unmasked_class00 3.9 and pool_last 1.8 times the bound.

The stem kernel rounds relu(bn1(c0)) to bf16 BEFORE its max-pool picks a window's first maximum; the oracle picks
among the fp64 values.  test_stem_rounding_before_the_pool_stays_inside measures what that alone costs a correct
trunk against this oracle."""
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import avenet_oracle as orc
from gradcheck import rule_full

E_REF_CAP, MAX_OVER_CAP = 0.1, 6  # test_trunk2d_backward_forced_gpu.py's condition on the yardstick (the R3D test's)
MODALS = ("vision", "audio")
_CACHE = {}


def _bf16(t):
    return t.to(torch.bfloat16).double()


def _inputs(modal):
    """The GPU test's input and upstream gradient."""
    if modal == "audio":
        return orc.make_spectrogram(2, 65, 76), orc.make_gout(2, 5, 5)
    return orc.make_image(3, 64), orc.make_gout(3, 4, 4)


def _recorded_forward(s, prefix, x, modal, round_h0=False):
    """resnet18_forward with every tensor the trunk stores -- conv outputs, the pooled stem output, the blocks' ReLU
    outputs -- rounded to bf16 where it is made (straight-through for the gradient) and recorded, in call order, under
    the tape's names.  The stem's full-resolution ReLU output is stored nowhere: it stays fp64 (round_h0: rounded too,
    before the max-pool picks, as the stem kernel does: test_stem_rounding_before_the_pool_stays_inside)."""
    convs, relus, pools = [], [], []
    conv2d, relu, max_pool2d = F.conv2d, F.relu, F.max_pool2d

    def stored(fn, seq, skip_first=False):
        def f(*a, **k):
            y = fn(*a, **k)
            if skip_first and not seq:
                seq.append(None)
                return y
            y = y + (_bf16(y) - y).detach()
            seq.append(y.detach().clone())
            return y
        return f

    with mock.patch.object(orc.F, "conv2d", stored(conv2d, convs)), \
            mock.patch.object(orc.F, "relu", stored(relu, relus, skip_first=not round_h0)), \
            mock.patch.object(orc.F, "max_pool2d", stored(max_pool2d, pools)):
        feat = orc.resnet18_forward(s, prefix, x, modal, training=True)
    ci, ri = iter(convs), iter(relus)
    next(ri)  # the stem's full-resolution ReLU output
    (p0,) = pools
    tape = {"c0": next(ci), "p0": p0, "blocks": []}
    for li in range(1, 5):
        for bi in range(2):
            tb = {"c1": next(ci), "h1": next(ri), "c2": next(ci)}
            if li > 1 and bi == 0:
                tb["cd"] = next(ci)
            tb["out"] = next(ri)
            tape["blocks"].append(tb)
    assert next(ci, None) is None and next(ri, None) is None
    return feat, tape


def _plain(sd, prefix, x, modal, g_out, round_h0=False):
    """(tape, {name: gradient}) of plain fp64 autograd through the recorded forward on the bf16-rounded conv weights
    and input."""
    names = [n for n, _, kind in orc.resnet18_entries(prefix) if kind in ("conv", "bn_w", "bn_b")]
    s = {k: (v.double().clone() if v.is_floating_point() else v.clone()) for k, v in sd.items()
         if k.startswith(prefix)}
    for n in names:
        s[n] = (_bf16(s[n]) if s[n].dim() == 4 else s[n]).requires_grad_(True)
    xin = _bf16(x).requires_grad_(True)
    feat, tape = _recorded_forward(s, prefix, xin, modal, round_h0)
    (feat * g_out.double()).sum().backward()
    plain = {n[len(prefix):]: s[n].grad for n in names if s[n].grad is not None}
    plain["input"] = xin.grad
    return tape, plain


def _simulated(modal):
    """A tape as the GPU test reads it off Trunk.forward, from resnet18_forward in fp64 on the bf16-rounded conv
    weights and input with every stored tensor rounded to bf16 where it is made (the later layers read the rounded
    values, as on the GPU; the rounding passes the gradient straight through), plain fp64 autograd's gradients of that
    network and loss, and the forced oracle's on the tape with and without bf16-stored gradients.  Once per modal."""
    if modal not in _CACHE:
        sd = orc.make_state(0)
        prefix = "audnet." if modal == "audio" else "imgnet."
        x, g_out = _inputs(modal)
        tape, plain = _plain(sd, prefix, x, modal, g_out)
        assert all(torch.equal(t, _bf16(t)) for t in (tape["p0"], tape["blocks"][7]["c2"]))  # bf16 values
        assert sorted(tape) == ["blocks", "c0", "p0"] and len(tape["blocks"]) == 8
        assert [("cd" in tb) for tb in tape["blocks"]] == [False, False, True, False, True, False, True, False]
        assert tuple(tape["blocks"][7]["out"].shape) == tuple(g_out.shape)
        forced = orc.resnet18_forced_grads(sd, x, modal, tape, g_out)
        yard = orc.resnet18_forced_grads(sd, x, modal, tape, g_out, round_grads=True)
        _CACHE[modal] = dict(sd=sd, x=x, g_out=g_out, tape=tape, plain=plain, forced=forced, yard=yard)
    return _CACHE[modal]


@pytest.mark.parametrize("modal", MODALS)
def test_forcing_is_sound(modal):
    """The forced oracle on the simulated tape against plain fp64 autograd of the same rounded-weights network, every
    one of the 60 parameter gradients and the input gradient inside the rule (the yardstick's error taken against the
    forced gradients, as the GPU test takes it).  On a tape the network itself made, forcing adds zeros: the two agree
    to fp64 rounding."""
    d = _simulated(modal)
    assert len(d["plain"]) == 61 and sorted(d["plain"]) == sorted(d["forced"])
    bad, worst = [], 0.0
    for n, ref in d["plain"].items():
        # the yardstick's deviation from the forced gradients, carried over to the plain ones
        b, e, _, _ = rule_full(d["forced"][n], ref, ref + (d["yard"][n] - d["forced"][n]))
        worst = max(worst, e)
        bad += [(n,) + x for x in b]
    print(f"{modal}: forced vs plain fp64 autograd, largest error vector {worst:.3e}")
    assert not bad, bad
    assert worst < 1e-9, worst


@pytest.mark.parametrize("modal", MODALS)
def test_forced_yardstick_within_cap(modal):
    """The bf16-hook yardstick's own error vector against the forced fp64 gradients: at most MAX_OVER_CAP of the 61
    tensors above E_REF_CAP."""
    d = _simulated(modal)
    e_ref = {n: rule_full(d["yard"][n], ref, d["yard"][n])[2] for n, ref in d["forced"].items()}
    v = np.array(list(e_ref.values()))
    over = [(n, round(e, 4)) for n, e in e_ref.items() if e > E_REF_CAP]
    print(f"{modal}: forced yardstick e_ref max {v.max():.3e} median {np.median(v):.3e} min {v.min():.3e}; "
          f"above {E_REF_CAP}: {over}")
    assert len(over) <= MAX_OVER_CAP, over


@pytest.mark.parametrize("modal", MODALS)
def test_stem_rounding_before_the_pool_stays_inside(modal):
    """A network that rounds the stem's ReLU output to bf16 before the max-pool picks (as the stem kernel does: two
    of a window's values that round to one bf16 number tie, and the first takes the gradient), plain fp64 autograd
    through it held against the forced oracle on its tape as the GPU test holds the trunk: the different routing
    reaches the stem weight, bn1.weight and the input gradient only, and stays inside the rule.  Measured: error
    vector 3.2e-2 (vision conv1.weight), 2.0e-2 (audio conv1_a.weight), 3.3e-2 / 3.7e-2 (input), bn1.weight < 1e-3;
    the pool_last fault is 1.8 times the bound."""
    d = _simulated(modal)
    prefix = "audnet." if modal == "audio" else "imgnet."
    tape, plain = _plain(d["sd"], prefix, d["x"], modal, d["g_out"], round_h0=True)
    forced = orc.resnet18_forced_grads(d["sd"], d["x"], modal, tape, d["g_out"])
    yard = orc.resnet18_forced_grads(d["sd"], d["x"], modal, tape, d["g_out"], round_grads=True)
    stem = ["conv1_a.weight" if modal == "audio" else "conv1.weight", "bn1.weight", "input"]
    bad = []
    for n, ref in forced.items():
        b, e, e_ref, ratio = rule_full(plain[n], ref, yard[n])
        if n in stem:
            print(f"{modal} {n}: e {e:.3e} e_ref {e_ref:.3e} ({ratio:.2f} of its bound)")
        else:
            assert e < 1e-9, (n, e)
        bad += [(n,) + x for x in b]
    assert not bad, bad


def _upstream(fault, modal):
    """Gradients the fault changes (all of them lie upstream of it; "input" is upstream of everything)."""
    stem = ["conv1_a.weight" if modal == "audio" else "conv1.weight", "bn1.weight", "bn1.bias"]
    names = [n for n in _simulated(modal)["forced"] if n not in stem and n != "input"]

    def layers(*ps):
        return [n for n in names if n.startswith(ps)]

    if fault == "drop_identity":  # the gradient of layer1.1's input = layer1.0's output
        return ["input"] + stem + layers("layer1.0.")
    if fault == "drop_downsample":  # the branch's own parameters (no gradient at all) and all below layer2.0's input
        return ["input"] + stem + layers("layer1.", "layer2.0.downsample.")
    if fault == "pool_last":
        # the stem's weight and the input only: bn1.bias' gradient, a sum over positions, is exactly the same
        # whichever of a window's equal maxima receives the gradient, and bn1.weight's nearly so (equal values of
        # relu(bn(c0)) in one channel have equal normalised values)
        return ["input"] + stem[:1]
    if fault == "unmasked_class00":  # layer1.1's g' = g * mask feeds its bn2, its identity branch and all below it
        return ["input"] + stem + layers("layer1.")
    return ["input"] + stem + names  # mask_c2: every block's output mask, layer4.1's included


@pytest.mark.parametrize("modal", MODALS)
@pytest.mark.parametrize("fault", orc.FORCED_FAULTS_2D)
def test_forced_oracle_sees_miswiring(fault, modal):
    """A forced oracle with one wiring fault, held against the right one as a GPU result would be: every gradient
    upstream of the fault is out of bound (so the GPU test cannot pass with that fault in Trunk.backward)."""
    d = _simulated(modal)
    wrong = orc.resnet18_forced_grads(d["sd"], d["x"], modal, d["tape"], d["g_out"], fault=fault)
    up = _upstream(fault, modal)
    assert up and all(n in d["forced"] for n in up)
    inside, least = [], None
    for n in up:
        b, e, e_ref, ratio = rule_full(wrong[n], d["forced"][n], d["yard"][n])
        if not b:
            inside.append((n, round(e, 4), round(e_ref, 4)))
        if least is None or ratio < least[1]:
            least = (n, ratio)
    print(f"{modal} {fault}: {len(up)} upstream gradients, {len(up) - len(inside)} out of bound; smallest error "
          f"{least[1]:.2f} of its bound ({least[0]})")
    assert not inside, inside
