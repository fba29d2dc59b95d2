"""tests/tube_e2e_oracle.py -- the fp64 restatement of the tube step with the video features attached, and the
comparators test_tube_e2e_gpu.py applies -- checked on the CPU at that test's base geometry (b = 2, t = 3, 64 x 64
frames: a 4 x 4 layer4 map, so the head has 6 rows of 16 positions; 65 x 76 spectrograms, one per clip):

  * with ``.detach()`` put back the restatement is tube_oracle.tube_train_step, exactly (loss, A, logits, every audnet
    gradient: torch.equal in fp64), and no gradient reaches vidnet;
  * attached, its vidnet and audnet gradients equal plain fp64 autograd through tube_oracle.fullmodel_forward with the
    hook's detach taken out;
  * on a tape simulated by the fp64 forward (every stored tensor rounded to bf16 where it is made) the forced variant
    reproduces plain autograd, its bf16-storage yardstick meets the forced tests' cap, and detached it gives the
    detached step's audnet gradients and zeros for vidnet;
  * three wiring faults are flagged by the comparators the GPU test uses: gv not scaled by the normalisation and the
    vidnet gradient taken for one clip only (grad_violations: every vidnet tensor out of bound), fc included in Adam
    (adam_scope_violations: weight decay alone moves it)."""
from collections import OrderedDict
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import avenet_oracle as orc
import tube_e2e_oracle as e2e
import tube_oracle as tor
from gradcheck import rule_full
from test_r3d_forced_oracle_cpu import _recorded_forward as _recorded_r3d
from test_trunk2d_forced_oracle_cpu import _bf16, _recorded_forward as _recorded_2d

B_CLIPS, T, SIZE, FREQ, FRAMES = 2, 3, 64, 65, 76
_CACHE = {}


def _inputs():
    return orc.make_spectrogram(B_CLIPS, FREQ, FRAMES), tor.make_video(B_CLIPS, T, SIZE)


def _sd64():
    return OrderedDict((k, v.double() if v.is_floating_point() else v.clone()) for k, v in tor.make_tube_state(0).items())


def test_names():
    """60 vidnet tensors (20 convs, 20 BNs' weight and bias; fc left out) and the audio trunk's 60."""
    assert len(e2e.vid_names()) == 60 and len(e2e.e2e_names()) == 120
    assert not any(".fc." in n for n in e2e.e2e_names())
    un = e2e.untrained_names(tor.make_tube_state(0))
    assert sorted(un) == sorted(["vidnet.fc.weight", "vidnet.fc.bias", "audnet.fc.weight", "audnet.fc.bias",
                                 "audnet.conv1.weight", "audnet.conv1_flow.weight"]), un


def _plain():
    """Once: the detached and the attached step of the helper, tube_train_step, and plain autograd through
    fullmodel_forward with the hook's detach taken out."""
    if "plain" not in _CACHE:
        spec, video = _inputs()
        spec, video = spec.double(), video.double()
        det = e2e.tube_e2e_step(_sd64(), spec, video, detach=True, names=e2e.e2e_names())
        ref = tor.tube_train_step(_sd64(), spec, video, None)
        att = e2e.tube_e2e_step(_sd64(), spec, video)
        sd = _sd64()
        leaves = {n: sd[n].clone().requires_grad_(True) for n in e2e.e2e_names()}
        work = OrderedDict(sd)
        work.update(leaves)
        with mock.patch.object(torch.Tensor, "detach", lambda self: self):  # the hook's output.detach(), taken out
            A, logits = tor.fullmodel_forward(work, tor.repeat_spectrogram(spec, T), video, training=True)
        loss = orc.hardway_ce(logits)
        gl = torch.autograd.grad(loss, list(leaves.values()))
        _CACHE["plain"] = dict(det=det, ref=ref, att=att, auto=(loss.detach(), dict(zip(leaves, gl))))
    return _CACHE["plain"]


def test_detached_is_tube_train_step():
    d = _plain()
    (loss, A, logits, g), (rloss, rA, rlogits, rg) = d["det"], d["ref"]
    assert torch.equal(loss, rloss) and torch.equal(A, rA) and torch.equal(logits, rlogits)
    assert sorted(rg) == sorted(tor.trainable_names_tube())
    for n in rg:
        assert torch.equal(g[n], rg[n]), n
    assert all(g[n] is None for n in e2e.vid_names())  # detached: nothing reaches vidnet


def test_attached_is_autograd_without_the_detach():
    d = _plain()
    (loss, A, logits, g), (aloss, ag) = d["att"], d["auto"]
    assert torch.equal(loss, d["det"][0]) and torch.equal(logits, d["det"][2])  # the forward does not change
    assert torch.equal(loss, aloss)
    for n in e2e.e2e_names():
        assert g[n] is not None and torch.equal(g[n], ag[n]), n
    for n in e2e.vid_names():
        assert g[n].abs().max() > 0, n
    for n in tor.trainable_names_tube():  # the audnet gradients are those of the detached step
        assert torch.equal(g[n], d["det"][3][n]), n


def _simulated(t=T, per_clip=True):
    """Once per case: the step simulated in fp64 on the bf16-rounded conv weights and inputs with every stored tensor
    rounded where it is made (per-clip audio: the unit vectors repeated t times; folded: the repeated spectrograms
    through the trunk), the tapes that forward left, plain autograd's gradients, and the forced oracle and its
    yardstick on the tapes."""
    key = ("sim", t, per_clip)
    if key not in _CACHE:
        sd = tor.make_tube_state(0)
        spec, video = orc.make_spectrogram(B_CLIPS, FREQ, FRAMES), tor.make_video(B_CLIPS, t, SIZE)
        if not per_clip:
            spec = tor.repeat_spectrogram(spec, t)
        s = {k: (v.double().clone() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
        for n in e2e.e2e_names():
            s[n] = (_bf16(s[n]) if s[n].dim() >= 4 else s[n]).requires_grad_(True)
        feat_a, tape_a = _recorded_2d(s, "audnet.", _bf16(spec), "audio")
        amax = feat_a.detach().flatten(2).argmax(-1)
        an = F.normalize(F.adaptive_max_pool2d(feat_a, 1).flatten(1), dim=1)
        if per_clip:
            an = an.repeat_interleave(t, 0)
        feat_v, tape_v = _recorded_r3d(s, _bf16(video), False)
        assert tuple(feat_v.shape) == (B_CLIPS, 512, t, 4, 4)
        A, logits = orc.hardway_attention(an, F.normalize(feat_v, dim=1))
        orc.hardway_ce(logits).backward()
        plain = {n: s[n].grad for n in e2e.e2e_names()}
        assert all(v is not None for v in plain.values())
        tape = {"vid": tape_v, "aud": tape_a, "amax": amax}
        forced = e2e.tube_e2e_forced_grads(sd, spec, video, tape)
        yard = e2e.tube_e2e_forced_grads(sd, spec, video, tape, round_grads=True)
        _CACHE[key] = dict(sd=sd, spec=spec, video=video, tape=tape, plain=plain, forced=forced, yard=yard)
    return _CACHE[key]


@pytest.mark.parametrize("t,per_clip", [(1, False), (3, True)], ids=["t1-folded", "t3-perclip"])
def test_forcing_is_sound_and_yardstick_within_cap(t, per_clip):
    """The GPU test's two cases.  (t = 1: a depth of one, where the forced trunk needs the layer4 map's gradient as a
    dense copy -- tube_e2e_forced_grads.)"""
    d = _simulated(t, per_clip)
    bad, worst = [], 0.0
    for n, ref in d["plain"].items():
        b, e, _, _ = rule_full(d["forced"][n], ref, ref + (d["yard"][n] - d["forced"][n]))
        worst = max(worst, e)
        bad += [(n,) + x for x in b]
    print(f"forced vs plain fp64 autograd, largest error vector {worst:.3e}")
    assert not bad and worst < 1e-9, (worst, bad)
    viol, w = e2e.grad_violations(d["yard"], d["forced"], d["yard"])  # the yardstick itself: in bound, under the cap
    e_ref = np.array([rule_full(d["yard"][n], r, d["yard"][n])[2] for n, r in d["forced"].items()])
    print(f"yardstick e_ref {e_ref.min():.3e} to {e_ref.max():.3e} median {np.median(e_ref):.3e}")
    assert not viol, viol


def test_forced_detached_gives_the_detached_step():
    d = _simulated()
    det = e2e.tube_e2e_forced_grads(d["sd"], d["spec"], d["video"], d["tape"], detach=True)
    for n in e2e.vid_names():
        assert det[n].abs().max() == 0, n
    for n in tor.trainable_names_tube():  # the audio trunk's gradient does not depend on the video graph
        assert torch.equal(det[n], d["forced"][n]), n


@pytest.mark.parametrize("fault", e2e.E2E_FAULTS)
def test_comparator_flags_gradient_faults(fault):
    """A forced oracle with one wiring fault, held against the right one as the GPU result is: every vidnet tensor is
    out of bound, and no audnet tensor is for the one-clip fault (the audio branch does not see it)."""
    d = _simulated()
    wrong = e2e.tube_e2e_forced_grads(d["sd"], d["spec"], d["video"], d["tape"], fault=fault)
    viol, worst = e2e.grad_violations(wrong, d["forced"], d["yard"])
    flagged = {v[0] for v in viol}
    inside = [n for n in e2e.vid_names() if n not in flagged]
    print(f"{fault}: {len(flagged)} tensors out of bound, largest error {worst[1]:.1f} of its bound ({worst[0]})")
    assert not inside, inside
    if fault == "one_clip":
        assert not any(n.startswith("audnet.") for n in flagged), sorted(flagged)


def test_comparator_flags_fc_in_adam():
    """Adam with weight decay over a parameter set that wrongly includes vidnet.fc (zero gradient): the decay alone
    moves it, and adam_scope_violations says so; over the right set it reports nothing.  A trained parameter that an
    optimizer skipped is reported as frozen."""
    sd = _sd64()
    before = {k: v.clone() for k, v in sd.items()}
    trained, untrained = e2e.e2e_names(), e2e.untrained_names(sd)
    g = torch.Generator().manual_seed(5)
    grads = {n: torch.randn(sd[n].shape, generator=g, dtype=torch.float64) for n in trained}
    opt = orc.AdamRef(lr=1e-4, weight_decay=1e-4)
    opt.step({n: sd[n] for n in trained}, grads)
    assert e2e.adam_scope_violations(before, sd, trained, untrained) == []
    wrong = ["vidnet.fc.weight", "vidnet.fc.bias"]
    opt2 = orc.AdamRef(lr=1e-4, weight_decay=1e-4)
    opt2.step({n: sd[n] for n in wrong}, {n: torch.zeros_like(sd[n]) for n in wrong})
    assert sorted(e2e.adam_scope_violations(before, sd, trained, untrained)) == sorted((n, "moved") for n in wrong)
    sd["vidnet.layer3.0.downsample.0.weight"].copy_(before["vidnet.layer3.0.downsample.0.weight"])
    assert ("vidnet.layer3.0.downsample.0.weight", "frozen") in e2e.adam_scope_violations(before, sd, trained, untrained)
