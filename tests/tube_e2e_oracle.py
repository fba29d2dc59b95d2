"""fp64 restatement of the tube step with the video features ATTACHED (FullModel.enable_video_backward) -- test
infrastructure, shared by test_tube_e2e_oracle_cpu.py and test_tube_e2e_gpu.py.

The reference's layer4 hook stores ``output.detach()`` (model.py:14), and tube_oracle.fullmodel_forward restates that.
Here the same forward keeps the layer4 map on the graph (``detach=False``; ``detach=True`` puts the reference's
behaviour back, and test_tube_e2e_oracle_cpu.py pins it to tube_oracle.tube_train_step), and a forced-tape variant
(tube_oracle.r3d18_forward_forced for the video trunk, avenet_oracle's forced audio trunk and pool) takes the GPU's own
tapes, so that the fp64 head sees bit-identical maps: the reference of TubeEngine's backward on its own forward.

Also here, so that the CPU test can show what they catch: the comparators the GPU test applies -- ``grad_violations``
(gradcheck.rule_full per tensor and the forced tests' condition on the yardstick, per trunk) and
``adam_scope_violations`` (which parameters an optimizer may move)."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

import avenet_oracle as orc
import tube_oracle as tor
from gradcheck import rule_full

E_REF_CAP, MAX_OVER_CAP = 0.1, 6  # the forced tests' condition on the yardstick, per trunk
E2E_FAULTS = ("gv_unnormalised", "one_clip")


def vid_names():
    """The vidnet parameters the layer4 map depends on: conv1, bn1, layer1..4 with their downsamples (not fc)."""
    return [n for n, _, kind in tor.r3d18_entries("vidnet.") if kind in ("conv", "bn_w", "bn_b")]


def e2e_names():
    """Every parameter that receives a gradient on the end-to-end tube step, in state_dict order."""
    return vid_names() + tor.trainable_names_tube()


def untrained_names(sd):
    """Floating-point parameters no gradient reaches: vidnet.fc.*, the unused audnet stems and fc."""
    train = set(e2e_names())
    return [k for k, v in sd.items() if v.is_floating_point() and k not in train
            and not k.endswith(("running_mean", "running_var"))]


def tube_e2e_forward(sd, audio, video, training=True, detach=False):
    """tube_oracle.fullmodel_forward with the video features attached: audio [(b t),1,F,T], video [b,3,t,H,W] ->
    (A, logits).  detach=True: the reference's hook (``output.detach()``)."""
    B = audio.shape[0]
    aud = orc.resnet18_forward(sd, "audnet.", audio, "audio", training)
    aud = F.normalize(F.adaptive_max_pool2d(aud, 1).view(B, -1), dim=1)
    vid = tor.r3d18_forward(sd, "vidnet.", video, training)
    if detach:
        vid = vid.detach()
    return orc.hardway_attention(aud, F.normalize(vid, dim=1))


def tube_e2e_step(sd, spec, video, detach=False, names=None):
    """(loss, A, logits, {name: gradient}) of CE(logits, 0) for one train_3D.py step on the per-clip spectrograms
    [b,1,F,T] (repeated t times and folded, train_3D.py:128-130).  names: the leaves (default: e2e_names(), or the
    audio trunk's alone when detached); sd's buffers are updated as by tube_oracle.tube_train_step."""
    if names is None:
        names = tor.trainable_names_tube() if detach else e2e_names()
    leaves = {n: sd[n].detach().clone().requires_grad_(True) for n in names}
    work = OrderedDict(sd)
    work.update(leaves)
    A, logits = tube_e2e_forward(work, tor.repeat_spectrogram(spec, video.shape[2]), video, True, detach)
    loss = orc.hardway_ce(logits)
    gl = torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)
    return loss.detach(), A.detach(), logits.detach(), {n: g for n, g in zip(names, gl)}


def forced_leaves(sd):
    """{name: fp64 leaf} of e2e_names(): conv weights at their bf16-rounded values (the operands the trunks compute
    with), BN parameters as they are."""
    s = {}
    for n in e2e_names():
        v = sd[n].detach()
        v = v.to(torch.bfloat16) if v.dim() >= 4 else v
        s[n] = v.to(torch.float64).clone().requires_grad_(True)
    return s


def tube_e2e_forced_grads(sd, audio, video, tape, cot_A=None, round_grads=False, fault=None, detach=False):
    """The end-to-end tube step's backward on a recorded forward: {name: fp64 gradient} for e2e_names() of
        CE(logits, 0) [+ <cot_A, A>]
    with the video trunk teacher-forced onto tape["vid"] (NCDHW: c0, h0, blocks; tube_oracle.r3d18_forward_forced) and
    the audio trunk onto tape["aud"] (NCHW: c0, p0, blocks; avenet_oracle.resnet18_forward_forced), the audio pool
    taken at tape["amax"], and the normalisations and the head in fp64.  audio: what the step was given -- the folded
    [(b t),1,F,T] batch, or one spectrogram per clip [b,1,F,T], whose unit vectors are then repeated t times ('(b t)'
    rows), so that the audio trunk receives the gradient summed over each clip's frames.
    round_grads: the yardstick -- every activation gradient the trunks store in bf16 is rounded to bf16 (both layer4
    maps' included); the head's internals stay unrounded (fp32 on the GPU).  detach: the reference's detached layer4
    (the vidnet gradients are then zero).
    fault (tests only; E2E_FAULTS): "gv_unnormalised" -- the video map's L2 normalisation passes the gradient straight
    through (gv = dvh, not inv * (dvh - vh <vh, dvh>)); "one_clip" -- only clip 0's frames of the layer4 map receive a
    gradient."""
    assert fault is None or fault in E2E_FAULTS, fault
    b, t = video.shape[0], video.shape[2]
    s = forced_leaves(sd)
    rnd = orc._bf16_round if round_grads else None
    ain = orc._bf16_leaf(audio)
    an = orc._forced_audio_vectors(s, ain, tape["aud"], tape["amax"], rnd, None)
    if audio.shape[0] == b and t > 1:
        an = an.repeat_interleave(t, 0)
    assert an.shape[0] == b * t
    v = tor.r3d18_forward_forced(s, "vidnet.", video, orc._tape64(tape["vid"]), grad_round=rnd)
    # the map's gradient enters the forced trunk as a dense NCDHW copy: at t = 1 (a depth of one, whose stride is
    # arbitrary) torch's CPU backward of the forced block otherwise returns other numbers than plain autograd of the
    # same network (test_tube_e2e_oracle_cpu.py::test_forcing_is_sound_and_yardstick_within_cap[t1-folded])
    v = v * 1.0
    if v.requires_grad:
        v.register_hook(lambda g: g.contiguous().clone())
    if detach:
        v = v.detach()
    elif fault == "one_clip":
        keep = torch.zeros(b, 1, 1, 1, 1, dtype=v.dtype)
        keep[0] = 1
        v = v * keep + (v * (1 - keep)).detach()
    vn = F.normalize(v, dim=1)
    if fault == "gv_unnormalised":
        vn = v + (vn - v).detach()
    A, logits = orc.hardway_attention(an, vn)
    loss = orc.hardway_ce(logits)
    if cot_A is not None:
        loss = loss + (cot_A.double().reshape(A.shape) * A).sum()
    loss.backward()
    return {n: orc._grad_or_zero(s[n]) for n in s}


def head_gv_reference(v, an, cot_A=None):
    """fp64 autograd of the head alone at the GPU's saved tensors: v [B,h,w,C] (the bf16 layer4 map, '(b t) h w c'),
    an [B,C] (the fp32 unit audio vectors) -> d (CE(logits, 0) [+ <cot_A, A>]) / d v, [B,h,w,C]."""
    vt = v.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    A, logits, _, _, _ = orc.hardway_head(F.normalize(vt, dim=1), an.double(), 0.65, 0.4, 0.03, True, True)
    loss = orc.hardway_ce(logits)
    if cot_A is not None:
        loss = loss + (cot_A.double().reshape(A.shape) * A).sum()
    loss.backward()
    return vt.grad.permute(0, 2, 3, 1)


def grad_violations(grads, ref, yard, names=None):
    """The GPU test's comparator: every tensor of `names` (default: all of ref) by gradcheck.rule_full against the
    forced reference with the bf16-storage yardstick, and the forced tests' condition on the yardstick (per trunk at
    most MAX_OVER_CAP tensors with e_ref above E_REF_CAP).  Returns (violations, worst) -- violations a list of
    (name, kind, value, yardstick's value), "yardstick" entries for a trunk over the cap; worst = (name, the largest
    error as a fraction of its bound)."""
    names = list(ref) if names is None else names
    bad, over, worst = [], {"vidnet.": [], "audnet.": []}, (None, 0.0)
    for n in names:
        if n not in grads or grads[n] is None:
            bad.append((n, "missing", None, None))
            continue
        assert tuple(grads[n].shape) == tuple(ref[n].shape), n
        viol, e, e_ref, ratio = rule_full(grads[n], ref[n], yard[n])
        if e_ref > E_REF_CAP:
            over[n[:7]].append((n, round(e_ref, 4)))
        if ratio > worst[1]:
            worst = (n, ratio)
        bad += [(n,) + x for x in viol]
    for k, v in over.items():
        if len(v) > MAX_OVER_CAP:
            bad.append((k, "yardstick", len(v), MAX_OVER_CAP))
    return bad, worst


def adam_scope_violations(before, after, trained, untrained):
    """Which parameters moved that may not, and which did not that must: before / after {name: tensor} (compared
    bitwise), trained / untrained name lists.  Returns a list of (name, "moved" | "frozen")."""
    bad = [(n, "moved") for n in untrained if not torch.equal(before[n], after[n])]
    bad += [(n, "frozen") for n in trained if torch.equal(before[n], after[n])]
    return bad
