"""avenet_oracle.avenet_forced_grads / twoview_forced_grads -- the fp64 reference of the WHOLE step's backward on a
recorded forward (both trunks teacher-forced onto their tapes, the audio pool at the recorded positions, the head in
fp64) that test_step_backward_forced_gpu.py holds AVEngine.backward and TwoViewEngine.backward against -- checked on
the CPU at that test's shapes (images 64 x 64, spectrograms 65 x 76; B = 3 one-frame, b = 2, t = 2 two-view), with
tapes simulated by the fp64 oracle's own forward, every stored tensor rounded to bf16 where it is made
(test_trunk2d_forced_oracle_cpu._recorded_forward, per trunk): forcing is sound (it reproduces plain autograd of the
step), the bf16-storage yardstick stays under the cap, each of five wiring faults of the step falls out of
gradcheck.rule_full's bound, and the data-parallel shards of test_ddp_gpu.py are far enough from the full batch for
test_dp_mean_gradient_forced's sep / 4 to mean something.

Measured on the simulated tapes: forced against plain autograd at most 2.7e-15 on every tensor, in every form; the
yardstick's e_ref 1.8e-3 to 1.42e-2 (one-frame, CE only), 1.5e-3 to 1.47e-2 (CE and the four map cotangents), 1.7e-3
to 1.57e-2 (two-view) and to 2.03e-2 (two-view, undeduplicated), medians 6.1e-3 to 6.5e-3, no tensor above the cap, so
every bound is the 5e-2 floor; the de-duplicated two-view oracle against the undeduplicated one 7.4e-15 on the audio
trunk; sep = 1.155."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import avenet_oracle as orc
from gradcheck import rule_full
from test_trunk2d_forced_oracle_cpu import _bf16, _recorded_forward

E_REF_CAP, MAX_OVER_CAP = 0.1, 6  # the forced tests' condition on the yardstick, per trunk
B, SIZE, FREQ, FRAMES = 3, 64, 65, 76
TV_B, TV_T, LW = 2, 2, 0.1
_CACHE = {}


def _work(sd):
    """(names, the fp64 working state): the trainable parameters as leaves, conv weights at their bf16 values."""
    names = orc.trainable_names(sd)
    s = {k: (v.double().clone() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for n in names:
        s[n] = (_bf16(s[n]) if s[n].dim() == 4 else s[n]).requires_grad_(True)
    return names, s


def _audio_vectors(s, ain):
    """(unit vectors, trunk tape, amax) of AVENet's audio branch on the recorded forward; amax as the pool kernel
    records it: the first maximum's row y * w + x."""
    feat, tape = _recorded_forward(s, "audnet.", ain, "audio")
    amax = feat.detach().flatten(2).argmax(-1)
    return F.normalize(F.adaptive_max_pool2d(feat, 1).flatten(1), dim=1), tape, amax


def _vision_map(s, xin):
    feat, tape = _recorded_forward(s, "imgnet.", xin, "vision")
    return F.normalize(feat, dim=1), tape


def _collect(names, s, inputs):
    g = {n: s[n].grad for n in names}
    g.update({k: x.grad for k, x in inputs.items()})
    assert all(v is not None for v in g.values())
    return g


def _sim_step(maps):
    """The one-frame step simulated: plain fp64 autograd of train_step's network and loss (with the cotangents) on
    the bf16-rounded weights and inputs, every stored tensor rounded where it is made; the tape that forward left;
    the forced oracle and its yardstick on that tape.  Once per cotangent set."""
    key = ("step", maps)
    if key not in _CACHE:
        sd = orc.make_state(0)
        image, audio = orc.make_image(B, SIZE), orc.make_spectrogram(B, FREQ, FRAMES)
        names, s = _work(sd)
        xin, ain = _bf16(image).requires_grad_(True), _bf16(audio).requires_grad_(True)
        vn, tape_i = _vision_map(s, xin)
        an, tape_a, amax = _audio_vectors(s, ain)
        cot = orc.make_cot(B, vn.shape[2], vn.shape[3], maps=maps)
        A, logits, wA, Pos, Neg = orc.hardway_head(vn, an)
        loss = cot["scale"] * orc.hardway_ce(logits)
        if maps:
            loss = loss + sum((cot[k].double().reshape(o.shape) * o).sum()
                              for k, o in (("wA", wA), ("A", A), ("Pos", Pos), ("Neg", Neg)))
        loss.backward()
        plain = _collect(names, s, {"image": xin, "audio": ain})
        tape = {"img": tape_i, "aud": tape_a, "amax": amax}
        assert tuple(tape_a["blocks"][7]["out"].shape[2:]) == (5, 5) and tuple(vn.shape[2:]) == (4, 4)
        forced = orc.avenet_forced_grads(sd, image, audio, tape, cot)
        yard = orc.avenet_forced_grads(sd, image, audio, tape, cot, round_grads=True)
        _CACHE[key] = dict(sd=sd, image=image, audio=audio, tape=tape, cot=cot, plain=plain, forced=forced, yard=yard)
    return _CACHE[key]


def _twoview_inputs():
    return (orc.make_frames(TV_B, TV_T, SIZE, seed=3), orc.make_frames(TV_B, TV_T, SIZE, seed=4),
            orc.make_spectrogram(TV_B, FREQ, FRAMES))


def _sim_twoview(dedup):
    """The two-view step simulated in the same way (twoview_step's network and loss), with the audio trunk run once
    on the b spectrograms and its unit vectors repeated (dedup) or once per view on the folded (b t) rows."""
    key = ("twoview", dedup)
    if key not in _CACHE:
        sd = orc.make_state(0)
        frames, augmented, spec = _twoview_inputs()
        names, s = _work(sd)
        xs = [_bf16(orc.fold_frames(x)).requires_grad_(True) for x in (frames, augmented)]
        views = [_vision_map(s, x) for x in xs]
        if dedup:
            ains = [_bf16(spec).requires_grad_(True)]
            an, tape_a, amax = _audio_vectors(s, ains[0])
            ans, tapes_a, amaxs = [an.repeat_interleave(TV_T, 0)] * 2, [tape_a], [amax]
        else:
            ains = [_bf16(orc.fold_spec(spec, TV_T)).requires_grad_(True) for _ in range(2)]
            auds = [_audio_vectors(s, a) for a in ains]
            ans, tapes_a, amaxs = [a[0] for a in auds], [a[1] for a in auds], [a[2] for a in auds]
        outs = [orc.hardway_head(vn, an) for (vn, _), an in zip(views, ans)]
        orc.twoview_losses(outs[0], outs[1], TV_B, TV_T, LW)[0].backward()
        inputs = {"frames": xs[0], "augmented": xs[1]}
        inputs.update(zip(("audio",) if dedup else ("audio1", "audio2"), ains))
        plain = _collect(names, s, inputs)
        tape = {"img": [t for _, t in views], "aud": tapes_a, "amax": amaxs}
        kw = dict(loss_weight=LW, dedup_audio=dedup)
        forced = orc.twoview_forced_grads(sd, frames, augmented, spec, tape, **kw)
        yard = orc.twoview_forced_grads(sd, frames, augmented, spec, tape, round_grads=True, **kw)
        _CACHE[key] = dict(sd=sd, tape=tape, kw=kw, plain=plain, forced=forced, yard=yard)
    return _CACHE[key]


FORMS = {"ce": lambda: _sim_step(False), "ce+maps": lambda: _sim_step(True),
         "twoview": lambda: _sim_twoview(True), "twoview-nodedup": lambda: _sim_twoview(False)}


@pytest.mark.parametrize("form", FORMS)
def test_forcing_is_sound(form):
    """The forced oracle on the simulated tape against plain fp64 autograd of the same step, all 120 parameter
    gradients and the input gradients inside the rule and within 1e-9 (the level the one-trunk test accepts): on a
    tape the network itself made, forcing adds zeros."""
    d = FORMS[form]()
    assert sorted(d["plain"]) == sorted(d["forced"]) and len(orc.trainable_names(d["sd"])) == 120
    bad, worst = [], 0.0
    for n, ref in d["plain"].items():
        b, e, _, _ = rule_full(d["forced"][n], ref, ref + (d["yard"][n] - d["forced"][n]))
        worst = max(worst, e)
        bad += [(n,) + x for x in b]
    print(f"{form}: forced vs plain fp64 autograd, largest error vector {worst:.3e}")
    assert not bad, bad
    assert worst < 1e-9, worst


@pytest.mark.parametrize("form", FORMS)
def test_forced_yardstick_within_cap(form):
    """The bf16-hook yardstick's own error vector against the forced fp64 gradients: per trunk (its parameters and
    its inputs) at most MAX_OVER_CAP tensors above E_REF_CAP."""
    d = FORMS[form]()
    e_ref = {n: rule_full(d["yard"][n], ref, d["yard"][n])[2] for n, ref in d["forced"].items()}
    v = np.array(list(e_ref.values()))
    print(f"{form}: forced yardstick e_ref max {v.max():.3e} median {np.median(v):.3e} min {v.min():.3e}")
    for trunk in ("audnet.", "imgnet."):
        mine = (lambda n: n.startswith(("audnet.", "audio"))) if trunk == "audnet." else \
            (lambda n: not n.startswith(("audnet.", "audio")))
        over = [(n, round(e, 4)) for n, e in e_ref.items() if mine(n) and e > E_REF_CAP]
        print(f"{form} {trunk}: above {E_REF_CAP}: {over}")
        assert len(over) <= MAX_OVER_CAP, over


def test_dedup_oracle_equals_undeduplicated():
    """For a fixed forward the audio trunk's backward is linear in its upstream gradient and BatchNorm over t
    identical copies of each row has the rows' own statistics: the de-duplicated oracle's audio-trunk gradients are
    the undeduplicated one's (two trunks' summed), the spectrogram gradient the sum over its 2 t copies."""
    d, u = _sim_twoview(True), _sim_twoview(False)
    worst = 0.0
    for n, ref in u["forced"].items():
        if n.startswith("audnet."):
            worst = max(worst, rule_full(d["forced"][n], ref, ref)[1])
    gx = (u["forced"]["audio1"] + u["forced"]["audio2"]).reshape(TV_B, TV_T, *u["forced"]["audio1"].shape[1:]).sum(1)
    worst = max(worst, rule_full(d["forced"]["audio"], gx, gx)[1])
    print(f"de-duplicated vs undeduplicated forced oracle, audio trunk: largest error vector {worst:.3e}")
    assert worst < 1e-6, worst


def _out_of_bound(wrong, d):
    out = [n for n, ref in d["forced"].items() if rule_full(wrong[n], ref, d["yard"][n])[0]]
    least = min(rule_full(wrong[n], d["forced"][n], d["yard"][n])[3] for n in out) if out else 0.0
    return out, least


@pytest.mark.parametrize("fault", orc.STEP_FAULTS)
def test_forced_oracle_sees_step_miswiring(fault):
    """A forced oracle with one wiring fault of the step, held against the right one as a GPU result would be: every
    gradient the fault reaches falls out of rule_full's bound (so the GPU test cannot pass with that fault in the
    step) -- the audio trunk's 60 and its input's for detach_audio, pool_spread and gan_overwrite, the vision trunk's
    and its input's for const_norm, all 122 for ce_sum.  Measured, the smallest error in units of its bound:
    detach_audio 20.0, const_norm 17.1, pool_spread 7.5, ce_sum 40.0, gan_overwrite 11.9."""
    if fault == "gan_overwrite":
        d = _sim_twoview(True)
        frames, augmented, spec = _twoview_inputs()
        wrong = orc.twoview_forced_grads(d["sd"], frames, augmented, spec, d["tape"], fault=fault, **d["kw"])
    else:
        d = _sim_step(False)
        wrong = orc.avenet_forced_grads(d["sd"], d["image"], d["audio"], d["tape"], d["cot"], fault=fault)
    out, least = _out_of_bound(wrong, d)
    print(f"{fault}: {len(out)} of {len(d['forced'])} tensors out of bound (the least at {least:.2f} of its bound): "
          f"{sorted(out)[:4]} ...")
    audio = [n for n in d["forced"] if n.startswith(("audnet.", "audio"))]
    reached = {"ce_sum": list(d["forced"]), "const_norm": [n for n in d["forced"] if n not in audio]}.get(fault, audio)
    assert len(reached) >= 61 and not set(reached) - set(out), sorted(set(reached) - set(out))


def dp_separation():
    """(sep, fp64 shard-mean gradient vector): the relative distance between the fp64 full-batch gradient and the
    mean of the two shards' fp64 gradients (test_ddp_gpu._shards: local negatives per shard), from plain
    orc.train_step -- the oracle alone."""
    if "sep" not in _CACHE:
        from test_ddp_gpu import _shards

        shards = _shards()
        img, aud = torch.cat([s[0] for s in shards]), torch.cat([s[1] for s in shards])
        names = orc.trainable_names(orc.make_state(0))

        def vec(batches):
            gs = []
            for i, a in batches:
                sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in orc.make_state(0).items()}
                gs.append(orc.train_step(sd, i.double(), a.double())[2])
            return torch.cat([sum(g[n] for g in gs).flatten() / len(gs) for n in names])

        mean = vec(shards)
        full = vec([(img, aud)])
        _CACHE["sep"] = (((full - mean).norm() / mean.norm()).item(), mean)
    return _CACHE["sep"]


def test_dp_shards_are_separated():
    """test_dp_mean_gradient_forced's condition on its inputs: sep >= 0.2."""
    sep, _ = dp_separation()
    print(f"fp64 full-batch gradient vs the shard mean: sep = {sep:.3f}")
    assert sep >= 0.2, sep
