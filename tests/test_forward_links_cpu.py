"""The forward link oracle (tests/fwdlink.py) is sound and has teeth -- on the CPU, at the shapes of
tests/test_forward_links_gpu.py: images 64 x 64 and spectrograms 65 x 76 at B = 3 (one-frame step), b = 2, t = 2
(two-view step: two vision calls of 4 rows; the audio trunk once over 2 rows at momentum 0.19 / rep 2, or twice over
the 4 folded rows at 0.1).

Sound: on fwdlink.emulate_tape -- the library's composition restated with fp32 conv sums, statistics from the unrounded
values and every stored activation rounded to bf16 -- every link of every run is within its bound.  Teeth: each of 13
wiring faults, injected into the emulation one at a time, puts a link out of bound, and the first link out of bound (in
launch order, buffers last) is the one the fault touches.

The tightened statistics bounds.  Three of the faults stay inside the worst-case statistics bounds (|mean - mean64| <=
u E|c| + .., |var - var64| <= 4u E[c^2] + ..): eps 1e-3 moves var by 1e-3 where 4u E[c^2] is 8e-3 E[c^2]; invstd from
the unbiased variance moves it by var / R (R from 48 to 3762 rows); a stale accumulator or a missing tile can hide there
too at small R.  The deviation the bound covers is a sum of R independent roundings, so fwdlink.stats_link also holds it
in units of its standard scale (fwdlink's docstring): per channel for mean and var, and the signed var deviation
averaged over the channels times sqrt(C).  Measured here on emulate_tape against the same fp64 recomputation, the
maximum over every BN of the reference runs below (140 BN calls): mean 4.22, var 4.18, var_bias 3.05 of their units
(the units take u = 2^-9 / (1 - 2^-9) as the worst-case bounds do; bf16's own unit roundoff is twice that); fwdlink.STAT_Z is 8 x
those rounded up: 8 x 4.4 = 35.2, 8 x 4.4 = 35.2, 8 x 3.2 = 25.6 (the margin covers run-to-run input variation of a
rounding-noise statistic).  test_emulation_within_bounds asserts that the emulation's deviations are at most 1 / 8 of
STAT_Z and at least 1 / 9.2 of it, so the constants cannot drift from what they are said to be.  With them: eps 1e-3
falls out of the worst-case var bound at the stem (ratio 2.0: c0's variance is 0.09); invstd from the unbiased
variance, injected at layer2.1.bn2 (R = 192, C = 128), is caught by var_bias alone, at 4.4 of its bound.  No link is
excluded anywhere.

A fault carried by every BN of a call (R = rows for rows * rep) shows at the first BN whose variance is large enough;
the stems' is not (0.09), so the first link out of bound may be any running_var of that trunk, never another kind.

Worst ratio to its bound per kind over the reference runs (printed by test_emulation_within_bounds): conv 0.992,
apply 0.996, pool 0.990 (one bf16 rounding against 2^-8 |v|: no slack to expect), stats 0.550 (a worst-case mean bound
in layer3 of the audio trunk, R <= 100), affine 0.124, running 0.052, the exact kinds 0."""
import copy

import pytest
import torch

import avenet_oracle as orc
import fwdlink as fl

B, SIZE, FREQ, FRAMES = 3, 64, 65, 76
TV_B, TV_T = 2, 2
M2 = 1.0 - (1.0 - 0.1) ** 2
IMG_BNS, AUD_BNS = fl.bn_names("imgnet."), fl.bn_names("audnet.")
ALL_BNS = IMG_BNS + AUD_BNS


def _state():
    return orc.make_state(0)


def _run(sd, calls, names=ALL_BNS, inc=1, link_sd=None, emu=None, link=None):
    """Emulate calls = [(prefix, modal, x, rep, m)] in order on a copy of sd, then every link of the step.  emu:
    {call index: emulate_tape keywords (a fault, or another rep / momentum than the links expect)}; link_sd: the
    weights the links take (default: sd's); link: a function (work, before, call index) run before that call's
    emulation (a fault on the buffers).  Returns (records, tapes)."""
    work = copy.deepcopy(sd)
    before = fl.snapshot(work, names)
    tapes, lcalls = [], []
    for i, (prefix, modal, x, rep, m) in enumerate(calls):
        kw = dict(rep=rep, momentum=m, calls=0)
        kw.update((emu or {}).get(i, {}))
        if link is not None:
            link(work, before, i)
        tp = fl.emulate_tape(work, x, modal, prefix=prefix, **kw)
        tapes.append(tp)
        lcalls.append((prefix, modal, tp, x, rep, m, tp["blocks"][-1]["out"]))
    for n in names:
        work[n + ".num_batches_tracked"].add_(inc)
    after = fl.snapshot(work, names)
    return fl.step_links(link_sd if link_sd is not None else sd, names, before, after, lcalls, inc), tapes


def _image():
    return orc.make_image(B, SIZE)


def _spec(b=B):
    return orc.make_spectrogram(b, FREQ, FRAMES)


def _views():
    return [orc.fold_frames(orc.make_frames(TV_B, TV_T, SIZE, seed=s)) for s in (3, 4)]


def test_emulation_within_bounds():
    """The five reference runs: the one-frame step's two trunks, the two-view step's two vision calls (chained
    buffers), its de-duplicated audio call (momentum 0.19, rep 2, counters +2) and its two undeduplicated audio calls,
    and the audio pool; every link within its bound, the statistics' deviations at most STAT_Z / 8."""
    sd = _state()
    spec2 = _spec(TV_B)
    runs = {
        "one-frame": ([("imgnet.", "vision", _image(), 1, 0.1), ("audnet.", "audio", _spec(), 1, 0.1)], ALL_BNS, 1),
        "two-view vision": ([("imgnet.", "vision", v, 1, 0.1) for v in _views()], IMG_BNS, 2),
        "two-view audio, de-duplicated": ([("audnet.", "audio", spec2, TV_T, M2)], AUD_BNS, 2),
        "two-view audio, folded": ([("audnet.", "audio", orc.fold_spec(spec2, TV_T), 1, 0.1)] * 2, AUD_BNS, 2),
    }
    dev = {"mean": 0.0, "var": 0.0, "var_bias": 0.0}
    allrec = []
    for tag, (calls, names, inc) in runs.items():
        rec, tapes = _run(sd, calls, names, inc)
        for (prefix, modal, *_), tp in zip(calls, tapes):
            for c, st in [(tp["c0"], tp["st0"])] + [(tb[c], tb[s]) for tb in tp["blocks"]
                                                    for c, s in (("c1", "s1"), ("c2", "s2"), ("cd", "sd")) if c in tb]:
                d = fl.stat_deviations(c, st)
                dev = {k: max(dev[k], d[k]) for k in dev}
            if modal == "audio":
                a = tp["blocks"][-1]["out"]
                rep = calls[0][3]
                an_a, amax, anorm, an = fl.emulate_audio_pool(a, rep)
                rec += fl.audio_pool_link(prefix + "pool", a, an_a, amax, anorm, an, rep)
        print(fl.report(tag, rec))
        bad = fl.failures(rec)
        assert not bad, bad[:5]
        allrec += rec
    print(fl.report("all reference runs", allrec))
    print("largest statistics deviations of the emulation, in their units:", {k: round(v, 3) for k, v in dev.items()})
    for k, v in dev.items():
        assert 8 * v <= fl.STAT_Z[k], (k, v, fl.STAT_Z[k])
        assert fl.STAT_Z[k] <= 8 * 1.15 * v, (k, v, fl.STAT_Z[k])  # and no looser than that, up to rounding up


def _vision(sd, **kw):
    return _run(sd, [("imgnet.", "vision", _image(), 1, 0.1)], IMG_BNS, 1, **kw)[0]


def _audio2(sd, **kw):
    return _run(sd, [("audnet.", "audio", _spec(TV_B), TV_T, M2)], AUD_BNS, 2, **kw)[0]


def _stale_stats(sd, bn):
    """The statistics of `bn` on another batch (the previous call's)."""
    work = copy.deepcopy(sd)
    tp = fl.emulate_tape(work, orc.make_image(B, SIZE, seed=5), "vision")
    return fl.trunk_calls("imgnet.", tp, 1, 0.1)[bn][0]


def _adam_step(sd):
    """One Adam step at lr 1e-2 from zero moments: every conv weight moves by lr * sign(g) (a seeded g)."""
    new = copy.deepcopy(sd)
    gen = torch.Generator().manual_seed(13)
    for n, v in new.items():
        if v.dim() == 4:
            g = torch.randn(v.shape, generator=gen)
            v.sub_(1e-2 * g / (g.abs() + 1e-8))
    return new


def _second_view_from_before(bn):
    def link(work, before, i):
        if i == 1:
            for k in (".running_mean", ".running_var"):
                work[bn + k].copy_(before[bn + k])
    return link


def _tiny_channel(sd):
    """layer1.1.bn2 with channel 0's gamma 0 and beta 1e-42: where the identity is 0 the pre-activation is a positive
    fp32 subnormal that rounds to a bf16 zero -- the one place where [pre > 0] and [out > 0] differ."""
    s = copy.deepcopy(sd)
    s["imgnet.layer1.1.bn2.weight"][0] = 0.0
    s["imgnet.layer1.1.bn2.bias"][0] = 1e-42
    return s


FAULT_CASES = {
    # name: (run, the records that may be the first out of bound)
    "residual from h1": (lambda sd: _vision(sd, emu={0: dict(fault="res_h1", fault_at="imgnet.layer1.0.")}),
                         ("imgnet.layer1.0.out",)),
    "downsample (scale, shift) swapped with bn2's": (
        lambda sd: _vision(sd, emu={0: dict(fault="swap_down", fault_at="imgnet.layer2.0.")}),
        ("imgnet.layer2.0.out", "imgnet.layer2.0.out.zero")),
    "biased running_var": (lambda sd: _vision(sd, emu={0: dict(fault="rv_biased", fault_at="imgnet.layer2.0.bn1")}),
                           ("imgnet.layer2.0.bn1.running_var",)),
    # (every BN of the call carries this fault: the first whose variance is large enough to show 1 / (2 R))
    "R = rows where rows * rep is due": (lambda sd: _audio2(sd, emu={0: dict(rep=1)}),
                                         tuple(n + ".running_var" for n in AUD_BNS)),
    "momentum 0.1 where 0.19 is due": (lambda sd: _audio2(sd, emu={0: dict(momentum=0.1)}),
                                       ("audnet.bn1.running_mean",)),
    "invstd from the unbiased variance": (
        lambda sd: _vision(sd, emu={0: dict(fault="invstd_unbiased", fault_at="imgnet.layer2.1.bn2")}),
        ("imgnet.layer2.1.bn2.var", "imgnet.layer2.1.bn2.var_z", "imgnet.layer2.1.bn2.var_bias")),
    "eps 1e-3": (lambda sd: _vision(sd, emu={0: dict(eps=1e-3)}),
                 ("imgnet.bn1.var", "imgnet.bn1.var_z", "imgnet.bn1.var_bias")),
    "stale statistics on layer3.0.bn2": (
        lambda sd: _vision(sd, emu={0: dict(fault="stale_stats", fault_at="imgnet.layer3.0.bn2",
                                            stale=_stale_stats(sd, "imgnet.layer3.0.bn2"))}),
        ("imgnet.layer3.0.bn2.mean", "imgnet.layer3.0.bn2.var", "imgnet.layer3.0.bn2.mean_z")),
    "a row tile missing from layer1.0.bn1's sum": (
        lambda sd: _vision(sd, emu={0: dict(fault="missing_tile", fault_at="imgnet.layer1.0.bn1")}),
        ("imgnet.layer1.0.bn1.mean", "imgnet.layer1.0.bn1.var", "imgnet.layer1.0.bn1.mean_z")),
    "weights of the previous step": (lambda sd: _vision(sd, link_sd=_adam_step(sd)), ("imgnet.conv1.weight",)),
    "om from the pre-rounding value": (
        lambda sd: _vision(_tiny_channel(sd), emu={0: dict(fault="om_prernd", fault_at="imgnet.layer1.1.")}),
        ("imgnet.layer1.1.om",)),
    "carg from the first window element": (lambda sd: _vision(sd, emu={0: dict(fault="carg_first")}),
                                           ("imgnet.maxpool.carg",)),
    "second view's BN update applied to the before buffer": (
        lambda sd: _run(sd, [("imgnet.", "vision", v, 1, 0.1) for v in _views()], IMG_BNS, 2,
                        link=_second_view_from_before("imgnet.layer2.0.bn1"))[0],
        ("imgnet.layer2.0.bn1.running_mean",)),
}


@pytest.mark.parametrize("case", list(FAULT_CASES))
def test_fault_caught_at_its_link(case):
    """One fault in the emulation: at least one link out of bound, the first of them the link the fault touches."""
    run, expect = FAULT_CASES[case]
    rec = run(_state())
    bad = fl.failures(rec)
    print(f"{case}: {len(bad)} of {len(rec)} links out of bound; first {bad[:1]}")
    assert bad, "the fault stays inside every bound"
    assert bad[0][0] in expect, (bad[0], expect)


def test_tiny_channel_reference_within_bounds():
    """The state the om fault needs (a channel whose positive pre-activations underflow in bf16), without the fault:
    every link within its bound."""
    bad = fl.failures(_vision(_tiny_channel(_state())))
    assert not bad, bad[:5]
