"""The train-mode forward, link by link, on the GPU's own tapes.

The forced-tape backward tests take the forward tape as given; the end-to-end forward checks sit behind the head's
sigmoid((A - eps) / 0.03) at 3 x a bf16 yardstick, where a stale statistic or a wrong residual at layer 2 disappears.
Here every launch group of the forward as Trunk.forward_iter, R3DTrunk.forward, AVEngine.forward, TwoViewEngine.forward
and the tube step compose it is checked on its own: its inputs are taken from the tape (the GPU's own bits), the one
link is recomputed in fp64 (tests/fwdlink.py) and compared with the tape's next tensor, to bounds that follow from one
bf16 rounding and fp32 sums -- nothing is amplified.  Every BN's running statistics and counter are recomputed from
the tape's own mean and invstd, chained over the calls of a step.  tests/test_forward_links_cpu.py shows that the
bounds hold for the reference emulation and that 13 wiring faults fall out of bound at their own link.

Shapes: images 64 x 64, spectrograms 65 x 76, B = 3; two-view b = 2, t = 2; video make_video(2, 4, 64) (R3D-18), the
tube step make_video(2, 4, 32) with one spectrogram per clip.  Each test prints the worst ratio to its bound per link
kind and names the link."""
import pytest
import torch

import avenet_oracle as orc
import fwdlink as fl
import tube_oracle as tor

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B, SIZE, FREQ, FRAMES = 3, 64, 65, 76
TV_B, TV_T, LW = 2, 2, 0.1
M2 = 1.0 - (1.0 - 0.1) ** 2
IMG_BNS, AUD_BNS = fl.bn_names("imgnet."), fl.bn_names("audnet.")


def _model():
    from avt_amd.model import AVENet, HardWayArgs

    m = AVENet(HardWayArgs(), False)
    m.load_state_dict(orc.make_state(0))
    return m.to(DEV).train()


def _state(module):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def _act(t):
    return t.detach().cpu().double()


def _finish(tag, rec):
    print(fl.report(tag, rec))
    bad = fl.failures(rec)
    for r in bad[:20]:
        print("OUT OF BOUND", r)
    assert not bad, bad[:5]


def _inputs():
    return orc.make_image(B, SIZE), orc.make_spectrogram(B, FREQ, FRAMES)


def _one_frame_links(tag, eng, model, training=True):
    """AVEngine.forward on the seeded inputs -> every link of both trunks, the audio pool, all 40 BNs' buffers and
    counters (an eval tape: nothing written)."""
    image, audio = _inputs()
    before = _state(model)
    if training:
        out, tape = eng.forward(image.to(DEV), audio.to(DEV), True, with_ce=True)
    else:
        out, tape = eng.forward(image.to(DEV), audio.to(DEV), False, tape=True)
    after = _state(model)
    calls = [("imgnet.", "vision", fl.cpu_tape(tape["img"]), image, 1, 0.1, _act(tape["v"])),
             ("audnet.", "audio", fl.cpu_tape(tape["aud"]), audio, 1, 0.1, _act(tape["a"]))]
    assert calls[0][2]["training"] == training and calls[1][2]["training"] == training
    rec = fl.step_links(before, IMG_BNS + AUD_BNS, before, after, calls, 1 if training else 0)
    rec += fl.audio_pool_link("audnet.pool", _act(tape["a"]), tape["an"].cpu(), tape["amax"].cpu(),
                              tape["anorm"].cpu())
    if not training:  # no parameter, buffer or counter of the model moved
        rec.append(("state", "running", *fl.exact(torch.tensor([torch.equal(before[k], after[k]) for k in before]))))
    _finish(tag, rec)
    return rec


@pytest.mark.parametrize("mode", ["two_streams", "one_stream", "splitk"])
def test_one_frame_step_links(mode):
    """AVEngine.forward(image, audio, True, with_ce=True) on a fresh model: on two streams (the default), on one
    (concurrent = False) and with engine.splitk (two splits forced with avt_set_halo_splitk(2, 0) when the planner
    splits nothing at these shapes).

    Measured on one MI355X, worst ratio to its bound per kind (563 links each): two streams and one stream give the
    same figures -- conv 0.989 (audnet.conv1_a.weight), apply 0.995 (imgnet.layer2.0.h1), pool 0.994 (imgnet.maxpool),
    stats 0.580 (imgnet.layer3.1.bn2.mean, the worst-case bound at R = 48), affine 0.124, running 0.029
    (audnet.layer2.0.downsample.1.running_var), every exact kind 0.  Split-K: the planner itself splits ten forward
    call sites per trunk (layer2.0.conv2 to layer4.1.conv2); conv 0.989, apply 0.995, pool 0.994, stats 0.572
    (imgnet.layer3.0.bn1.mean), affine 0.124, running 0.029."""
    from avt_amd._lib import call

    def run():
        model = _model()
        eng = model.engine()
        eng.concurrent = mode != "one_stream"
        eng.splitk = mode == "splitk"
        _one_frame_links(f"one-frame step, {mode}", eng, model)
        return eng

    try:
        eng = run()
        if mode == "splitk":
            tickets = [k for k, (_, cnt) in eng._splitk_cnt.items() if cnt is not None]
            if not tickets:
                call("avt_set_halo_splitk", 2, 0)
                eng = run()
                tickets = [k for k, (_, cnt) in eng._splitk_cnt.items() if cnt is not None]
            print(f"split-K forward call sites: {sorted({k[0] for k in tickets if not k[1]})}")
            assert any(not k[1] for k in tickets), "no forward conv was split"
    finally:
        call("avt_set_halo_splitk", 0, 0)


def test_second_step_links():
    """One HardWayTrainStep.step at lr 1e-2, then the forward again: the links take the UPDATED master weights (the
    bf16 packs redone after the device-side Adam) and the first step's buffers as `before` (chained running
    statistics, counters at 2).

    Measured on one MI355X: conv 0.993 (audnet.conv1_a.weight), apply 0.996 (audnet.layer1.0.out), pool 0.995
    (audnet.maxpool), stats 0.578 (imgnet.layer4.0.bn1.mean), affine 0.186, running 0.050
    (audnet.layer3.1.bn1.running_mean), every exact kind 0."""
    from avt_amd.train import HardWayTrainStep

    model = _model()
    step = HardWayTrainStep(model, lr=1e-2)
    image, audio = _inputs()
    w0 = _state(model)
    loss = step.step(image.to(DEV), audio.to(DEV))
    w1 = _state(model)
    assert torch.isfinite(loss).all()
    moved = [k for k in w0 if w0[k].dim() == 4 and not torch.equal(w0[k], w1[k])]
    assert len(moved) >= 40, len(moved)  # the step moved the conv weights: stale packs would show
    assert all(int(w1[n + ".num_batches_tracked"]) == 1 for n in IMG_BNS + AUD_BNS)
    _one_frame_links("second step", step.engine, model)


def test_eval_tape_links():
    """forward(training=False, tape=True) after one train-mode forward (so that the running statistics are not the
    initial 0 / 1): the tape's statistics are (gamma rsqrt(rv + eps), beta - rm scale, rm, rsqrt(rv + eps)), every
    other link as in train mode, and no parameter, buffer or counter is written.

    Measured on one MI355X (444 links): conv 0.993, apply 0.995, pool 0.995, stats 0.139 (an invstd, of its 4 ulp),
    affine 0.124; every buffer and counter bitwise unchanged."""
    model = _model()
    eng = model.engine()
    image, audio = _inputs()
    eng.forward(image.to(DEV), audio.to(DEV), True, with_ce=True)
    _one_frame_links("eval tape", eng, model, training=False)


@pytest.mark.parametrize("dedup", [True, False], ids=["dedup", "nodedup"])
def test_twoview_step_links(dedup):
    """TwoViewTrainStep.step (b = 2, t = 2), the tape taken by spying on step.engine.forward: both vision tapes and
    the vision BNs' two chained updates; the audio trunk once at momentum 0.19 / rep t (de-duplicated) or twice over
    the folded rows at 0.1; the audio pool with avt_repeat_rows_f32 of an; every counter at +2.

    Measured on one MI355X: de-duplicated (789 links) conv 0.991, apply 0.996, pool 0.995, stats 0.566
    (audnet.layer4.0.bn1.mean), affine 0.124, running 0.043 (imgnet.layer4.0.downsample.1.running_var); undeduplicated
    (1008 links) the same but running 0.051 (audnet.layer3.0.downsample.1.running_var); every exact kind 0."""
    from avt_amd.train import TwoViewTrainStep

    frames, augmented, spec = (orc.make_frames(TV_B, TV_T, SIZE, seed=3), orc.make_frames(TV_B, TV_T, SIZE, seed=4),
                               orc.make_spectrogram(TV_B, FREQ, FRAMES))
    model = _model()
    step = TwoViewTrainStep(model, loss_weight=LW, dedup_audio=dedup)
    kept = {}
    orig = step.engine.forward

    def spy(*a, **k):
        out, tape = orig(*a, **k)
        kept["tape"] = tape
        kept["after"] = _state(model)  # (before the optimizer moves the weights)
        return out, tape

    step.engine.forward = spy
    before = _state(model)
    losses = step.step(frames.to(DEV), augmented.to(DEV), spec.to(DEV))
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all()
    tp, after = kept["tape"], kept["after"]
    assert (tp["aud"][0] is tp["aud"][1]) == dedup
    calls = [("imgnet.", "vision", fl.cpu_tape(tp["img"][k]), x, 1, 0.1, _act(tp["head"][k]["v"]))
             for k, x in enumerate((frames, augmented))]
    auds = tp["aud"][:1] if dedup else tp["aud"]
    rep = TV_T if dedup else 1
    xa = spec if dedup else orc.fold_spec(spec, TV_T)
    calls += [("audnet.", "audio", fl.cpu_tape(ta["aud"]), xa, rep, M2 if dedup else 0.1, _act(ta["a"]))
              for ta in auds]
    rec = fl.step_links(before, IMG_BNS + AUD_BNS, before, after, calls, 2)
    for k, ta in enumerate(tp["aud"]):  # each view's head rows
        assert ta["rep"] == rep
        rec += fl.audio_pool_link(f"audnet.pool{k}", _act(ta["a"]), ta["an_a"].cpu(), ta["amax"].cpu(),
                                  ta["anorm"].cpu(), tp["head"][k]["an"].cpu(), rep)
    _finish(f"two-view step, dedup_audio={dedup}", rec)


@pytest.mark.parametrize("max_pool", [False, True])
def test_r3d_links(max_pool):
    """R3DTrunk.forward(video, store, True, tape=True) on make_video(2, 4, 64), with and without the stem max-pool:
    the temporal fold, the stem, every block including the per-frame 2-D downsample, all 20 BatchNorm3d buffers and
    counters.

    Measured on one MI355X (268 links each): without the max-pool conv 0.994 (layer2.0.downsample.0.weight), apply
    0.996, stats 0.305 (layer4.1.bn2.mean), affine 0.185, running 0.024; with it conv 0.992, apply 0.995, the pool
    exact, stats 0.885 (layer4.0.bn1.mean: the worst-case mean bound at R = 16 rows, where a sum of 16 roundings is
    not far from its worst case), affine 0.206, running 0.034."""
    from avt_amd.resnet3D import generate_model
    from avt_amd.tube import R3DEngine

    sd = tor.make_tube_state(0)
    net = generate_model(18, no_max_pool=not max_pool, n_classes=1039)
    net.load_state_dict({k[len("vidnet."):]: v for k, v in sd.items() if k.startswith("vidnet.")})
    net.enable_backward()
    net = net.to(DEV).train()
    engine = R3DEngine(net._flat_store(), "", max_pool=max_pool, with_backward=True)
    video = tor.make_video(2, 4, 64)
    before = _state(net)
    logits, tp = engine.forward(video.to(DEV), True, tape=True)
    after = _state(net)
    assert torch.isfinite(logits).all()
    t3 = fl.cpu_tape3d(tp)
    rec = fl.r3d_links(before, "", t3, video, max_pool)
    calls = fl.r3d_calls("", t3)
    rec += fl.buffer_links(fl.r3d_bn_names(""), before, after, lambda n: [calls[n]], 1)
    _finish(f"R3D-18, max_pool={max_pool}", rec)


def test_tube_step_audio_links():
    """The FullModel tube step's forward with one spectrogram per clip (bn_rep = t): the audio trunk's links, its
    running statistics with the unbiased factor of R = rows * t at momentum 0.1, the audio pool with the repeated
    rows, every counter of the model at +1.

    Measured on one MI355X (285 links): conv 0.991, apply 0.996, pool 0.984, stats 0.570 (audnet.layer4.0.bn2.mean),
    affine 0.189, running 0.027 (audnet.layer2.0.downsample.1.running_var), every exact kind 0."""
    from avt_amd.model import FullModel

    model = FullModel(orc.Args())
    model.load_state_dict(tor.make_tube_state(0))
    model = model.to(DEV).train()
    eng = model.engine()
    b, t = 2, 4
    video, spec = tor.make_video(b, t, 32), orc.make_spectrogram(b, FREQ, FRAMES)
    before = _state(model)
    out, tape = eng.forward(spec.to(DEV), video.to(DEV), True, with_ce=True)
    after = _state(model)
    assert tape["rep"] == t and torch.isfinite(out["loss"]).all()
    calls = [("audnet.", "audio", fl.cpu_tape(tape["aud"]), spec, t, 0.1, _act(tape["a"]))]
    rec = fl.step_links(before, AUD_BNS, before, after, calls, 1)
    rec += fl.audio_pool_link("audnet.pool", _act(tape["a"]), tape["an_a"].cpu(), tape["amax"].cpu(),
                              tape["anorm"].cpu(), tape["an"].cpu(), t)
    nbt = [k for k in before if k.endswith("num_batches_tracked")]
    rec.append(("counters", "counter", *fl.exact(torch.tensor([int(after[k]) - int(before[k]) == 1 for k in nbt]))))
    _finish("tube step, audio de-duplicated", rec)
