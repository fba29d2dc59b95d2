"""The whole train step's backward -- AVEngine.backward (the head's backward into gv and gan, gan through the audio
pool/normalise backward, both trunks interleaved on two streams over one store, optionally in two segments or with
on_trunk_end) and TwoViewEngine.backward (two views' heads accumulating one gan, avt_sum_rep_rows_f32 over the frames,
the vision trunk's gradients summed over the views) -- against fp64 autograd on the GPU's OWN forward state:
avenet_oracle.avenet_forced_grads / twoview_forced_grads force both trunks onto the step's tapes, so the fp64 head sees
bit-identical layer4 maps and the sigmoid((A - eps) / 0.03) that makes a bf16 rerun of the network 56 % wrong at these
sizes amplifies nothing.  What is left is what the composition can get wrong: the scale and routing of gan, the
normalisation backwards, the second view's audio gradient, which tape feeds which trunk, the shared workspaces of the
two streams.  tests/test_step_forced_oracle_cpu.py shows on the CPU that the oracle is sound, that its yardstick meets
the cap and that five such wiring faults fall out of bound.

Shapes: images 64 x 64 (layer4 map 4 x 4), spectrograms 65 x 76 (33 x 38 -> 17 x 19 -> 9 x 10 -> 5 x 5: ragged
stride-2 parity classes), B = 3 one-frame, b = 2, t = 2 two-view.  Every tensor by gradcheck.rule_full against the
forced oracle, the yardstick the same oracle with every bf16-stored activation gradient rounded to bf16; condition:
per trunk at most 6 tensors with the yardstick's own e_ref above 0.1.  The stem max-pool's routing among bf16 ties
(test_trunk2d_backward_forced_gpu.py's docstring) carries over: it sits inside the 5e-2 floor on the two stem weights
and the inputs."""
import numpy as np
import pytest
import torch

import avenet_oracle as orc
from gradcheck import rule_full

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
E_REF_CAP, MAX_OVER_CAP = 0.1, 6  # the forced tests' condition on the yardstick, per trunk
B, SIZE, FREQ, FRAMES = 3, 64, 65, 76
TV_B, TV_T, LW = 2, 2, 0.1
_REFS = []  # (key, tape, ref, yard): the oracle's gradients, computed once per distinct GPU tape and loss


def _nchw(t):
    """[N, H, W, C] bf16 on the GPU -> [N, C, H, W] fp32 on the CPU."""
    return t.permute(0, 3, 1, 2).float().cpu()


def _trunk_tape(tp):
    tape = {"c0": _nchw(tp["c0"]), "p0": _nchw(tp["blocks"][0]["x"]), "blocks": []}
    for tb in tp["blocks"]:
        tape["blocks"].append({k: _nchw(tb[k]) for k in ("c1", "h1", "c2", "cd", "out") if k in tb})
    return tape


def _same(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return torch.equal(a, b)


def _forced(key, tape, fn):
    """(ref, yard) = fn(round_grads=False / True) on this tape; shared by the runs whose forward gave the same bits."""
    for k, t, ref, yard in _REFS:
        if k == key and _same(t, tape):
            return ref, yard
    ref, yard = fn(round_grads=False), fn(round_grads=True)
    _REFS.append((key, tape, ref, yard))
    return ref, yard


def _check(tag, grads, ref, yard, names=None):
    """Every tensor of `names` (default: all of ref) by rule_full; the condition on the yardstick per trunk.  Returns
    the largest error as a fraction of its bound."""
    names = list(ref) if names is None else names
    assert all(n in grads for n in names), sorted(set(names) - set(grads))
    bad, over, e_refs, worst = [], {"aud": [], "img": []}, [], (None, 0.0)
    for n in names:
        assert tuple(grads[n].shape) == tuple(ref[n].shape), n
        viol, e, e_ref, ratio = rule_full(grads[n], ref[n], yard[n])
        print(f"  {n}: e {e:.3e} e_ref {e_ref:.3e} ({ratio:.2f} of its bound)")
        e_refs.append(e_ref)
        if e_ref > E_REF_CAP:
            over["aud" if n.startswith(("audnet.", "audio")) else "img"].append((n, round(e_ref, 4)))
        if ratio > worst[1]:
            worst = (n, ratio)
        bad += [(n,) + v for v in viol]
    e_refs = np.array(e_refs)
    print(f"{tag}: forced yardstick e_ref {e_refs.min():.3e} to {e_refs.max():.3e} median {np.median(e_refs):.3e}; "
          f"above {E_REF_CAP}: {over}; largest error {worst[1]:.2f} of its bound ({worst[0]})")
    for b in bad:
        print("OUT OF BOUND", b)
    assert all(len(v) <= MAX_OVER_CAP for v in over.values()), over
    assert not bad, bad
    return worst[1]


def _model():
    from avt_amd.model import AVENet, HardWayArgs

    m = AVENet(HardWayArgs(), False)
    m.load_state_dict(orc.make_state(0))
    return m.to(DEV).train()


def _inputs():
    return orc.make_image(B, SIZE), orc.make_spectrogram(B, FREQ, FRAMES)


def _run(maps=False, inputs=None, want_dx=False, splitk=False, defer=False, concurrent=True, on_boundary=None,
         on_trunk_end=None, seen=None, monkeypatch=None):
    """One step of a fresh model from the seeded weights: AVEngine.forward(image, audio, True, with_ce=True), then
    backward(tape, dlogits, gflat[, the four map cotangents]).  Returns (engine, tape, out, gflat on the CPU, cot).
    seen (with monkeypatch): receives (slabs pending before, after) each flush_wgrad."""
    image, audio = _inputs() if inputs is None else inputs
    eng = _model().engine()
    eng.defer_wgrad, eng.concurrent, eng.splitk = defer, concurrent, splitk
    if seen is not None:
        for tr in (eng.img, eng.aud):
            def flush(store, tr=tr, orig=tr.flush_wgrad):
                pend = store.wgrad_pending(tr.prefix)
                before = None if pend is None else len(pend)
                orig(store)
                seen.append((before, None if pend is None else len(pend)))
            monkeypatch.setattr(tr, "flush_wgrad", flush)
    out, tape = eng.forward(image.to(DEV), audio.to(DEV), True, with_ce=True)
    h, w = out["v"].shape[1:3]
    cot = orc.make_cot(image.shape[0], h, w, maps=maps)
    if want_dx:
        tape["img"]["want_dx"] = tape["aud"]["want_dx"] = True
    gflat = torch.zeros(eng.flat.n_train, device=DEV, dtype=torch.float32)
    kw = dict(dwA=cot["wA"].to(DEV), dA=cot["A"].to(DEV), dPos=cot["Pos"].to(DEV), dNeg=cot["Neg"].to(DEV)) if maps \
        else {}
    eng.backward(tape, out["dlogits"], gflat, on_boundary=on_boundary, on_trunk_end=on_trunk_end, **kw)
    torch.cuda.synchronize()
    assert eng.store.pending is None and eng.store.grads is None
    return eng, tape, out, gflat.cpu(), cot


def _step_grads(eng, tape, gflat, want_dx):
    grads = {n: g.detach().double() for n, g in eng.flat.param_grad_views(gflat).items()}
    if want_dx:
        grads["image"], grads["audio"] = tape["img"]["dx"].double().cpu(), tape["aud"]["dx"].double().cpu()
    return grads


def _step_oracle(tape, cot, inputs=None, tag="step"):
    """(ref, yard) of avenet_forced_grads on the step's tape."""
    image, audio = _inputs() if inputs is None else inputs
    assert tuple(tape["a"].shape[1:3]) == (5, 5)
    t = {"img": _trunk_tape(tape["img"]), "aud": _trunk_tape(tape["aud"]), "amax": tape["amax"].cpu()}
    assert torch.equal(t["img"]["blocks"][7]["out"], _nchw(tape["v"]))  # the head's inputs are the tapes' maps
    assert torch.equal(t["aud"]["blocks"][7]["out"], _nchw(tape["a"]))
    sd = orc.make_state(0)
    return _forced((tag, cot["wA"] is not None), t,
                   lambda round_grads: orc.avenet_forced_grads(sd, image, audio, t, cot, round_grads=round_grads))


@pytest.mark.parametrize("maps", [False, True], ids=["ce", "ce+maps"])
def test_step_forced_tape(maps, monkeypatch):
    """AVEngine.forward(image, audio, True, with_ce=True), then backward(tape, dlogits, gflat) with both trunk tapes'
    want_dx -- once from dlogits alone (loss = CE(logits, 0)), once with dense standard-normal dwA, dA, dPos, dNeg as
    well (make_cot) -- against avenet_forced_grads fed the tape: all 120 parameter gradients and the two input
    gradients by rule_full, the yardstick within the cap.  The audio pool is taken at the GPU's amax (the oracle
    asserts that it holds the channel maxima).

    Measured on one MI355X (no tensor above the cap, so every bound is the 5e-2 floor): CE only, the yardstick's e_ref
    is 1.6e-3 to 1.49e-2, median 6.0e-3; this build's largest error 0.62 of its bound (audio input, e 3.1e-2), then
    0.54 (image), 0.52 (imgnet.conv1.weight) and 0.41 (audnet.conv1_a.weight) -- the stem's routing among bf16 ties
    -- and, everything else, 0.31 (both bn1.bias, e 1.6e-2 against e_ref 1.2e-2 to 1.5e-2).  CE and the four maps:
    e_ref 1.5e-3 to 1.24e-2, median 6.0e-3; largest error 0.74 (audio input, e 3.7e-2), 0.50 (image), 0.47 and 0.40
    (the stem weights), everything else below 0.30."""
    import avt_amd.trunk

    monkeypatch.setattr(avt_amd.trunk, "FUSE_BN_BWD", False)
    eng, tape, out, gflat, cot = _run(maps, want_dx=True)
    assert torch.isfinite(gflat).all() and gflat.abs().sum() > 0
    ref, yard = _step_oracle(tape, cot)
    assert len(ref) == 122
    _check(f"one-frame step, {'CE + maps' if maps else 'CE'}", _step_grads(eng, tape, gflat, True), ref, yard)


def test_step_variants_bitwise(monkeypatch):
    """The ways of issuing the same launches, each on a fresh model from the same seed, held bitwise (loss and flat
    gradient, torch.equal) to the default run (CE only, two streams, one segment, no deferral): the default run a
    second time -- the check on the two streams' sharing of the store, the split-K, head and BN workspaces: run
    once more, not in a loop; a difference is a finding to trace in _interleave and the store --, the input
    gradients asked for (want_dx), two segments (on_boundary, called with the hi then the lo tags), on_trunk_end
    (called once per trunk), one stream (concurrent = False), and defer_wgrad on, in one segment and in two.  The
    deferred runs must have had slabs pending and left none; where the planner defers nothing at B = 3 they run
    again, with their own baseline, under avt_set_wgrad_policy(0, 1) (splits one k-tile deep), as
    test_engine_variants_bitwise does.

    Measured on one MI355X: every variant bitwise equal to the default run, the second default run included.  At
    B = 3 the planner's own splits leave no slab to defer (0 pending); under avt_set_wgrad_policy(0, 1): 12 slabs
    pending in the one-segment run and 12 in the two-segment run, none left."""
    import avt_amd.trunk
    from avt_amd._lib import call

    monkeypatch.setattr(avt_amd.trunk, "FUSE_BN_BWD", False)

    def run(**kw):
        _, _, out, g, _ = _run(monkeypatch=monkeypatch, **kw)
        return out["loss"].item(), g

    def deferred(loss0, g0):
        seen, seen2 = [], []
        loss, g = run(defer=True, seen=seen)
        assert all(a == 0 for _, a in seen), seen
        assert loss == loss0 and torch.equal(g, g0), "defer_wgrad changes the gradient bits"
        loss, g = run(defer=True, on_boundary=lambda t: None, seen=seen2)
        assert len(seen2) == 4 and all(a == 0 for _, a in seen2), seen2  # a flush per trunk and segment
        assert loss == loss0 and torch.equal(g, g0), "defer_wgrad in two segments changes the gradient bits"
        return sum(b for b, _ in seen), sum(b for b, _ in seen2)

    loss0, g0 = run()
    assert np.isfinite(loss0) and torch.isfinite(g0).all() and g0.abs().sum() > 0
    loss, g = run()
    assert loss == loss0 and torch.equal(g, g0), "the default step run a second time gives other bits"
    loss, g = run(want_dx=True)
    assert loss == loss0 and torch.equal(g, g0), "asking for the input gradients changes the gradient bits"
    tags = []
    loss, g = run(on_boundary=tags.append)
    assert tags == [("imgnet.hi", "audnet.hi"), ("imgnet.lo", "audnet.lo")], tags
    assert loss == loss0 and torch.equal(g, g0), "the two-segment backward changes the gradient bits"
    ended = []
    loss, g = run(on_trunk_end=lambda tr: ended.append(tr.prefix))
    assert sorted(ended) == ["audnet.", "imgnet."], ended
    assert loss == loss0 and torch.equal(g, g0), "on_trunk_end changes the gradient bits"
    loss, g = run(concurrent=False)
    assert loss == loss0 and torch.equal(g, g0), "one-stream issue changes the gradient bits"
    try:
        pending = deferred(loss0, g0)
        print(f"deferred wgrad slabs, the planner's own splits: {pending}")
        if not all(pending):
            call("avt_set_wgrad_policy", 0, 1)
            pending = deferred(*run())
            print(f"deferred wgrad slabs, splits of one k-tile: {pending}")
        assert all(pending), pending  # slabs were pending at some point, in one segment and in two
    finally:
        call("avt_set_wgrad_policy", 0, 4)  # the library's defaults


@pytest.mark.parametrize("mode", ["splitk", "fuse_bn_bwd"])
def test_step_modes_against_oracle(mode, monkeypatch):
    """The modes whose bits legitimately differ, against the oracle fed their own tape (CE only): engine.splitk (the
    layer3/4 3x3/s1 convs through the split-K kernels, forward and dgrad, on both streams at once; at least one call
    site split, every ticket array left zero) and FUSE_BN_BWD (the BN-backward reductions carried by the dgrad
    epilogues).

    Measured on one MI355X: split-K -- the planner itself splits ten call sites per trunk, forward and dgrad each
    (layer2.0.conv2 to layer4.1.conv2); yardstick e_ref 1.7e-3 to 1.54e-2, median 6.2e-3; largest error 0.50 of its
    bound (imgnet.conv1.weight), 0.41 (audnet.conv1_a.weight), everything else at most 0.33 (imgnet.bn1.bias).
    FUSE_BN_BWD (the default run's tape and yardstick): 0.52 (imgnet.conv1.weight), 0.40 (audnet.conv1_a.weight),
    everything else below 0.30."""
    import avt_amd.trunk
    from avt_amd._lib import call

    monkeypatch.setattr(avt_amd.trunk, "FUSE_BN_BWD", mode == "fuse_bn_bwd")
    splitk = mode == "splitk"

    def tickets(eng):
        return {k: cnt for k, (_, cnt) in eng._splitk_cnt.items() if cnt is not None}

    try:
        eng, tape, out, gflat, cot = _run(splitk=splitk)
        if splitk and not tickets(eng):  # the planner splits nothing at these shapes: force two splits
            call("avt_set_halo_splitk", 2, 0)
            eng, tape, out, gflat, cot = _run(splitk=True)
        ref, yard = _step_oracle(tape, cot)
        _check(f"one-frame step, {mode}", _step_grads(eng, tape, gflat, False), ref, yard,
               names=orc.trainable_names(orc.make_state(0)))
        if splitk:
            tk = tickets(eng)
            print(f"split-K call sites {sorted({(k[0], 'dgrad' if k[1] else 'fwd') for k in tk})}")
            assert any(k[0].startswith(("imgnet.layer3.", "imgnet.layer4.")) for k in tk), sorted(eng._splitk_cnt)
            assert any(k[0].startswith(("audnet.layer3.", "audnet.layer4.")) for k in tk), sorted(eng._splitk_cnt)
            assert all(int(cnt.abs().sum()) == 0 for cnt in tk.values()), "split-K tickets not left zero"
    finally:
        call("avt_set_halo_splitk", 0, 0)


_TWOVIEW = {}


def _twoview(dedup):
    """TwoViewTrainStep.step on a fresh model (b = 2, t = 2), the tape taken by spying on step.engine.forward (which
    also asks every trunk tape for its input gradient): (the step's gradients and input gradients, oracle ref,
    yard).  Once per form."""
    if dedup in _TWOVIEW:
        return _TWOVIEW[dedup]
    from avt_amd.train import TwoViewTrainStep

    frames, augmented, spec = (orc.make_frames(TV_B, TV_T, SIZE, seed=3), orc.make_frames(TV_B, TV_T, SIZE, seed=4),
                               orc.make_spectrogram(TV_B, FREQ, FRAMES))
    step = TwoViewTrainStep(_model(), loss_weight=LW, dedup_audio=dedup)
    kept = {}
    orig = step.engine.forward

    def spy(*a, **k):
        out, tape = orig(*a, **k)
        kept["tape"] = tape
        for t in tape["img"] + [ta["aud"] for ta in tape["aud"]]:
            t["want_dx"] = True
        return out, tape

    step.engine.forward = spy
    losses = step.step(frames.to(DEV), augmented.to(DEV), spec.to(DEV))
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all()
    tp = kept["tape"]
    assert (tp["aud"][0] is tp["aud"][1]) == dedup and tp["aud"][0]["rep"] == (TV_T if dedup else 1)
    grads = {n: g.detach().double().cpu() for n, g in step.flat.param_grad_views(step.grad).items()}
    grads["frames"], grads["augmented"] = (t["dx"].double().cpu() for t in tp["img"])
    auds = tp["aud"][:1] if dedup else tp["aud"]
    for k, ta in zip(("audio",) if dedup else ("audio1", "audio2"), auds):
        grads[k] = ta["aud"]["dx"].double().cpu()
    t = {"img": [_trunk_tape(x) for x in tp["img"]], "aud": [_trunk_tape(ta["aud"]) for ta in auds],
         "amax": [ta["amax"].cpu() for ta in auds]}
    for k in range(2):  # each view's head read that view's vision map
        assert torch.equal(t["img"][k]["blocks"][7]["out"], _nchw(tp["head"][k]["v"]))
    sd = orc.make_state(0)
    ref, yard = _forced(("twoview", dedup), t, lambda round_grads: orc.twoview_forced_grads(
        sd, frames, augmented, spec, t, loss_weight=LW, dedup_audio=dedup, round_grads=round_grads))
    _TWOVIEW[dedup] = (grads, ref, yard)
    return _TWOVIEW[dedup]


@pytest.mark.parametrize("dedup", [True, False], ids=["dedup", "nodedup"])
def test_twoview_step_forced_tape(dedup):
    """TwoViewTrainStep.step(frames, augmented, spec) at b = 2, t = 2: step.grad (the vision trunk's gradients summed
    over the two views, the audio trunk's over the views and -- de-duplicated -- the frames) and the input gradients
    of every trunk call against twoview_forced_grads fed the step's tapes (two vision tapes; one audio tape of the b
    spectrograms, or two of the folded b t rows), the loss twoview_losses' combined one with loss_weight 0.1.

    Measured on one MI355X (no tensor above the cap): de-duplicated, the yardstick's e_ref is 1.7e-3 to 1.49e-2,
    median 6.2e-3; largest error 0.67 of its bound (frames' gradient, e 3.3e-2), 0.60 (imgnet.conv1.weight), 0.54
    (augmented), 0.43 (spectrogram), 0.42 (audnet.conv1_a.weight) -- the stem's routing among bf16 ties -- and,
    everything else, 0.31 (imgnet.bn1.bias).  Undeduplicated: e_ref 1.7e-3 to 1.91e-2, median 6.6e-3; 0.67 (frames),
    0.65 and 0.43 (the two audio calls' inputs), 0.61 (imgnet.conv1.weight), everything else at most 0.37
    (audnet.bn1.bias)."""
    grads, ref, yard = _twoview(dedup)
    assert len(ref) == (123 if dedup else 124)
    _check(f"two-view step, dedup_audio={dedup}", grads, ref, yard)


def test_twoview_dedup_matches_undeduplicated():
    """The de-duplicated step's audio-trunk gradients against the undeduplicated step's, by rule_full with the
    undeduplicated oracle's yardstick carried over to them (its deviation from its own reference): one backward
    from the summed gan is the two per-view backwards' sum.  (The two runs' audio forwards differ in the BatchNorm
    statistics' rounding only.)

    Measured on one MI355X: the carried yardstick's e_ref is 2.4e-3 to 1.90e-2, median 7.0e-3; largest error 0.44 of
    its bound (audnet.bn1.bias, e 2.2e-2), 0.39 (audnet.conv1_a.weight), layer1.1's BN parameters 0.33, everything
    else below 0.30."""
    g_d, _, _ = _twoview(True)
    g_u, ref_u, yard_u = _twoview(False)
    names = [n for n in ref_u if n.startswith("audnet.")]
    assert len(names) == 60
    carried = {n: g_u[n] + (yard_u[n] - ref_u[n]) for n in names}
    _check("two-view step, de-duplicated vs undeduplicated audio trunk", g_d, g_u, carried, names=names)


def test_dp_mean_gradient_forced():
    """The data-parallel gradient -- the mean over the two shards of test_ddp_gpu._shards of each shard's
    local-negative gradient, each shard through its own forward and backward on one process -- as one vector over
    all 120 parameters against the mean of the two shards' forced oracles, by rule_full (yardstick: the mean of the
    two round_grads oracles), and closer to it than sep / 4, where sep >= 0.2 is the relative distance between the
    fp64 shard-mean gradient and the fp64 full-batch gradient (negatives from all four clips), from the oracle alone
    (test_step_forced_oracle_cpu.dp_separation).

    Measured on one MI355X: e 2.43e-2 against e_ref 1.06e-2 (0.49 of its bound); sep 1.155, so e is 0.084 of
    sep / 4."""
    from test_ddp_gpu import _shards
    from test_step_forced_oracle_cpu import dp_separation

    names = orc.trainable_names(orc.make_state(0))
    hip, ref, yard = [], [], []
    for r, shard in enumerate(_shards()):
        eng, tape, out, gflat, cot = _run(inputs=shard)
        g = _step_grads(eng, tape, gflat, False)
        rf, yd = _step_oracle(tape, cot, inputs=shard, tag=f"shard{r}")
        for dst, src in ((hip, g), (ref, rf), (yard, yd)):
            dst.append(torch.cat([src[n].double().flatten() for n in names]))
    hip, ref, yard = (sum(v) / len(v) for v in (hip, ref, yard))
    sep, _ = dp_separation()
    viol, e, e_ref, ratio = rule_full(hip, ref, yard)
    print(f"DP-mean gradient vs the shards' forced oracles: e {e:.3e} e_ref {e_ref:.3e} ({ratio:.2f} of its bound); "
          f"sep {sep:.3f}, e / (sep / 4) = {e / (sep / 4):.3f}")
    assert sep >= 0.2, sep
    assert not viol, viol
    assert e < sep / 4, (e, sep)
