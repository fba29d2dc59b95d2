"""FullModel.enable_video_backward(): the tube step with the video trunk trained end to end -- the
drop-in autograd path and train.HardWayTrainStep (eager, captured, the data-parallel schedule), both audio forms.

Geometry: b = 2 clips of t = 1 (the T = 1 Conv3d plans) or t = 3 (both clip ends and an interior frame) frames of
64 x 64 -- layer4 map 4 x 4, so the head has B = b t rows of P = 16 positions -- and 65 x 76 spectrograms, folded
[(b t),1,F,T] at t = 1 and one per clip (rep = t) at t = 3.

The backward is held against tests/tube_e2e_oracle.py's forced-tape fp64 oracle (both trunks forced onto the step's own
tapes) by gradcheck.rule_full with the bf16-storage yardstick and the forced tests' cap, as
test_step_backward_forced_gpu.py and test_r3d_backward_forced_gpu.py hold the same links; the one new link, the head's
gv into layer4, also on its own against fp64 autograd of the head at the saved (v, an) with test_hardway_head's bound
for the vision gradient (max error < 1e-2 of the largest value).  tests/test_tube_e2e_oracle_cpu.py shows that the
oracle is sound and that the comparators used here flag three wiring faults.  Everything else is bitwise: the opt-in
against the detached model, the ways of issuing the same launches, Adam's scope, the data-parallel schedule, the
checkpoint round trip."""
import ctypes

import pytest
import torch
import torch.distributed as dist

import avenet_oracle as orc
import tube_e2e_oracle as e2e
import tube_oracle as tor

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B_CLIPS, SIZE, FREQ, FRAMES = 2, 64, 65, 76
CASES = [(1, False), (3, True)]  # (t, one spectrogram per clip)
IDS = ["t1-folded", "t3-perclip"]
LR, WD = 1e-4, 1e-4
_RUNS = {}


def _model(optin=True):
    from avt_amd.model import FullModel

    m = FullModel(orc.Args())
    m.load_state_dict(tor.make_tube_state(0))
    m = m.to(DEV).train()
    return m.enable_video_backward() if optin else m


def _inputs(t, per_clip):
    """(audio as the step takes it, video), on the CPU."""
    spec = orc.make_spectrogram(B_CLIPS, FREQ, FRAMES)
    return (spec if per_clip else tor.repeat_spectrogram(spec, t)), tor.make_video(B_CLIPS, t, SIZE)


def _ce(logits):
    return torch.nn.CrossEntropyLoss()(logits, torch.zeros(logits.shape[0], dtype=torch.long, device=logits.device))


def _state(m, step=None):
    """Clones of everything a step changes: weights, running statistics, batch counters (, gradient, Adam moments)."""
    f = m._flat
    out = {"flat": f.flat.clone(), "bflat": f.bflat.clone(), "nbt": f.nbt.clone()}
    if step is not None:
        out.update(grad=step.grad.clone(), m1=step.opt.exp_avg.clone(), m2=step.opt.exp_avg_sq.clone())
    return out


def _assert_same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


def test_opt_in_fills_vidnet_grads():
    """Fails without the feature: enable_video_backward() exists, is idempotent and returns the model, keeps the
    state_dict (keys, shapes, values), and after it loss.backward() on the drop-in path fills .grad for conv1, bn1 and
    layer1..4 of vidnet (and the audio trunk's parameters); vidnet.fc's .grad, and the unused audnet stems' and fc's,
    stay None."""
    m = _model(optin=False)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.enable_video_backward() is m
    flat = m._flat
    assert m.enable_video_backward() is m and m._flat is flat  # idempotent: nothing is rebuilt
    after = m.state_dict()
    assert list(after) == list(before)
    for k in before:
        assert after[k].shape == before[k].shape and torch.equal(after[k], before[k]), k
    audio, video = _inputs(3, True)
    A, logits = m(audio.to(DEV), video.to(DEV))
    _ce(logits).backward()
    torch.cuda.synchronize()
    params = dict(m.named_parameters())
    for n in e2e.e2e_names():
        g = params[n].grad
        assert g is not None and g.shape == params[n].shape and torch.isfinite(g).all() and g.abs().max() > 0, n
    for n in e2e.untrained_names(tor.make_tube_state(0)):
        assert params[n].grad is None, n
    assert len([n for n in params if params[n].grad is not None]) == 120


def _nchw(t):
    return t.permute(0, 3, 1, 2).float().cpu()


def _ncdhw(t, b):
    n, h, w, c = t.shape
    return t.view(b, n // b, h, w, c).permute(0, 4, 1, 2, 3).float().cpu()


@pytest.mark.parametrize("t,per_clip", CASES, ids=IDS)
def test_backward_against_forced_oracle(t, per_clip, monkeypatch):
    """TubeEngine.forward(..., with_ce=True) then backward(tape, dlogits, gflat[, dA]) -- CE alone at t = 1, CE and a
    dense standard-normal cotangent of the returned A at t = 3 -- against tube_e2e_forced_grads fed the step's own
    tapes: all 60 vidnet and 60 audnet gradients by gradcheck.rule_full, the yardstick within the forced tests' cap
    per trunk.  The head's gv on its own: fp64 autograd of the head at the saved (v, an), max error < 1e-2 of the
    largest value (test_hardway_head's bound for the vision gradient).

    Measured on one MI355X: the head's gv 3.0e-3 (t = 1) and 3.3e-3 (t = 3) of the largest value; the largest error
    of the 120 gradients 0.35 (t = 1) and 0.33 (t = 3) of its bound, both on audnet.conv1_a.weight (the stem's routing
    among bf16 ties, as in test_step_backward_forced_gpu.py)."""
    import avt_amd.trunk

    monkeypatch.setattr(avt_amd.trunk, "FUSE_BN_BWD", False)
    audio, video = _inputs(t, per_clip)
    B = B_CLIPS * t
    cot_A = torch.randn(B, 1, 4, 4, generator=torch.Generator().manual_seed(17)) if t == 3 else None
    eng = _model().engine()
    assert eng.video_backward and [tr.prefix for tr in eng.backward_order()] == ["vidnet.", "audnet."]
    seen = {}
    orig = eng.head_backward

    def spy(*a, **k):
        seen["gv"], seen["gan"] = orig(*a, **k)
        return seen["gv"], seen["gan"]

    monkeypatch.setattr(eng, "head_backward", spy)
    out, tape = eng.forward(audio.to(DEV), video.to(DEV), True, with_ce=True)
    assert tuple(out["v"].shape) == (B, 4, 4, 512) and tape["rep"] == (t if per_clip else 1)
    gflat = torch.zeros(eng.flat.n_train, device=DEV, dtype=torch.float32)
    eng.backward(tape, out["dlogits"], gflat, dA=None if cot_A is None else cot_A.to(DEV))
    torch.cuda.synchronize()
    assert eng.store.grads is None and torch.isfinite(gflat).all()
    grads = {n: g.detach().double().cpu() for n, g in eng.flat.param_grad_views(gflat).items()}
    assert sorted(grads) == sorted(e2e.e2e_names())
    # the one new link: the head's gv
    gv_ref = e2e.head_gv_reference(tape["v"].float().cpu(), tape["an"].cpu(), cot_A)
    gv = seen["gv"].float().cpu().double()
    err = ((gv - gv_ref).abs().max() / gv_ref.abs().max()).item()
    print(f"t={t}: head gv max error {err:.3e} of the largest value (bound 1e-2)")
    assert tuple(gv.shape) == tuple(gv_ref.shape) and err < 1e-2, err
    # the whole backward on the step's own tapes
    tv, ta = tape["vid"], tape["aud"]
    vt = {"c0": _ncdhw(tv["c0"], B_CLIPS), "h0": _ncdhw(tv["h0"], B_CLIPS), "blocks": []}
    for tb in tv["blocks"]:
        vt["blocks"].append({k: _ncdhw(tb[k], B_CLIPS) for k in ("c1", "h1", "c2", "cd", "out") if k in tb})
    at = {"c0": _nchw(ta["c0"]), "p0": _nchw(ta["blocks"][0]["x"]), "blocks": []}
    for tb in ta["blocks"]:
        at["blocks"].append({k: _nchw(tb[k]) for k in ("c1", "h1", "c2", "cd", "out") if k in tb})
    assert torch.equal(vt["blocks"][7]["out"], _ncdhw(tape["v"], B_CLIPS))  # the head read the tapes' maps
    assert torch.equal(at["blocks"][7]["out"], _nchw(tape["a"]))
    forced = {"vid": vt, "aud": at, "amax": tape["amax"].cpu()}
    sd = tor.make_tube_state(0)
    ref = e2e.tube_e2e_forced_grads(sd, audio, video, forced, cot_A)
    yard = e2e.tube_e2e_forced_grads(sd, audio, video, forced, cot_A, round_grads=True)
    assert len(ref) == 120
    bad, worst = e2e.grad_violations(grads, ref, yard)
    print(f"t={t} per_clip={per_clip}: largest error {worst[1]:.2f} of its bound ({worst[0]})")
    for x in bad:
        print("OUT OF BOUND", x)
    assert not bad, bad


@pytest.mark.parametrize("t,per_clip", CASES, ids=IDS)
def test_opt_in_changes_nothing_else(t, per_clip):
    """Identical weights and inputs, a model with the opt-in against one without (drop-in path): loss, logits, A, the
    BN running statistics and batch counters, and every audnet gradient bitwise equal (the head's gan does not depend
    on whether gv is asked for: dA0 and its GEMM are the same launches); the detached model's vidnet gets no
    gradient."""
    audio, video = _inputs(t, per_clip)
    res = []
    for optin in (False, True):
        m = _model(optin)
        A, logits = m(audio.to(DEV), video.to(DEV))
        loss = _ce(logits)
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        res.append((loss.detach(), logits.detach(), A.detach(), _state(m), grads))
    (l0, lg0, A0, s0, g0), (l1, lg1, A1, s1, g1) = res
    assert torch.equal(l0, l1) and torch.equal(lg0, lg1) and torch.equal(A0, A1)
    _assert_same({k: s0[k] for k in ("bflat", "nbt")}, {k: s1[k] for k in ("bflat", "nbt")}, "opt-in vs detached")
    assert sorted(g0) == sorted(tor.trainable_names_tube())
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    assert sorted(g1) == sorted(e2e.e2e_names())


def _steps(t, per_clip, mode, n=4):
    """n HardWayTrainStep steps of a fresh opted-in model: mode "eager", "serial" (one stream), "graph" / "graph2"
    (one eager step, capture, replays).  Returns (losses, the state after the last step).  Once per (case, mode)."""
    key = (t, per_clip, mode, n)
    if key not in _RUNS:
        from avt_amd.train import HardWayTrainStep

        audio, video = (x.to(DEV) for x in _inputs(t, per_clip))
        m = _model()
        step = HardWayTrainStep(m, lr=LR, weight_decay=WD)
        step.engine.concurrent = mode != "serial"
        losses = []
        for i in range(n):
            if i == 1 and mode.startswith("graph"):
                step.capture(audio.clone(), video.clone())
            losses.append(step.step(audio, video).clone())
        torch.cuda.synchronize()
        assert (step._graph is not None) == mode.startswith("graph")
        assert all(torch.isfinite(x) for x in losses)
        _RUNS[key] = (torch.stack(losses).cpu(), {k: v.cpu() for k, v in _state(m, step).items()})
    return _RUNS[key]


@pytest.mark.parametrize("t,per_clip", CASES, ids=IDS)
def test_ways_of_issuing_agree_bitwise(t, per_clip):
    """HardWayTrainStep eager (two streams), eager on one stream (engine.concurrent = False), and captured after one
    eager step then replayed three times, twice over (determinism): losses of all four steps, the last flat gradient,
    the weights and moments after Adam and the running statistics bitwise equal.  The drop-in autograd path on the
    same weights, its logits' cotangent taken from avt_hardway_ce as the fused step takes it: the first step's loss
    and flat gradient bitwise equal to the fused step's."""
    from avt_amd._lib import call
    from avt_amd.train import HardWayTrainStep

    le, se = _steps(t, per_clip, "eager")
    for mode in ("serial", "graph", "graph2"):
        lm, sm = _steps(t, per_clip, mode)
        assert torch.equal(le, lm), (mode, le, lm)
        _assert_same(se, sm, f"eager vs {mode}")
    # the drop-in path's first step against the fused step's
    audio, video = (x.to(DEV) for x in _inputs(t, per_clip))
    m1 = _model()
    s1 = HardWayTrainStep(m1, lr=LR, weight_decay=WD)
    loss1 = s1.step(audio, video).clone()
    m2 = _model()
    A, logits = m2(audio, video)
    Bn, L = logits.shape
    loss2 = torch.empty((), device=DEV)
    dl = torch.empty(Bn, L, device=DEV)
    lg = logits.detach().contiguous()
    call("avt_hardway_ce", ctypes.c_void_p(lg.data_ptr()), Bn, L, 1.0, ctypes.c_void_p(loss2.data_ptr()),
         ctypes.c_void_p(dl.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    logits.backward(dl)
    torch.cuda.synchronize()
    assert torch.equal(loss1, loss2) and torch.equal(loss1.cpu(), le[0])
    views = m1._flat.param_grad_views(s1.grad)
    params = dict(m2.named_parameters())
    for n in e2e.e2e_names():
        assert torch.equal(params[n].grad, views[n]), n
    _assert_same({k: v for k, v in _state(m1).items() if k != "flat"},
                 {k: v for k, v in _state(m2).items() if k != "flat"}, "fused vs drop-in running statistics")


@pytest.mark.parametrize("t,per_clip", CASES, ids=IDS)
def test_adam_scope(t, per_clip):
    """After the eager steps with weight decay on: vidnet.fc.* and the never-trained audnet parameters bit-identical
    to their initial values, every trained parameter (vidnet's 60 included) moved."""
    from avt_amd.train import HardWayTrainStep

    audio, video = (x.to(DEV) for x in _inputs(t, per_clip))
    m = _model()
    step = HardWayTrainStep(m, lr=LR, weight_decay=WD)
    for _ in range(3):
        step.step(audio, video)
    torch.cuda.synchronize()
    before = tor.make_tube_state(0)
    after = {k: v.cpu() for k, v in m.state_dict().items()}
    bad = e2e.adam_scope_violations(before, after, e2e.e2e_names(), e2e.untrained_names(before))
    assert not bad, bad
    assert int(step.opt.t) == 3


class _Work:
    def __init__(self, ev):
        self.ev = ev

    def wait(self):
        torch.cuda.current_stream().wait_event(self.ev)
        return True


def test_data_parallel_schedule(monkeypatch):
    """One process, the world > 1 overlap schedule forced (step.world, step.overlap = 2, True, as
    test_side_stream_adam_ordering_without_host_sync) with an all-reduce that doubles its bucket on a stream of its own
    (two ranks with the same shard): the weights after every step -- eager, then two segment graphs -- equal Adam on
    (g + g) / 2 of the one-rank gradient, bitwise, with the vidnet buckets among the four."""
    from avt_amd.train import HardWayTrainStep

    comm = torch.cuda.Stream(device=DEV)
    reduced = []

    def fake_all_reduce(t, op=None, group=None, async_op=False):
        reduced.append(t.numel())
        comm.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(comm):
            t.mul_(2.0)
            ev = torch.cuda.Event()
            ev.record(comm)
        w = _Work(ev)
        if async_op:
            return w
        w.wait()

    monkeypatch.setattr(dist, "all_reduce", fake_all_reduce)
    audio, video = (x.to(DEV) for x in _inputs(3, True))
    m = _model()
    step = HardWayTrainStep(m, lr=LR, weight_decay=WD)
    step.world, step.overlap = 2, True
    assert list(step.buckets) == ["vidnet.hi", "vidnet.lo", "audnet.hi", "audnet.lo"]
    spans = sorted(step.buckets.values())
    assert spans[0][0] == 0 and spans[-1][1] == m._flat.n_train
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))  # the four buckets tile the trainable segment
    ref_m = _model()
    ref = HardWayTrainStep(ref_m, lr=LR, weight_decay=WD)
    for i in range(4):
        if i == 2:
            step.capture(audio.clone(), video.clone())
        step.step(audio, video)
        snap = m._flat.flat.clone()  # on the current stream right after step(): no host sync
        ref._fwd_bwd(audio, video)
        ref.opt.step(ref.grad * 2.0, grad_scale=0.5)
        torch.cuda.synchronize()
        assert torch.equal(snap, ref_m._flat.flat), f"step {i}: not Adam on g / 2 of the summed gradient"
        assert torch.equal(m._flat.bflat, ref_m._flat.bflat)
    assert step._seg_graphs is not None and len(step._seg_graphs) == 2
    assert sum(reduced[:4]) == m._flat.n_train  # one step's collectives cover every trainable element once


def test_checkpoint_round_trip():
    """Two steps, save, load into a fresh opted-in model and its step, one more step: weights, running statistics,
    counters, gradient and Adam moments bitwise equal to three uninterrupted steps.  The torch-Adam layout of the
    state: entries for exactly the 120 parameters that receive gradients, at their positions in model.parameters()
    (none for vidnet.fc.*, the unused audnet stems and fc), loadable by torch.optim.Adam over model.parameters() and
    back, bitwise."""
    from avt_amd.checkpoint import flat_adam_state_dict, load_checkpoint, load_flat_adam_state_dict, save_checkpoint
    from avt_amd.train import HardWayTrainStep

    audio, video = (x.to(DEV) for x in _inputs(3, True))
    _, whole = _steps(3, True, "eager", n=3)
    m1 = _model()
    s1 = HardWayTrainStep(m1, lr=LR, weight_decay=WD)
    for _ in range(2):
        s1.step(audio, video)
    ck = save_checkpoint(None, 7, m1, s1)
    ck["model_state_dict"] = {k: v.detach().clone().cpu() for k, v in ck["model_state_dict"].items()}
    m2 = _model()
    s2 = HardWayTrainStep(m2, lr=LR, weight_decay=WD)
    assert load_checkpoint(ck, m2, s2) == 7
    s2.step(audio, video)
    torch.cuda.synchronize()
    _assert_same(whole, {k: v.cpu() for k, v in _state(m2, s2).items()}, "resumed vs uninterrupted")
    # the torch-Adam layout
    osd = flat_adam_state_dict(m2, s2.opt)
    names = [n for n, _ in m2.named_parameters()]
    assert sorted(names[i] for i in osd["state"]) == sorted(e2e.e2e_names())
    assert osd["state"][names.index("vidnet.conv1.weight")]["exp_avg"].shape == (64, 3, 7, 7, 7)
    topt = torch.optim.Adam(m2.parameters(), lr=LR, weight_decay=WD)
    topt.load_state_dict(osd)
    m3 = _model()
    s3 = HardWayTrainStep(m3, lr=LR, weight_decay=WD)
    load_flat_adam_state_dict(m3, s3.opt, topt.state_dict())
    assert torch.equal(s3.opt.exp_avg, s2.opt.exp_avg) and torch.equal(s3.opt.exp_avg_sq, s2.opt.exp_avg_sq)
    assert int(s3.opt.t) == int(s2.opt.t) == 3


def test_refusals():
    """What stays refused with the opt-in: an eval-mode model computes no gradient (its outputs carry no graph, so
    backward raises), a video that requires grad raises, vidnet.enable_backward() on the adopted trunk raises and
    points to FullModel.enable_video_backward(), and the trunk called on its own in grad mode stays forward-only."""
    audio, video = (x.to(DEV) for x in _inputs(1, False))
    m = _model()
    with pytest.raises(RuntimeError, match="FullModel.enable_video_backward"):
        m.vidnet.enable_backward()
    with pytest.raises(NotImplementedError, match="video"):
        m(audio, video.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        m.vidnet(video)
    m.eval()
    A, logits = m(audio, video)
    assert not logits.requires_grad and not A.requires_grad
    with pytest.raises(RuntimeError):
        _ce(logits).backward()
    assert all(p.grad is None for p in m.parameters())
