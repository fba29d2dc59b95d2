"""FullModel.enable_folded_inference() / resnet3D.ResNet.enable_folded_inference(): the eval forward of the tube model
and of the R3D-18 trunk with every BatchNorm folded into its conv.

Parity is judged against the in-repo fp64 oracle (tube_oracle.fullmodel_forward(training=False); for the standalone
trunk r3d18_forward(training=False) + mean + fc) with the unfolded eval forward's own deviation from that oracle, on
the same inputs, as the yardstick: err_folded <= max(floor, 3 x err_unfolded) per output (the rule
of tests/test_folded_inference_gpu.py).  Floors: A 3e-2 absolute (test_tube_gpu.py's eval check), the head's logits
2e-2 absolute off the diagonal and 2e-3 relative on it (test_model_gpu.py); the standalone trunk's fc logits, which
have no diagonal, take test_model_gpu.py's relative floor 2e-3, of the largest reference logit.  Every BatchNorm's
running mean and variance, gamma and beta are moved by a seeded draw: a fresh model's (0, 1, 1, 0) would make the
fold trivial.  Tiny fixtures: video 2 x 4 x 32^2, spectrogram 65 x 76."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import avenet_oracle as orc
import tube_oracle as tor

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FLOORS = {"A_abs": 3e-2, "logits_off_abs": 2e-2, "logits_diag_rel": 2e-3, "fc_rel": 2e-3}


def _state(seed=0):
    """make_tube_state with every BatchNorm's gamma, beta, running mean and running variance moved (seeded)."""
    sd = tor.make_tube_state(0)
    g = torch.Generator().manual_seed(2000 + seed)
    for k in sd:
        if ".bn" in k or "downsample.1" in k:
            if k.endswith(".weight"):
                sd[k] = sd[k] * (1 + 0.2 * torch.randn(sd[k].shape, generator=g))
            elif k.endswith(".bias"):
                sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
            elif k.endswith("running_mean"):
                sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
            elif k.endswith("running_var"):
                sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g)
    return sd


def _inputs():
    return tor.make_video(2, 4, 32), orc.make_spectrogram(2, 65, 76)


def _fullmodel(sd, folded):
    from avt_amd.model import FullModel

    m = FullModel(orc.Args())
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    return m.enable_folded_inference() if folded else m


def _standalone(sd, max_pool, folded, backward=None):
    from avt_amd.resnet3D import generate_model

    net = generate_model(18, no_max_pool=not max_pool, n_classes=1039)
    net.load_state_dict({k[len("vidnet."):]: v for k, v in sd.items() if k.startswith("vidnet.")})
    if backward is not None:
        net.enable_backward(**backward)
    net = net.to(DEV).eval()
    return net.enable_folded_inference() if folded else net


def _fwd(m, *inputs):
    with torch.no_grad():
        out = m(*[x.to(DEV) for x in inputs])
    torch.cuda.synchronize()
    return [o.detach().cpu() for o in (out if isinstance(out, tuple) else (out,))]


def _sd64(sd):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


_ORACLE = {}


def _oracle_full(sd, spec, video, key):
    if key not in _ORACLE:
        with torch.no_grad():
            A, logits = tor.fullmodel_forward(_sd64(sd), tor.repeat_spectrogram(spec, video.shape[2]).double(),
                                              video.double(), training=False)
        _ORACLE[key] = (A.double(), logits.double())
    return _ORACLE[key]


def _devs_full(out, ref):
    A, logits = (o.double().numpy() for o in out)
    rA, rl = (r.numpy() for r in ref)
    diag = np.eye(A.shape[0], logits.shape[1], k=1, dtype=bool)
    return {"A_abs": np.abs(A - rA).max(),
            "logits_off_abs": np.abs(logits[~diag] - rl[~diag]).max(),
            "logits_diag_rel": (np.abs(logits[diag] - rl[diag]) / np.abs(rl[diag])).max()}


def _assert_parity(tag, ef, eu):
    for k in ef:
        print(f"{tag}: {k}: folded {ef[k]:.3e} unfolded {eu[k]:.3e} tol {max(FLOORS[k], 3 * eu[k]):.3e}")
    for k in ef:
        assert ef[k] <= max(FLOORS[k], 3 * eu[k]), (tag, k, ef[k], eu[k])


@pytest.mark.parametrize("per_clip", [False, True])
def test_fullmodel_parity_with_oracle(per_clip):
    """Both audio conventions ([b*t,1,F,T] folded repeat, [b,1,F,T] per clip): folded against the fp64 oracle, the
    unfolded eval forward of the same build as the yardstick.  Measured on one MI355X: see DESIGN 6l."""
    sd = _state()
    video, spec = _inputs()
    audio = spec if per_clip else tor.repeat_spectrogram(spec, 4)
    ref = _oracle_full(sd, spec, video, "state0")
    plain, fold = _fullmodel(sd, False), _fullmodel(sd, True)
    out_u, out_f = _fwd(plain, audio, video), _fwd(fold, audio, video)
    for a, b in zip(out_u, out_f):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.isfinite(b).all()
    assert not all(torch.equal(a, b) for a, b in zip(out_u, out_f))  # the folded path ran
    assert fold.engine().fold_launches == 2 and plain.engine().fold_launches == 0
    _assert_parity(f"FullModel per_clip={per_clip}", _devs_full(out_f, ref), _devs_full(out_u, ref))


@pytest.mark.parametrize("max_pool", [True, False])
def test_standalone_trunk_parity_with_oracle(max_pool):
    """A standalone generate_model(18, ...) with and without the stem max-pool: the fc logits, same rule."""
    sd = _state()
    video, _ = _inputs()
    with torch.no_grad():
        s64 = _sd64(sd)
        feat = tor.r3d18_forward(s64, "vidnet.", video.double(), training=False, max_pool=max_pool)
        ref = F.linear(feat.mean(dim=(2, 3, 4)), s64["vidnet.fc.weight"], s64["vidnet.fc.bias"])
    plain, fold = _standalone(sd, max_pool, False), _standalone(sd, max_pool, True)
    (lu,), (lf,) = _fwd(plain, video), _fwd(fold, video)
    assert lf.shape == lu.shape == (2, 1039) and torch.isfinite(lf).all()
    assert not torch.equal(lu, lf)  # the folded path ran
    assert fold._avt_engine.fold_launches == 1 and plain._avt_engine.folds3d is None
    scale = ref.abs().max().item()
    ef = {"fc_rel": (lf.double() - ref).abs().max().item() / scale}
    eu = {"fc_rel": (lu.double() - ref).abs().max().item() / scale}
    _assert_parity(f"standalone max_pool={max_pool}", ef, eu)


@pytest.mark.parametrize("max_pool", [False, True])
def test_launch_count(max_pool):
    """A folded video-trunk forward: exactly 1 im2col + 20 conv launches (+ 1 max-pool); no avt_bn_apply, no
    avt_bn_finalize*, no avt_pack_conv3d*, no torch BN arithmetic -- counted as tools/infer_bench.py counts."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        from infer_bench import count_launches
    finally:
        sys.path.pop(0)
    video, _ = _inputs()
    net = _standalone(_state(), max_pool, True)
    vd = video.to(DEV)
    _fwd(net, video)  # the first folded forward folds
    c = count_launches(net, vd)
    print(dict(c))
    convs = c["avt_conv3d_fwd_bias"] + c["avt_conv2d_fwd_bias"]
    assert c["avt_video_stem_im2col"] == 1 and convs == 20 and c["avt_conv3d_fwd_bias"] == 17
    assert c["avt_maxpool3d_fwd"] == int(max_pool)
    assert sum(c.values()) == 21 + int(max_pool)
    assert not any(k.startswith(("avt_bn_apply", "avt_bn_finalize", "avt_pack_conv3d", "torch BN")) for k in c)
    # and the unfolded forward of the same trunk, for the record: its BN passes and packs are what the fold removes
    u = count_launches(_standalone(_state(), max_pool, False), vd)
    assert u["avt_bn_apply"] == 17 and u["avt_pack_conv3d_weights_batched"] == 1


def _sgd_audnet(m, spec, video):
    opt = torch.optim.SGD(m.audnet.parameters(), lr=1e-2)
    torch.manual_seed(7)
    for p in m.audnet.parameters():
        p.grad = torch.randn_like(p)
    opt.step()
    m.zero_grad()


def _load_other(m, spec, video):
    m.load_state_dict(_state(1))


def _scale_var(m, spec, video):
    with torch.no_grad():
        m.vidnet.bn1.running_var.mul_(4)


def _train_forward(m, spec, video):
    m.train()
    with torch.no_grad():
        m(spec.to(DEV), video.to(DEV))
    m.eval()


@pytest.mark.parametrize("change", [_load_other, _sgd_audnet, _scale_var, _train_forward])
def test_staleness(change):
    """A folded forward, a change of the parameters or buffers, a folded forward: exactly one refold per trunk, the
    output moved, bitwise that of a fresh folded model built from the updated state (the fold is deterministic), and
    within the parity bound of the fp64 oracle on that state."""
    sd = _state()
    video, spec = _inputs()
    m = _fullmodel(sd, True)
    before = _fwd(m, spec, video)
    n0 = m.engine().fold_launches
    assert n0 == 2
    change(m, spec, video)
    after = _fwd(m, spec, video)
    assert m.engine().fold_launches == n0 + 2
    new_sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    fresh = _fwd(_fullmodel(new_sd, True), spec, video)
    for x, y in zip(after, fresh):
        assert torch.equal(x, y)
    assert not torch.equal(before[0], after[0])
    ref = _oracle_full(new_sd, spec, video, change.__name__)
    _assert_parity(change.__name__, _devs_full(after, ref),
                   _devs_full(_fwd(_fullmodel(new_sd, False), spec, video), ref))


def test_staleness_sgd_on_a_trainable_standalone_trunk():
    """torch.optim.SGD on a standalone enable_backward() trunk: a train step (forward, backward, step) is followed by
    exactly one refold, and the folded logits are bitwise a fresh folded trunk's on the updated state."""
    video, _ = _inputs()
    vd = video.to(DEV)
    net = _standalone(_state(), False, True, backward={})
    opt = torch.optim.SGD(net.parameters(), lr=1e-2)

    def step():
        net.train()
        opt.zero_grad()
        F.cross_entropy(net(vd), torch.tensor([7, 911], device=DEV)).backward()
        opt.step()
        net.eval()

    step()  # the trainable engine exists from here on
    before = _fwd(net, video)[0]
    eng = net._avt_engine
    assert eng.fold_launches == 1
    assert torch.equal(_fwd(net, video)[0], before) and eng.fold_launches == 1
    step()
    after = _fwd(net, video)[0]
    assert net._avt_engine is eng and eng.fold_launches == 2
    assert not torch.equal(before, after)
    new_sd = {"vidnet." + k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    fresh = _fwd(_standalone(new_sd, False, True), video)[0]
    assert torch.equal(after, fresh)


def test_no_needless_refold_and_invalidate():
    """Two folded forwards with nothing in between: bitwise equal, no fold launch; invalidate_folded() forces one per
    trunk; model.vidnet(video) and model.audnet(x) follow the model's flag on engines of their own."""
    video, spec = _inputs()
    m = _fullmodel(_state(), True)
    first = _fwd(m, spec, video)
    assert m.engine().fold_launches == 2
    second = _fwd(m, spec, video)
    assert m.engine().fold_launches == 2
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    assert m.invalidate_folded() is m and m.enable_folded_inference() is m
    _fwd(m, spec, video)
    assert m.engine().fold_launches == 4
    plain = _fullmodel(_state(), False)
    for name, x in (("vidnet", video), ("audnet", spec)):
        f, u = _fwd(getattr(m, name), x)[0], _fwd(getattr(plain, name), x)[0]
        assert getattr(m, name)._avt_engine.fold_launches == 1 and getattr(plain, name)._avt_engine.fold_launches == 0
        assert f.shape == u.shape and not torch.equal(f, u)
        d = (f.double() - u.double()).abs().max().item() / u.abs().max().item()
        print(f"model.{name}(x): folded - unfolded = {d:.3e} of max |unfolded|")
        assert d <= 2 * 3e-2  # each path within 3e-2 of the exact output (test_tube_gpu.py's standalone-trunk bound)
        _fwd(getattr(m, name), x)
        assert getattr(m, name)._avt_engine.fold_launches == 1


def test_non_interference():
    """Without the opt-in no fold operand is allocated; with it a train-mode forward and backward are bitwise those
    of a model without it, and the state_dict keys are unchanged."""
    sd = _state()
    video, spec = _inputs()
    runs, keys = [], []
    for folded in (False, True):
        m = _fullmodel(sd, folded)
        out_eval = _fwd(m, spec, video)
        if not folded:
            assert m.engine().folds is None and m.engine().folds3d is None and m.engine().fold_launches == 0
        keys.append(list(m.state_dict()))
        assert sorted(keys[-1]) == sorted(sd)
        m.train()
        A, logits = m(spec.to(DEV), video.to(DEV))
        loss = F.cross_entropy(logits, torch.zeros(8, dtype=torch.long, device=DEV))
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        runs.append((A.detach().clone(), logits.detach().clone(), grads,
                     {k: v.clone() for k, v in m.state_dict().items()}, out_eval))
    (A0, l0, g0, s0, e0), (A1, l1, g1, s1, e1) = runs
    assert torch.equal(A0, A1) and torch.equal(l0, l1) and sorted(g0) == sorted(g1) and g0
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    for n in s0:
        assert torch.equal(s0[n], s1[n]), n
    assert keys[0] == keys[1]
    assert not torch.equal(e0[0], e1[0])  # while the eval forwards did take different paths


def test_eval_grad_of_a_standalone_trunk_unchanged():
    """enable_backward(eval_grad=True) on a standalone trunk, with and without the folded opt-in: a grad-mode eval
    call takes the autograd path, bitwise the same logits and gradients; under no_grad the opted-in one folds."""
    sd = _state()
    video, _ = _inputs()
    vd = video.to(DEV)
    runs = []
    for folded in (False, True):
        net = _standalone(sd, True, folded, backward=dict(eval_grad=True))
        if folded:
            _fwd(net, video)  # a fold exists before the grad-mode call
            assert net._avt_engine.fold_launches == 1
        logits = net(vd)
        F.cross_entropy(logits, torch.tensor([7, 911], device=DEV)).backward()
        torch.cuda.synchronize()
        runs.append((logits.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters()}))
    (l0, g0), (l1, g1) = runs
    assert torch.equal(l0, l1) and sorted(g0) == sorted(g1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
