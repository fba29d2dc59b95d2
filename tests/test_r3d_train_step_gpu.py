"""train.R3DTrainStep -- the fused fine-tuning step of a stand-alone R3D-18 -- on the smallest clip
test_r3d_backward_end_to_end runs (make_video(2, 4, 64)), n_classes = 7, with and without the stem max-pool:

* composition: one eager step leaves the flat gradient, the parameters, the momentum buffers and the BatchNorm
  buffers bitwise equal to the same libavt calls issued by hand (R3DTrunk.forward(tape=True), the five head entry
  points, R3DTrunk.backward, one avt_sgd_step_dev), and two runs from the same state are bitwise equal;
* capture: three replayed steps equal three eager steps bitwise (loss, gradient, parameters, momentum buffers, running
  statistics, num_batches_tracked), with a FlatMultiStepLR change between the replays, and a batch of another shape
  runs eagerly;
* against the parent's path: per-parameter gradients of the fused step and of F.cross_entropy(net(video), labels)
  .backward() on a deep copy, both against the fp64 oracle (tube_oracle.r3d18_forward + fc + F.cross_entropy):
  the fused error vector <= max(5e-2, 3 x the autograd path's), the loss <= max(1e-4, 3 x the autograd path's)
  (test_fullsize_gpu._check_grads' rule with the parent's path as the yardstick);
* refusals."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import tube_oracle as tor  # noqa: E402
from avt_amd._lib import call, query  # noqa: E402
from avt_amd.optim import FlatMultiStepLR, FlatSGD  # noqa: E402
from avt_amd.resnet3D import generate_model  # noqa: E402
from avt_amd.train import R3DTrainStep  # noqa: E402
from avt_amd.tube import R3DEngine  # noqa: E402

DEV = torch.device("cuda")
N_CLS = 7
LABELS = torch.tensor([3, 6])
HYPER = dict(lr=0.01, momentum=0.9, weight_decay=1e-3)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _state():
    """make_tube_state's vidnet with a 7-class fc (U(+-1/sqrt(512)), seeded)"""
    sd = tor.make_tube_state(0)
    g = torch.Generator().manual_seed(17)
    bound = 1.0 / 512 ** 0.5
    sd["vidnet.fc.weight"] = (torch.rand(N_CLS, 512, generator=g) * 2 - 1) * bound
    sd["vidnet.fc.bias"] = (torch.rand(N_CLS, generator=g) * 2 - 1) * bound
    return sd


def _net(max_pool, sd=None):
    sd = _state() if sd is None else sd
    net = generate_model(18, no_max_pool=not max_pool, n_classes=N_CLS)
    net.load_state_dict({k[len("vidnet."):]: v for k, v in sd.items() if k.startswith("vidnet.")})
    return net.to(DEV).train()


def _inputs():
    return tor.make_video(2, 4, 64).to(DEV), LABELS.to(DEV)


def _snapshot(step):
    torch.cuda.synchronize()
    f = step.flat
    return dict(grad=step.grad.clone(), flat=f.flat.clone(), bflat=f.bflat.clone(), nbt=f.nbt.clone(),
                buf=step.opt.momentum_buffer.clone(), t=step.opt.t)


def _assert_same(a, b, what):
    for k in a:
        if k == "t":
            assert a[k] == b[k], (what, k)
        else:
            assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                               b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), (what, k)


def _by_hand(net, video, labels):
    """the step's launches issued one by one on a second trunk; returns (loss, correct, snapshot-like dict)"""
    flat = net.enable_backward()._flat_store()
    eng = R3DEngine(flat, "", max_pool=not net.no_max_pool, with_backward=True)
    opt = FlatSGD(flat, **HYPER)
    eng.pack_weights()
    flat.nbt += 1
    v, tape = eng.vid.forward(video, eng.store, True, tape=True)
    b, C = video.shape[0], v.shape[-1]
    per = v.numel() // (b * C)
    w, bias = flat.raw("fc.weight"), flat.raw("fc.bias")
    wsb = int(query("avt_cls_pool_ws_bytes", b, per, C))
    ws = torch.empty(wsb, device=DEV, dtype=torch.uint8)
    feat = torch.empty(b, C, device=DEV)
    call("avt_cls_pool_fwd", P(v), P(feat), b, per, C, P(ws), wsb, S())
    logits = torch.empty(b, N_CLS, device=DEV)
    call("avt_cls_fc_fwd", P(feat), P(w), P(bias), P(logits), b, C, N_CLS, S())
    loss, dl = torch.empty(1, device=DEV), torch.empty_like(logits)
    correct = torch.empty(1, device=DEV, dtype=torch.int32)
    call("avt_softmax_ce", P(logits), P(labels), b, N_CLS, 1.0, P(loss), P(dl), P(correct), S())
    gflat = torch.zeros(flat.n_train, device=DEV)
    grads = flat.grad_views(gflat)
    gfeat = torch.empty_like(feat)
    call("avt_cls_fc_bwd", P(dl), P(feat), P(w), P(grads["fc.weight"]), P(grads["fc.bias"]), P(gfeat), b, C, N_CLS, S())
    g = torch.empty_like(v)
    call("avt_cls_pool_bwd", P(gfeat), P(g), b, per, C, S())
    eng.store.grads = grads
    eng.vid.backward(tape, g, eng.store)
    eng.store.grads = None
    opt.step(gflat, 1.0)
    torch.cuda.synchronize()
    snap = dict(grad=gflat, flat=flat.flat.clone(), bflat=flat.bflat.clone(), nbt=flat.nbt.clone(),
                buf=opt.momentum_buffer.clone(), t=opt.t)
    return loss, correct, logits, snap


@pytest.mark.parametrize("max_pool", [False, True])
def test_composition(max_pool):
    video, labels = _inputs()
    steps = [R3DTrainStep(_net(max_pool), "sgd", **HYPER) for _ in range(2)]
    losses = [s.step(video, labels) for s in steps]
    snaps = [_snapshot(s) for s in steps]
    assert losses[0].shape == () and losses[0].is_cuda and torch.isfinite(losses[0])
    assert torch.equal(losses[0], losses[1])
    _assert_same(snaps[0], snaps[1], "two runs from the same state")
    loss, correct, logits, hand = _by_hand(_net(max_pool), video, labels)
    assert torch.equal(loss[0], losses[0]) and torch.equal(correct, steps[0].correct)
    assert torch.equal(logits, steps[0].logits)
    _assert_same(snaps[0], hand, "the step vs the calls by hand")
    assert snaps[0]["t"] == 1 and int(snaps[0]["nbt"].min()) == 1
    gv = steps[0].flat.grad_views(steps[0].grad)
    assert bool(gv["fc.weight"].any()) and bool(gv["fc.bias"].any()) and bool(gv["conv1.weight"].any())
    assert 0 <= int(steps[0].correct) <= 2
    # the parameters the module shows are the updated ones (views of the flat store)
    assert not torch.equal(steps[0].net.fc.weight.detach().cpu(), _state()["vidnet.fc.weight"])


@pytest.mark.parametrize("max_pool", [False, True])
def test_capture_replays_equal_eager(max_pool):
    video, labels = _inputs()
    s_e, s_g, s_fix = (R3DTrainStep(_net(max_pool), "sgd", **HYPER) for _ in range(3))
    with pytest.raises(RuntimeError, match="eager step"):
        s_g.capture(video, labels)
    for s in (s_e, s_g, s_fix):
        s.step(video, labels)
    sched = [FlatMultiStepLR(s.opt, [2], gamma=0.5) for s in (s_e, s_g)]
    sv, sl = video.clone(), labels.clone()
    s_g.capture(sv, sl)
    _assert_same(_snapshot(s_e), _snapshot(s_g), "capture changed the training state")
    for k in range(3):
        le = s_e.step(video, labels)
        lg = s_g.step(video, labels)  # copied into the static inputs
        _assert_same(_snapshot(s_e), _snapshot(s_g), f"replay {k}")
        assert torch.equal(le, lg) and torch.equal(s_e.correct, s_g.correct) and torch.equal(s_e.logits, s_g.logits)
        for sc in sched:
            sc.step()
        s_fix.step(video, labels)
    assert s_g._graph is not None and s_e.opt.lr == pytest.approx(0.005) and s_g.opt.t == 4
    # the schedule took effect inside the replays: the run at a fixed lr ended elsewhere
    assert not torch.equal(_snapshot(s_fix)["flat"], _snapshot(s_g)["flat"])
    # a batch of another shape runs eagerly, on both
    le, lg = s_e.step(video[:1], labels[:1]), s_g.step(video[:1], labels[:1])
    assert torch.equal(le, lg) and s_g.logits.shape == (1, N_CLS)
    _assert_same(_snapshot(s_e), _snapshot(s_g), "eager fall-back")
    # and the graph still replays afterwards
    le, lg = s_e.step(video, labels), s_g.step(sv, sl)
    assert torch.equal(le, lg)
    _assert_same(_snapshot(s_e), _snapshot(s_g), "replay after the fall-back")


def _oracle(sd, video, max_pool):
    """fp64: (loss, {name: gradient}) of CE(fc(avgpool(r3d18_forward(video))), LABELS) on the CPU"""
    names = [k for k, v in sd.items() if k.startswith("vidnet.") and v.is_floating_point()
             and not k.endswith(("running_mean", "running_var"))]
    s = {k: (v.detach().double().clone() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for n in names:
        s[n].requires_grad_(True)
    feat = tor.r3d18_forward(s, "vidnet.", video.double(), training=True, max_pool=max_pool)
    logits = F.linear(feat.mean(dim=(2, 3, 4)), s["vidnet.fc.weight"], s["vidnet.fc.bias"])
    loss = F.cross_entropy(logits, LABELS)
    loss.backward()
    return float(loss), {n[len("vidnet."):]: s[n].grad for n in names}


@pytest.mark.parametrize("max_pool", [False, True])
def test_against_the_autograd_path(max_pool):
    """Measured on the MI355X (both settings): the two paths share the trunk's kernels, so their error columns agree
    to the printed digits for every trunk parameter; the fc gradients and the loss differ in the last fp32 bits of the
    head only."""
    video, labels = _inputs()
    sd = _state()
    net = _net(max_pool, sd).enable_backward()
    twin = copy.deepcopy(net)
    step = R3DTrainStep(net, "sgd", lr=0.0, momentum=0.0, weight_decay=0.0)
    loss = float(step.step(video, labels))
    fused = {n: g.detach().double().cpu() for n, g in step.flat.param_grad_views(step.grad).items()}
    loss_auto = F.cross_entropy(twin(video), labels)
    loss_auto.backward()
    auto = {n: p.grad.detach().double().cpu() for n, p in twin.named_parameters()}
    torch.cuda.synchronize()
    loss64, g64 = _oracle(sd, video.cpu(), max_pool)
    e_loss, e_loss_auto = abs(loss - loss64) / abs(loss64), abs(float(loss_auto) - loss64) / abs(loss64)
    print(f"max_pool={max_pool}: loss rel err fused {e_loss:.3e} autograd {e_loss_auto:.3e}")
    assert e_loss <= max(1e-4, 3 * e_loss_auto)
    assert set(fused) == set(auto) == set(g64)
    bad = []
    for n, ref in g64.items():
        r = ref.flatten().numpy()
        nr = max(np.linalg.norm(r), 1e-300)
        e = np.linalg.norm(fused[n].flatten().numpy() - r) / nr
        e_auto = np.linalg.norm(auto[n].flatten().numpy() - r) / nr
        print(f"  {n:32s} fused {e:.4e}  autograd {e_auto:.4e}")
        if not e <= max(5e-2, 3 * e_auto):
            bad.append((n, float(e), float(e_auto)))
    assert not bad, bad


def test_refusals():
    from avt_amd.model import FullModel

    video, labels = _inputs()
    with pytest.raises(RuntimeError, match="FullModel"):
        R3DTrainStep(FullModel().to(DEV).train().vidnet)
    net = _net(False)
    net.fc.bias.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="freez"):
        R3DTrainStep(net)
    with pytest.raises(RuntimeError, match="eval"):
        R3DTrainStep(_net(False).eval())
    with pytest.raises(NotImplementedError, match="process group"):
        R3DTrainStep(_net(False), process_group=object())
    with pytest.raises(ValueError, match="optimizer"):
        R3DTrainStep(_net(False), "rmsprop")
    with pytest.raises(RuntimeError, match="GPU"):
        R3DTrainStep(generate_model(18, n_classes=N_CLS).train())
    step = R3DTrainStep(_net(False), "adam", lr=1e-4, weight_decay=0.0)
    with pytest.raises(RuntimeError, match="GPU"):
        step.step(video.cpu(), labels)
    with pytest.raises(RuntimeError, match="GPU"):
        step.step(video, labels.cpu())
    with pytest.raises(ValueError, match="labels"):
        step.step(video, labels[:1])
    before = step.flat.flat.clone()
    step.net.eval()
    with pytest.raises(RuntimeError, match="eval"):
        step.step(video, labels)
    assert torch.equal(before, step.flat.flat) and step.opt.t == 0  # a refused call changed nothing
    step.net.train()
    assert torch.isfinite(step.step(video, labels)) and step.opt.t == 1  # the Adam form runs
    assert not torch.equal(before, step.flat.flat)
