"""The video's gradient through the standalone R3D-18 trunk (``enable_backward(input_grad=True)``): the stem's input
gradient kernel ``avt_video_stem_dgrad`` in both forms against ``torch.nn.grad.conv3d_input`` in fp64 on identical
operands, and ``video.grad`` of the whole trunk against ``tube_oracle`` under autograd.

Kernel bound: rel_err < 1e-5, test_kernels_gpu.py::test_stem_dgrad's bound for the same kind of result -- fp32 sums of
products of identically rounded operands, nothing rounded afterwards.  It holds for BOTH forms: the MFMA form fuses the
temporal fold-back and stores no bf16 intermediate (its weights are rounded to bf16, and so are the reference's)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import tube_oracle as tor
from avt_amd._lib import call, query
from gradcheck import rule_full

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
_KEEP = []
LABELS = torch.tensor([7, 911])


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _KEEP.clear()
    call("avt_set_video_stem_dgrad", -1)


def P(t):
    if t is None:
        return None
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# (N, T, H, W)
SHAPES = [
    (2, 1, 9, 8),      # T = 1: all seven temporal taps but one fall outside; odd H, even W
    (1, 3, 7, 7),      # T < 7: every frame sees a clipped tap range
    (2, 6, 10, 14),
    (1, 7, 8, 7),      # T = kt
    (1, 8, 12, 10),    # T = kt + 1: the fold ring's first reuse of a slot
    (3, 2, 1, 5),      # H = 1: the h % 2 = 1 classes are empty
    (3, 2, 5, 1),      # W = 1: the w % 2 = 1 classes are empty
    (2, 4, 20, 22),    # tile interiors plus ragged edges, several blocks per class
    (1, 9, 33, 31),
    (2, 16, 32, 32),   # two clips of the tube step's 16 frames (test_clips_do_not_mix runs them apart too)
    (1, 2, 224, 224),  # the real frame size
]
_REF = {}


def _data(shape):
    """(gy bf16 [N,T,P,Q,64], w fp32 OIDHW, {form: fp64 reference}) of a shape, computed once.  Form 0 is referred to
    the fp32 weights, form 1 to the same weights rounded to bf16.  At the real frame size the fp32 weights are
    bf16-exact, so that one fp64 reference (several seconds of CPU) serves both forms."""
    if shape not in _REF:
        N, T, H, W = shape
        g = torch.Generator().manual_seed(53)
        Pq, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        gy = torch.randn(N, T, Pq, Q, 64, generator=g).to(torch.bfloat16)
        w = (torch.randn(64, 3, 7, 7, 7, generator=g) * (2.0 / (64 * 343)) ** 0.5).float()
        if H * W > 10000:
            w = w.to(torch.bfloat16).float()
        gyn = gy.double().permute(0, 4, 1, 2, 3)

        def ref(wt):
            return torch.nn.grad.conv3d_input((N, 3, T, H, W), wt.double(), gyn, stride=(1, 2, 2), padding=3)

        r1 = ref(w.to(torch.bfloat16))
        r0 = r1 if torch.equal(w.to(torch.bfloat16).float(), w) else ref(w)
        _REF[shape] = (gy, w, {0: r0, 1: r1})
    return _REF[shape]


def _run(form, gy, w, shape, wp=None):
    N, T, H, W = shape
    call("avt_set_video_stem_dgrad", form)
    if wp is None:
        wp = torch.empty(int(query("avt_video_stem_dgrad_pack_bytes")), device=DEV, dtype=torch.uint8)
        call("avt_pack_video_stem_dgrad", P(w), P(wp), S())
    gx = torch.full((N, 3, T, H, W), float("nan"), device=DEV)
    # each form reads its own weight argument only
    call("avt_video_stem_dgrad", P(gy), P(w) if form == 0 else None, P(wp) if form == 1 else None, P(gx), N, T, H, W,
         S())
    return gx


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_video_stem_dgrad(shape, form):
    """avt_video_stem_dgrad (form 0 direct / form 1 MFMA with the fused fold-back) vs fp64 conv3d_input, rel_err <
    1e-5 (no bf16 intermediate in either form); the output pre-filled with NaN (every voxel is written); two calls
    bitwise equal."""
    gy, w, refs = _data(shape)
    gyd, wd = gy.to(DEV), w.to(DEV)
    gx = _run(form, gyd, wd, shape)
    gx2 = _run(form, gyd, wd, shape)
    torch.cuda.synchronize()
    err = rel_err(gx, refs[form])
    print(f"{shape} form {form}: video stem dgrad rel err {err:.3e}")
    assert err < 1e-5, err
    assert torch.equal(gx, gx2)


def test_video_stem_dgrad_forms_agree():
    """The weaker second check: on bf16-exact weights the two forms sum the same products (in different orders)."""
    shape = (2, 6, 10, 14)
    gy, w, _ = _data(shape)
    gyd, wd = gy.to(DEV), w.to(torch.bfloat16).float().to(DEV)
    a, b = _run(0, gyd, wd, shape), _run(1, gyd, wd, shape)
    torch.cuda.synchronize()
    assert rel_err(a, b) < 1e-5


@pytest.mark.parametrize("form", [0, 1])
def test_clips_do_not_mix(form):
    """(2, 16, 32, 32): the two clips run together equal the two clips run separately, bitwise -- no gradient leaks
    across the clip boundary (frames outside a clip are zero padding)."""
    shape = (2, 16, 32, 32)
    gy, w, _ = _data(shape)
    gyd, wd = gy.to(DEV), w.to(DEV)
    both = _run(form, gyd, wd, shape)
    parts = [_run(form, gyd[i:i + 1].contiguous(), wd, (1,) + shape[1:]) for i in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(both, torch.cat(parts))


def test_video_stem_dgrad_refusals():
    """A missing operand of the selected form, and a setting outside -1..1, are errors (nothing runs)."""
    from avt_amd._lib import lib

    gy = torch.zeros(1, 1, 2, 2, 64, device=DEV, dtype=torch.bfloat16)
    gx = torch.zeros(1, 3, 1, 4, 4, device=DEV)
    w = torch.zeros(64, 3, 7, 7, 7, device=DEV)
    call("avt_set_video_stem_dgrad", 1)
    assert lib().avt_video_stem_dgrad(P(gy), P(w), None, P(gx), 1, 1, 4, 4, S()) != 0
    call("avt_set_video_stem_dgrad", 0)
    assert lib().avt_video_stem_dgrad(P(gy), None, None, P(gx), 1, 1, 4, 4, S()) != 0
    assert lib().avt_set_video_stem_dgrad(2) != 0


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def _standalone(max_pool, **kw):
    from avt_amd.resnet3D import generate_model

    sd = tor.make_tube_state(0)
    net = generate_model(18, no_max_pool=not max_pool, n_classes=1039)
    net.load_state_dict({k[len("vidnet."):]: v for k, v in sd.items() if k.startswith("vidnet.")})
    net.enable_backward(**kw)
    return net.to(DEV).train(), sd


def oracle_video_grad(sd, video, max_pool, autocast, training):
    """(logits, d CE / d video in fp64, {name: parameter gradient}) of tube_oracle.r3d18_forward on the CPU."""
    names = [k for k, v in sd.items() if k.startswith("vidnet.") and v.is_floating_point()
             and not k.endswith(("running_mean", "running_var"))]
    dt = torch.float32 if autocast else torch.float64
    s = {k: (v.detach().to(dt).clone() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for n in names:
        s[n].requires_grad_(True)
    x = video.to(dt).clone().requires_grad_(True)
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        feat = tor.r3d18_forward(s, "vidnet.", x, training=training, max_pool=max_pool)
        logits = F.linear(feat.mean(dim=(2, 3, 4)), s["vidnet.fc.weight"], s["vidnet.fc.bias"])
    F.cross_entropy(logits.float() if autocast else logits, LABELS).backward()
    return logits.detach(), x.grad.double(), {n[len("vidnet."):]: s[n].grad.double() for n in names}, s


@pytest.mark.parametrize("max_pool", [False, True])
def test_video_grad_train_mode(max_pool):
    """video.grad of CE(fc logits) on make_video(2, 4, 64) in train mode vs the fp64 oracle, by gradcheck.rule_full
    against the bf16-autocast oracle's own video gradient (the yardstick; printed).  As for the parameter gradients
    (test_r3d_backward_end_to_end) the train-mode yardstick on this 2-clip batch is loose: the batch statistics of
    two clips amplify the forward's bf16 noise (measured: yardstick 0.36 without the max-pool, 0.37 with it, above
    0.3; this build 0.35 / 0.38, a third of its bound).  The tight end-to-end check is test_video_grad_forced_tape
    (measured: yardstick 8.7e-3, this build 9.4e-3 / 9.3e-3, 0.19 of the 5e-2 floor)."""
    video = tor.make_video(2, 4, 64)
    net, sd = _standalone(max_pool, input_grad=True)
    x = video.to(DEV).requires_grad_(True)
    F.cross_entropy(net(x), LABELS.to(DEV)).backward()
    torch.cuda.synchronize()
    assert x.grad is not None and x.grad.dtype == torch.float32 and x.grad.shape == video.shape
    _, g64, _, _ = oracle_video_grad(sd, video, max_pool, False, True)
    _, gbf, _, _ = oracle_video_grad(sd, video, max_pool, True, True)
    assert torch.isfinite(gbf).all()
    bad, e, e_ref, ratio = rule_full(x.grad.cpu().numpy(), g64.numpy(), gbf.numpy())
    print(f"max_pool={max_pool} train: video.grad e {e:.3e}, yardstick e_ref {e_ref:.3e} ({ratio:.2f} of its bound)")
    assert not bad, bad


def _ncdhw(t, b):
    n, h, w, c = t.shape
    return t.view(b, n // b, h, w, c).permute(0, 4, 1, 2, 3).float().cpu()


@pytest.mark.parametrize("max_pool", [False, True])
def test_video_grad_forced_tape(max_pool):
    """The tight end-to-end check: R3DEngine.backward's video gradient against fp64 autograd through
    tube_oracle.r3d18_forward_forced fed the GPU's own tape (as test_r3d_backward_forced_gpu.py; the oracle is used
    unchanged: its input is a differentiable bf16 rounding of the video).  Loss (logits * glogits).sum(); yardstick: the
    same oracle with every stored activation gradient rounded to bf16.  rule_full, and the yardstick's own error must
    stay under that file's 0.1 cap so that the bound bites."""
    from avt_amd.tube import R3DEngine

    video = tor.make_video(2, 4, 64)
    b = video.shape[0]
    glogits = tor.make_glogits(b)
    net, sd = _standalone(max_pool, input_grad=True)
    engine = R3DEngine(net._flat_store(), "", max_pool=max_pool, with_backward=True)
    logits, tp = engine.forward(video.to(DEV), True, tape=True, input_grad=True)
    gflat = torch.zeros(engine.flat.n_train, device=DEV, dtype=torch.float32)
    gx = engine.backward(tp, glogits.float().to(DEV), gflat, want_gvideo=True)
    torch.cuda.synchronize()
    tape = {"c0": _ncdhw(tp["c0"], b), "h0": _ncdhw(tp["h0"], b), "blocks": []}
    for tb in tp["blocks"]:
        tape["blocks"].append({k: _ncdhw(tb[k], b) for k in ("c1", "h1", "c2", "cd", "out") if k in tb})
    tape64 = {k: v.double() for k, v in tape.items() if k != "blocks"}
    tape64["blocks"] = [{k: v.double() for k, v in tb.items()} for tb in tape["blocks"]]
    s = {k: (v.to(torch.bfloat16) if v.dim() == 5 else v).double() for k, v in sd.items()
         if k.startswith("vidnet.") and v.is_floating_point()}
    out = {}
    for name, rnd in (("ref", None), ("yard", lambda g: g.to(torch.bfloat16).to(g.dtype))):
        x = video.double().clone().requires_grad_(True)
        feat = tor.r3d18_forward_forced(s, "vidnet.", x, tape64, max_pool=max_pool, grad_round=rnd)
        lg = F.linear(feat.mean(dim=(2, 3, 4)), s["vidnet.fc.weight"], s["vidnet.fc.bias"])
        (lg * glogits).sum().backward()
        out[name] = x.grad
    bad, e, e_ref, ratio = rule_full(gx.cpu().numpy(), out["ref"].numpy(), out["yard"].numpy())
    print(f"max_pool={max_pool} forced tape: video gradient e {e:.3e}, yardstick e_ref {e_ref:.3e} "
          f"({ratio:.2f} of its bound)")
    assert e_ref <= 0.1, e_ref
    assert not bad, bad


def test_input_grad_behaviour():
    """The opt-in: plain enable_backward() and eval_grad alone still refuse a video that requires grad; input_grad alone
    still refuses an eval-mode grad-mode call; FullModel.vidnet refuses any arguments; widening the opt-in keeps the
    flat store; with every parameter frozen the video still gets its gradient and no parameter does; video.grad is
    bitwise equal across two runs; a video that does not require grad gives parameter gradients bitwise equal to a
    plain enable_backward() trunk's from the same state dict."""
    from avt_amd.model import FullModel

    video = tor.make_video(2, 4, 64).to(DEV)
    labels = LABELS.to(DEV)
    with pytest.raises(RuntimeError):
        FullModel().vidnet.enable_backward(input_grad=True)
    plain, _ = _standalone(False)
    with pytest.raises(NotImplementedError, match="input_grad"):
        plain(video.clone().requires_grad_(True))
    ev, _ = _standalone(False, eval_grad=True)
    with pytest.raises(NotImplementedError, match="input_grad"):
        ev(video.clone().requires_grad_(True))
    net, _ = _standalone(False, input_grad=True)
    net.eval()
    with pytest.raises(NotImplementedError, match="eval_grad"):
        net(video.clone().requires_grad_(True))
    net.train()
    flat = net._flat_store()
    assert net.enable_backward(input_grad=True, eval_grad=True) is net and net._flat_store() is flat
    # parameter gradients: the same bits as the plain trunk's when the video does not require grad
    grads = []
    for m in (plain, net):
        m.zero_grad(set_to_none=True)
        F.cross_entropy(m(video), labels).backward()
        grads.append({n: p.grad.clone() for n, p in m.named_parameters()})
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n
    # ... and when it does; video.grad bitwise repeatable
    state = {k: v.clone() for k, v in net.state_dict().items()}
    vg = []
    for _ in range(2):
        net.load_state_dict(state)
        net.zero_grad(set_to_none=True)
        x = video.clone().requires_grad_(True)
        loss = F.cross_entropy(net(x), labels)
        loss.backward()
        vg.append(x.grad.clone())
    with pytest.raises(RuntimeError):
        loss.backward()
    assert torch.equal(vg[0], vg[1]) and torch.isfinite(vg[0]).all() and vg[0].abs().max() > 0
    # the pure-attribution case: every parameter frozen
    net.load_state_dict(state)
    net.zero_grad(set_to_none=True)
    for p in net.parameters():
        p.requires_grad_(False)
    x = video.clone().requires_grad_(True)
    F.cross_entropy(net(x), labels).backward()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in net.parameters())
    assert torch.equal(x.grad, vg[0])
