"""AVENet.enable_folded_inference(): the eval forward with every BatchNorm folded into its conv.

Parity is judged against the fp64 oracle (avenet_oracle.avenet_forward(training=False)) with the unfolded eval
forward's own deviation from that oracle, on the same inputs, as the yardstick: err_folded <= max(floor, 3 x
err_unfolded) per output, with the floors of tests/test_model_gpu.py for A, the logits and
weighted_A.  Pos / Neg = sigmoid(+-(A - eps) / tau) have slope at most 1 / (4 tau) = 8.4 in A, so their floor is
that slope times A's.  Folding moves the roundings (weights are rounded after scaling; the pre-BN tensor is never
rounded), so the error is another draw of the same size."""
import numpy as np
import pytest
import torch

import avenet_oracle as orc
from test_trunk2d_eval_forced_cpu import e2e_inputs, running_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
NAMES = ("A", "logits", "weighted_A", "Pos", "Neg")
TAU = 0.03


def _state(seed=0):
    """running_state() (moved running statistics) with gamma and beta of every BatchNorm moved too (seeded)."""
    sd = running_state()
    g = torch.Generator().manual_seed(1000 + seed)
    for k in sd:
        if ".bn" in k or "downsample.1" in k:
            if k.endswith(".weight"):
                sd[k] = sd[k] * (1 + 0.2 * torch.randn(sd[k].shape, generator=g))
            elif k.endswith(".bias"):
                sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
            elif k.endswith("running_var") and seed:
                sd[k] = sd[k] * (0.5 + torch.rand(sd[k].shape, generator=g))
    return sd


def _model(sd, folded):
    from avt_amd.model import AVENet, HardWayArgs

    m = AVENet(HardWayArgs(), False)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    return m.enable_folded_inference() if folded else m


def _inputs(B):
    if B == 2:
        img, aud, _ = e2e_inputs()
    else:
        img, aud = orc.make_image(B, 64), orc.make_spectrogram(B, 65, 76)
    return img, aud


def _fwd(model, img, aud):
    with torch.no_grad():
        out = model(img.to(DEV), aud.to(DEV))
    torch.cuda.synchronize()
    return [o.detach().cpu() for o in out]


def _oracle(sd, img, aud):
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    with torch.no_grad():
        return [o.double() for o in orc.avenet_forward(sd64, img.double(), aud.double(), None, training=False)]


def _devs(out, ref):
    """The per-output deviations of tests/test_model_gpu.py (+ Pos, Neg as A)."""
    A, logits, wA, Pos, Neg = (o.double().numpy() for o in out)
    rA, rl, rw, rP, rN = (r.numpy() for r in ref)
    b = A.shape[0]
    diag = np.eye(b, logits.shape[1], k=1, dtype=bool)
    return {
        "A_abs": np.abs(A - rA).max(),
        "logits_off_abs": np.abs(logits[~diag] - rl[~diag]).max(),
        "logits_diag_rel": (np.abs(logits[diag] - rl[diag]) / np.abs(rl[diag])).max(),
        "wA_rel": np.abs(wA - rw.reshape(wA.shape)).max() / np.abs(rw).max(),
        "Pos_abs": np.abs(Pos - rP).max(),
        "Neg_abs": np.abs(Neg - rN).max(),
    }


FLOORS = {"A_abs": 1e-2, "logits_off_abs": 2e-2, "logits_diag_rel": 2e-3, "wA_rel": 5e-2,
          "Pos_abs": 1e-2 / (4 * TAU), "Neg_abs": 1e-2 / (4 * TAU)}


def _assert_parity(tag, folded_out, unfolded_out, ref):
    ef, eu = _devs(folded_out, ref), _devs(unfolded_out, ref)
    for k in ef:
        tol = max(FLOORS[k], 3 * eu[k])
        print(f"{tag}: {k}: folded {ef[k]:.3e} unfolded {eu[k]:.3e} tol {tol:.3e}")
    for k in ef:
        assert ef[k] <= max(FLOORS[k], 3 * eu[k]), (tag, k, ef[k], eu[k])


@pytest.mark.parametrize("B", [2, 3])
def test_parity_with_oracle(B):
    """Folded against the fp64 oracle, the unfolded eval forward of the same build as the yardstick.
    Measured on one MI355X: see DESIGN 6k."""
    sd = _state()
    img, aud = _inputs(B)
    ref = _oracle(sd, img, aud)
    plain, fold = _model(sd, False), _model(sd, True)
    out_u, out_f = _fwd(plain, img, aud), _fwd(fold, img, aud)
    for a, b in zip(out_u, out_f):
        assert a.shape == b.shape and a.dtype == b.dtype
    assert not all(torch.equal(a, b) for a, b in zip(out_u, out_f))  # the folded path ran
    assert fold.engine().fold_launches == 2
    _assert_parity(f"B={B}", out_f, out_u, ref)


def test_no_op_without_the_opt_in():
    """Without the opt-in an eval forward is bitwise what an untouched model gives; with it, a model in train mode
    or one taking the autograd eval path goes where it went."""
    sd = _state()
    img, aud = _inputs(2)
    a, b = _model(sd, False), _model(sd, False)
    for x, y in zip(_fwd(a, img, aud), _fwd(b, img, aud)):
        assert torch.equal(x, y)
    assert a.engine().folds is None and a.engine().fold_launches == 0


def test_state_dict_train_step_and_eval_backward_unchanged():
    """After enable_folded_inference(): the same 248 state_dict keys, bitwise; a train-mode step (forward, CE
    backward, Adam) bitwise that of a model without the opt-in; a grad-mode eval call with enable_eval_backward()
    gives bitwise the gradients it gives without it."""
    from avt_amd.optim import Adam

    sd = _state()
    img, aud = _inputs(2)
    runs = []
    for folded in (False, True):
        m = _model(sd, folded)
        if folded:
            _fwd(m, img, aud)  # a fold exists before the train step
        s0 = m.state_dict()
        assert len(s0) == 248 and list(s0) == list(sd)
        for k in sd:
            assert torch.equal(s0[k].cpu(), sd[k].to(s0[k].dtype)), k
        m.train()
        opt = Adam(m.parameters(), lr=1e-4, weight_decay=1e-4)
        logits = m(img.to(DEV), aud.to(DEV))[1]
        loss = torch.nn.CrossEntropyLoss()(logits, torch.zeros(2, dtype=torch.long, device=DEV))
        loss.backward()
        grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        opt.step()
        m.eval().enable_eval_backward()
        m.zero_grad()
        A = m(img.to(DEV).requires_grad_(), aud.to(DEV))[0]
        A.sum().backward()
        eg = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        torch.cuda.synchronize()
        runs.append((loss.item(), grads, {k: v.clone() for k, v in m.state_dict().items()}, eg))
    (l0, g0, w0, e0), (l1, g1, w1, e1) = runs
    assert l0 == l1 and sorted(g0) == sorted(g1) and sorted(e0) == sorted(e1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    for n in w0:
        assert torch.equal(w0[n], w1[n]), n
    for n in e0:
        assert torch.equal(e0[n], e1[n]), n


def _adam_step(m, img, aud):
    """The device-side Adam (libavt writes the flat parameters through raw pointers) on seeded gradients: no forward,
    so the step is the only change."""
    from avt_amd.optim import Adam

    opt = Adam(m.parameters(), lr=1e-2)
    torch.manual_seed(7)
    for p in m.parameters():
        p.grad = torch.randn_like(p)
    opt.step()
    m.zero_grad()


def _load_other(m, img, aud):
    m.load_state_dict(_state(1))


def _scale_var(m, img, aud):
    with torch.no_grad():
        m.imgnet.layer2[0].bn1.running_var.mul_(4)


def _train_forward(m, img, aud):
    m.train()
    with torch.no_grad():
        m(img.to(DEV), aud.to(DEV))
    m.eval()


@pytest.mark.parametrize("change", [_adam_step, _load_other, _scale_var, _train_forward])
def test_staleness(change):
    """A folded forward, then a change of the parameters or buffers: the next folded forward is bitwise that of a
    fresh folded model built from the updated state (the fold is deterministic), within the parity bound of the fp64
    oracle on that state, and differs from the output before the change."""
    sd = _state()
    img, aud = _inputs(2)
    m = _model(sd, True)
    before = _fwd(m, img, aud)
    n0 = m.engine().fold_launches
    change(m, img, aud)
    after = _fwd(m, img, aud)
    assert m.engine().fold_launches == n0 + 2  # refolded once per trunk
    new_sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    fresh = _fwd(_model(new_sd, True), img, aud)
    for x, y in zip(after, fresh):
        assert torch.equal(x, y)
    assert not torch.equal(before[0], after[0])
    _assert_parity(change.__name__, after, _fwd(_model(new_sd, False), img, aud), _oracle(new_sd, img, aud))


def test_no_needless_refold():
    """Two folded forwards with nothing changed: bitwise equal outputs, and the second launches no fold."""
    img, aud = _inputs(3)
    m = _model(_state(), True)
    first = _fwd(m, img, aud)
    n = m.engine().fold_launches
    assert n == 2
    second = _fwd(m, img, aud)
    assert m.engine().fold_launches == n
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    m.invalidate_folded()
    _fwd(m, img, aud)
    assert m.engine().fold_launches == n + 2


def test_layer4_hook():
    """A forward hook on imgnet.layer4 sees tensors of the unfolded path's shapes and dtypes.  Its output against the
    fp64 oracle's layer4 map by the parity rule (floor: the conv bound, 8e-3 of the map's largest magnitude; yardstick:
    the unfolded path's hook output); its input against the unfolded path's within twice that bound (both paths lie
    within it of the exact map; the oracle exposes no layer3 map)."""
    sd = _state()
    img, aud = _inputs(2)
    seen = {}
    for folded in (False, True):
        m = _model(sd, folded)
        m.imgnet.layer4.register_forward_hook(
            lambda mod, inp, out, f=folded: seen.__setitem__(f, (inp[0].detach().cpu(), out.detach().cpu())))
        _fwd(m, img, aud)
    for i in range(2):
        u, f = seen[False][i], seen[True][i]
        assert u.shape == f.shape and u.dtype == f.dtype == torch.float32 and torch.isfinite(f).all()
    assert tuple(seen[True][0].shape) == (2, 256, 4, 4) and tuple(seen[True][1].shape) == (2, 512, 4, 4)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        ref = orc.resnet18_forward(sd64, "imgnet.", img.double(), "vision", training=False)
    scale = ref.abs().max().item()
    e_u = (seen[False][1].double() - ref).abs().max().item() / scale
    e_f = (seen[True][1].double() - ref).abs().max().item() / scale
    rel = max(8e-3, 3 * e_u)
    d_in = (seen[True][0].double() - seen[False][0].double()).abs().max().item() / seen[False][0].abs().max().item()
    print(f"layer4 hook: output folded {e_f:.3e} unfolded {e_u:.3e} of max |ref|; input folded - unfolded {d_in:.3e}")
    assert e_f <= rel
    assert d_in <= 2 * rel
