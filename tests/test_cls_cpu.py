"""Host side of the R3D fine-tuning step, without a GPU:

* optim.FlatSGD <-> torch.optim.SGD ``state_dict`` conversion (checkpoint.flat_sgd_state_dict /
  load_flat_sgd_state_dict) as a round trip over a CPU FlatStore: shapes, positions, the OIHW <-> OHWI permutation of a
  2-D conv's buffer, the empty state before the first step, the None buffers of momentum 0;
* FlatMultiStepLR driving a FlatSGD exactly as torch's MultiStepLR drives torch.optim.SGD, and FlatSGD's refusals;
* tests/clscheck.py's torch restatement of the five head links against F.adaptive_avg_pool3d + nn.Linear +
  F.cross_entropy(ignore_index=-100) under autograd in fp64, and six injected faults, each of which must fall outside
  the exact comparison or the bound test_cls_kernels_gpu.py applies to the device's outputs."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import clscheck as cc
from avt_amd.checkpoint import flat_sgd_state_dict, load_checkpoint, load_flat_sgd_state_dict, save_checkpoint
from avt_amd.engine import FlatStore
from avt_amd.optim import FlatMultiStepLR, FlatSGD


class _Net(nn.Module):
    """one parameter of each rank the stores hold: Conv3d (as stored), Conv2d (OHWI in the store), BatchNorm, Linear"""

    def __init__(self):
        super().__init__()
        self.conv3 = nn.Conv3d(3, 4, 3, bias=False)
        self.conv2 = nn.Conv2d(5, 6, 3, bias=False)
        self.bn = nn.BatchNorm3d(4)
        self.fc = nn.Linear(7, 3)


def _flat_net(seed=0):
    torch.manual_seed(seed)
    net = _Net()
    return net, FlatStore(net, lambda n: True)


def _torch_sgd_after(net, steps, **hyper):
    opt = torch.optim.SGD(net.parameters(), **hyper)
    g = torch.Generator().manual_seed(5)
    for _ in range(steps):
        for p in net.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt


@pytest.mark.parametrize("hyper", [dict(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=1e-3, nesterov=False),
                                   dict(lr=0.05, momentum=0.5, dampening=0.0, weight_decay=0.0, nesterov=True),
                                   dict(lr=0.05, momentum=0.5, dampening=0.25, weight_decay=0.0, nesterov=False)])
def test_flat_sgd_state_dict_round_trip(hyper):
    net, flat = _flat_net()
    ref = _torch_sgd_after(net, 2, **hyper)
    sd = ref.state_dict()
    opt = FlatSGD(flat, lr=1.0, momentum=0.1)
    load_flat_sgd_state_dict(net, opt, sd)
    assert (opt.lr, opt.momentum, opt.dampening, opt.wd, opt.nesterov) == (
        hyper["lr"], hyper["momentum"], hyper["dampening"], hyper["weight_decay"], hyper["nesterov"])
    assert opt.t == 1  # torch's SGD keeps no count; restored buffers mean "not the first step"
    assert torch.equal(opt._hyper, torch.tensor([hyper["lr"], hyper["momentum"], hyper["dampening"],
                                                 hyper["weight_decay"], float(hyper["nesterov"])]))
    names = [n for n, _ in net.named_parameters()]
    covered = torch.zeros(flat.n_train, dtype=torch.bool)
    for i, n in enumerate(names):
        off, shape = flat.poff[n]
        want = sd["state"][i]["momentum_buffer"]
        assert tuple(want.shape) == shape
        k = want.numel()
        stored = opt.momentum_buffer[off:off + k]
        if len(shape) == 4:  # the store keeps 2-D conv weights (and what mirrors them) OHWI
            assert torch.equal(stored.view(shape[0], shape[2], shape[3], shape[1]), want.permute(0, 2, 3, 1))
        else:
            assert torch.equal(stored.view(shape), want)
        covered[off:off + k] = True
    assert not opt.momentum_buffer[~covered].any()  # the alignment padding stays zero
    back = flat_sgd_state_dict(net, opt)
    assert set(back["state"]) == set(sd["state"])
    for i in sd["state"]:
        assert torch.equal(back["state"][i]["momentum_buffer"], sd["state"][i]["momentum_buffer"])
        assert back["state"][i]["momentum_buffer"].is_contiguous()
    g0, g1 = back["param_groups"][0], sd["param_groups"][0]
    for key in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize", "params"):
        assert g0[key] == g1[key], key
    fresh = torch.optim.SGD(net.parameters(), lr=1.0)
    fresh.load_state_dict(back)  # torch accepts it, buffer for buffer
    for p, q in zip(fresh.state.values(), ref.state.values()):
        assert torch.equal(p["momentum_buffer"], q["momentum_buffer"])


def test_flat_sgd_state_dict_edges():
    net, flat = _flat_net()
    opt = FlatSGD(flat, lr=0.1, momentum=0.9)
    sd = flat_sgd_state_dict(net, opt)
    assert sd["state"] == {} and torch.optim.SGD(net.parameters(), lr=0.1, momentum=0.9).state_dict()["state"] == {}
    load_flat_sgd_state_dict(net, opt, torch.optim.SGD(net.parameters(), lr=0.3, momentum=0.9).state_dict())
    assert opt.t == 0 and opt.lr == 0.3 and not opt.momentum_buffer.any()
    # momentum 0: no buffer, torch's state holds None per parameter after a step
    plain = FlatSGD(flat, lr=0.1, momentum=0.0, weight_decay=0.0)
    assert plain.momentum_buffer is None
    ref0 = _torch_sgd_after(net, 1, lr=0.1)
    load_flat_sgd_state_dict(net, plain, ref0.state_dict())
    assert plain.t == 0
    plain.t_dev.fill_(3)
    sd0 = flat_sgd_state_dict(net, plain)
    assert all(v == {"momentum_buffer": None} for v in sd0["state"].values()) and len(sd0["state"]) == 6
    with pytest.raises(ValueError, match="momentum"):
        load_flat_sgd_state_dict(net, plain, _torch_sgd_after(net, 1, lr=0.1, momentum=0.9).state_dict())
    with pytest.raises(ValueError, match="momentum"):
        plain.momentum = 0.5
    # a wrong parameter count, a wrong shape
    other = nn.Linear(2, 2)
    with pytest.raises(ValueError, match="covers"):
        load_flat_sgd_state_dict(net, opt, torch.optim.SGD(other.parameters(), lr=0.1).state_dict())
    bad = _torch_sgd_after(net, 1, lr=0.1, momentum=0.9).state_dict()
    bad["state"][0]["momentum_buffer"] = torch.zeros(2, 2)
    with pytest.raises(ValueError, match="shape"):
        load_flat_sgd_state_dict(net, opt, bad)
    # through save_checkpoint / load_checkpoint (the fused step's entry: an object with .opt)
    class _Step:
        pass

    st = _Step()
    st.opt = FlatSGD(flat, lr=0.1, momentum=0.9)
    load_flat_sgd_state_dict(net, st.opt, _torch_sgd_after(net, 2, lr=0.2, momentum=0.9).state_dict())
    ck = save_checkpoint(None, 4, net, st, data_parallel=False)
    st2 = _Step()
    st2.opt = FlatSGD(flat, lr=0.1, momentum=0.9)
    assert load_checkpoint(ck, net, st2) == 4
    assert torch.equal(st2.opt.momentum_buffer, st.opt.momentum_buffer) and st2.opt.lr == 0.2


def test_flat_sgd_refusals():
    _, flat = _flat_net()
    for kw in (dict(momentum=0.0, nesterov=True), dict(momentum=0.9, dampening=0.1, nesterov=True)):
        with pytest.raises(ValueError, match="Nesterov"):
            FlatSGD(flat, lr=0.1, **kw)
        with pytest.raises(ValueError, match="Nesterov"):
            torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.1, **kw)
    with pytest.raises(ValueError):
        FlatSGD(flat, lr=-1.0)
    opt = FlatSGD(flat, lr=0.1, momentum=0.9, nesterov=True)
    with pytest.raises(ValueError, match="Nesterov"):
        opt.dampening = 0.5
    assert opt.dampening == 0.0 and float(opt._hyper[2]) == 0.0  # a refused write changes nothing


def test_multistep_lr_drives_flat_sgd():
    net, flat = _flat_net()
    opt = FlatSGD(flat, lr=0.1, momentum=0.9)
    sched = FlatMultiStepLR(opt, [2, 5, 6], gamma=0.1)
    ref_opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.1, momentum=0.9)
    ref = torch.optim.lr_scheduler.MultiStepLR(ref_opt, [2, 5, 6], gamma=0.1)
    assert opt.initial_lr == 0.1
    for epoch in range(8):
        assert opt.lr == pytest.approx(ref_opt.param_groups[0]["lr"], rel=1e-12), epoch
        assert float(opt._hyper[0]) == pytest.approx(opt.lr, rel=1e-6)  # the device copy follows
        ref_opt.step()
        sched.step()
        ref.step()
    assert flat_sgd_state_dict(net, opt)["param_groups"][0]["initial_lr"] == 0.1
    # resume: a new schedule at last_epoch = 6 keeps the restored lr
    opt2 = FlatSGD(flat, lr=opt.lr, momentum=0.9)
    opt2.initial_lr = 0.1
    s2 = FlatMultiStepLR(opt2, [2, 5, 6], gamma=0.1, last_epoch=6)
    assert s2.get_last_lr()[0] == pytest.approx(1e-4, rel=1e-9)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement of the head and the faults
# ---------------------------------------------------------------------------------------------------------------------
B, T, H, W_, C, N = 3, 2, 9, 5, 520, 65  # per = 90: two slots, the second short; C and n off the wave width
LABELS = torch.tensor([0, -100, N - 1])
SCALE = 0.5


def _exact_case():
    """operands on which the pool and the fc links are exact (clscheck's conditions), one ignored row"""
    g = torch.Generator().manual_seed(11)
    per = T * H * W_
    v = torch.randint(-8, 9, (B, per, C), generator=g)
    v[:, -1] = torch.randint(1, 9, (B, C), generator=g)  # the last row counts
    feat = (torch.randint(-1, 2, (B, C), generator=g) * (torch.rand(B, C, generator=g) < 0.75)).double() / 16
    Wt = torch.randint(-1, 2, (N, C), generator=g).double() / 32
    bias = torch.randint(-64, 65, (N,), generator=g).double() / 512
    dl = (torch.randint(-1, 2, (B, N), generator=g)).double() / 32
    dl[-1] = torch.tensor([1.0, -1.0]).repeat(N)[:N] / 32  # the last row's column sums are not zero
    z = torch.randn(B, N, generator=g)
    return dict(v=v, feat=feat, W=Wt, bias=bias, dl=dl, z=z, per=per)


def _run_checks(fault):
    """every link of the restatement (fp64, rounded to the device's output types) through the GPU test's checks"""
    c = _exact_case()
    out = []
    feat = cc.restate_pool_fwd(c["v"].double(), fault).float()
    out += cc.check_pool_fwd(feat, c["v"])
    logits = cc.restate_fc_fwd(c["feat"], c["W"], c["bias"], fault).float()
    out += cc.check_fc_fwd_exact(logits, c["feat"], c["W"], c["bias"])
    loss, dz, correct, _ = cc.restate_ce(c["z"].double(), LABELS, SCALE, fault)
    out += cc.check_ce(loss.float(), dz.float(), correct, c["z"], LABELS, SCALE)[0]
    gW, gbias, gfeat = cc.restate_fc_bwd(c["dl"], c["feat"], c["W"], fault)
    out += cc.check_fc_bwd_exact(gW.float(), gbias.float(), gfeat.float(), c["dl"], c["feat"], c["W"])
    gf = torch.randn(B, C, generator=torch.Generator().manual_seed(3))
    g = cc.restate_pool_bwd(gf.double(), T, H * W_, fault).float().to(torch.bfloat16)
    out += cc.check_pool_bwd(g, gf, c["per"])
    return out


def test_restated_head_passes_the_gpu_checks():
    assert cc.header_pool_rule() == "divide"
    assert _run_checks(None) == []


@pytest.mark.parametrize("fault", cc.FAULTS)
def test_injected_fault_is_caught(fault):
    link = {"pool_last_row": "pool_fwd", "pool_slot_twice": "pool_fwd", "fc_ktail_zero": "fc_fwd",
            "ce_denominator": "ce", "gbias_row": "fc_bwd gbias", "pool_bwd_hw": "pool_bwd"}[fault]
    found = _run_checks(fault)
    print(fault, found)
    assert found and all(f.startswith(link) for f in found), found


def test_restated_head_equals_torch_autograd_fp64():
    """pool -> fc -> CE(ignore_index=-100) and its gradients: the five links chained vs torch's own modules"""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, C, T, H, W_, generator=g, dtype=torch.float64, requires_grad=True)  # NCDHW, as resnet3D's map
    fc = nn.Linear(C, N).double()
    loss = SCALE * F.cross_entropy(fc(F.adaptive_avg_pool3d(x, 1).flatten(1)), LABELS, ignore_index=-100)
    loss.backward()
    v = x.detach().permute(0, 2, 3, 4, 1).reshape(B, T * H * W_, C)  # the device layout [b][per][C]
    feat = cc.restate_pool_fwd(v)
    logits = cc.restate_fc_fwd(feat, fc.weight.detach(), fc.bias.detach())
    rl, dz, correct, nv = cc.restate_ce(logits, LABELS, SCALE)
    gW, gbias, gfeat = cc.restate_fc_bwd(dz, feat, fc.weight.detach())
    gv = cc.restate_pool_bwd(gfeat, T, H * W_)
    assert nv == 2 and correct == int((logits.argmax(1) == LABELS).sum())
    tol = dict(rtol=1e-11, atol=1e-14)
    torch.testing.assert_close(rl[0], loss.detach(), **tol)
    torch.testing.assert_close(gW, fc.weight.grad, **tol)
    torch.testing.assert_close(gbias, fc.bias.grad, **tol)
    torch.testing.assert_close(gv.reshape(B, T, H, W_, C).permute(0, 4, 1, 2, 3), x.grad, **tol)
    # no valid row: zeros here (torch: NaN), stated in include/avt.h
    rl0, dz0, c0, nv0 = cc.restate_ce(logits, torch.tensor([-100, N, -1]), SCALE)
    assert float(rl0) == 0 and not dz0.any() and (c0, nv0) == (0, 0)
    assert torch.isnan(F.cross_entropy(logits, torch.full((B,), -100), ignore_index=-100))
