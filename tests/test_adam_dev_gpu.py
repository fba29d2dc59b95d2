"""The Adam that writes the weights -- avt_adam_step_dev, and avt_adam_prep_dev + avt_adam_apply_dev over regions
(device step counter, device hyper-parameters, bias corrections computed in adam_prep_kernel) -- element by element
against the fp64 AdamRef over several steps, with the learning rate and the weight decay changing between steps.
The bound is measured, not assumed: 3 x the error of torch.optim.Adam in fp32 on the CPU (tests/adamcheck.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adamcheck import HYPER, AdamPair, check_elementwise, f32  # noqa: E402
from avt_amd._lib import call  # noqa: E402

DEV = "cuda"
_KEEP = []  # device temporaries passed to the C-ABI stay alive until the test ends


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _KEEP.clear()


def P(t):
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _params(n, g):
    """fp32 parameters, a few of them exactly 0."""
    p = torch.randn(n, generator=g)
    p[5::11] = 0.0
    return p


def _grad(n, g):
    """A fresh fp32 gradient, some elements exactly 0."""
    x = torch.randn(n, generator=g)
    x[3::7] = 0.0
    return x


class DevAdam:
    """The device-side state of one flat buffer: p, exp_avg, exp_avg_sq, hyper, the step counter, coef."""

    def __init__(self, p0, hyper=HYPER, m0=None, v0=None, t0=0):
        n = p0.numel()
        self.n = n
        self.p = p0.clone().to(DEV)
        self.m = torch.zeros(n, device=DEV) if m0 is None else m0.clone().to(DEV)
        self.v = torch.zeros(n, device=DEV) if v0 is None else v0.clone().to(DEV)
        self.hyper = torch.tensor(hyper, dtype=torch.float32).to(DEV)
        self.t = torch.full((1,), t0, dtype=torch.int32, device=DEV)
        self.coef = torch.full((8,), float("nan"), device=DEV)  # AVT_ADAM_COEF_FLOATS

    def step_dev(self, g, scale=1.0):
        call("avt_adam_step_dev", P(self.p), P(g), P(self.m), P(self.v), self.n, scale, P(self.hyper), P(self.t),
             P(self.coef), S())

    def prep(self):
        call("avt_adam_prep_dev", P(self.hyper), P(self.t), P(self.coef), S())

    def apply(self, g, lo, hi, scale=1.0):
        call("avt_adam_apply_dev", P(self.p[lo:]), P(g[lo:]), P(self.m[lo:]), P(self.v[lo:]), hi - lo, scale,
             P(self.coef), S())

    def state(self):
        torch.cuda.synchronize()
        return {"p": self.p, "m": self.m, "v": self.v}

    def same_as(self, other):
        a, b = self.state(), other.state()
        return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a) and \
            self.t.item() == other.t.item()


def _check_coef(d, t):
    """The counter is t, and coef is what the host computes in double from the fp32 hyper-parameters: step size
    lr / (1 - b1^t) and sqrt(1 - b2^t) to one fp32 ulp (pow is not correctly rounded), the four copies exactly."""
    torch.cuda.synchronize()
    assert d.t.item() == t
    lr, b1, b2, eps, wd = (float(x) for x in d.hyper.cpu())
    coef = d.coef.cpu().numpy()
    want = np.array([lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)]).astype(np.float32)
    for i in range(2):
        assert abs(float(coef[i]) - float(want[i])) <= float(np.spacing(want[i])), (t, i, coef[i], want[i])
    assert coef[2:6].tolist() == [np.float32(x) for x in (b1, b2, eps, wd)]


BIG = 8_388_608 + 4 * 256 + 3  # past 8192 blocks x 256 threads x 4: the grid-stride loop wraps; a 3-element tail
POPULATION = 4096  # elements the fp32 yardstick is measured on when the kernel's own are fewer


@pytest.mark.parametrize("n,wd", [(1, 1e-4), (3, 1e-4), (4, 1e-4), (7, 1e-4), (1001, 1e-4), (1001, 0.0), (BIG, 1e-4)])
def test_adam_step_dev_six_steps(n, wd):
    """Six steps of avt_adam_step_dev: fresh gradients, lr x 0.1 written into the device hyper tensor after step 2,
    a new weight decay after step 4 (from 0 as well); after every step the counter, coef, and every element of p,
    exp_avg and exp_avg_sq."""
    g = torch.Generator().manual_seed(31 + n)
    N = max(n, POPULATION)
    hyper = HYPER[:4] + (wd,)
    p0 = _params(N, g)
    pair = AdamPair(p0, hyper)
    d = DevAdam(p0[:n], hyper)
    worst = {}
    for t in range(1, 7):
        gr = _grad(N, g)
        ref, yard, unit = pair.step(gr)
        d.step_dev(gr[:n].to(DEV))
        _check_coef(d, t)
        res = check_elementwise(f"adam_step_dev n={n} wd={wd} t={t}", d.state(), ref, yard, unit, n)
        for k, (K, E) in res.items():
            worst[k] = tuple(max(a, b) for a, b in zip(worst.get(k, (0.0, 0.0)), (K, E)))
        if t == 2:
            d.hyper[0] = f32(HYPER[0] * 0.1)
            pair.set(lr=HYPER[0] * 0.1)
        if t == 4:
            d.hyper[4] = f32(5e-4)
            pair.set(wd=5e-4)
    print(f"adam_step_dev n={n} wd={wd}: worst over 6 steps (kernel ulp, fp32 CPU Adam ulp) {worst}")


def test_adam_regions_equal_whole():
    """One avt_adam_prep_dev, then avt_adam_apply_dev over [0, a), [a, b), [b, n) == one avt_adam_step_dev, bitwise,
    over three steps; the counter advances once per step, not once per region."""
    g = torch.Generator().manual_seed(41)
    n, a, b = 10243, 1000, 4096  # cuts at multiples of 4 (16-byte regions), n % 4 == 3
    p0 = _params(n, g)
    whole, parts = DevAdam(p0), DevAdam(p0)
    for t in range(1, 4):
        gr = _grad(n, g).to(DEV)
        whole.step_dev(gr)
        parts.prep()
        for lo, hi in ((0, a), (a, b), (b, n)):
            parts.apply(gr, lo, hi)
        assert parts.same_as(whole), t
        assert parts.t.item() == t
        assert torch.equal(parts.coef[:6], whole.coef[:6])


def test_adam_grad_scale():
    """(2 g, grad_scale 0.5) == (g, 1.0), bitwise: the scale multiplies the gradient before anything else."""
    g = torch.Generator().manual_seed(43)
    n = 1003
    p0 = _params(n, g)
    one, half = DevAdam(p0), DevAdam(p0)
    for _ in range(3):
        gr = _grad(n, g).to(DEV)
        one.step_dev(gr, 1.0)
        half.step_dev(gr * 2, 0.5)
        assert half.same_as(one)


@pytest.mark.parametrize("t", [1, 2, 50])
def test_adam_host_and_device_forms_agree(t):
    """avt_adam_step with host scalars at step t == avt_adam_step_dev with the device counter at t - 1, bitwise."""
    g = torch.Generator().manual_seed(47 + t)
    n = 1003
    p0 = _params(n, g)
    m0 = 0.1 * torch.randn(n, generator=g) if t > 1 else torch.zeros(n)
    v0 = 1e-3 * torch.rand(n, generator=g) if t > 1 else torch.zeros(n)
    gr = _grad(n, g).to(DEV)
    dev, host = DevAdam(p0, m0=m0, v0=v0, t0=t - 1), DevAdam(p0, m0=m0, v0=v0, t0=t)
    dev.step_dev(gr)
    _check_coef(dev, t)  # the bias corrections at t = 50 as well
    lr, b1, b2, eps, wd = HYPER
    call("avt_adam_step", P(host.p), P(gr), P(host.m), P(host.v), n, 1.0, lr, b1, b2, eps, wd, t, S())
    assert dev.same_as(host)


@pytest.mark.parametrize("entry", ["avt_adam_step", "avt_adam_step_dev", "avt_adam_apply_dev"])
@pytest.mark.parametrize("which", ["param", "grad", "exp_avg", "exp_avg_sq"])
def test_adam_refuses_misaligned_buffers(entry, which):
    """A base pointer 4 bytes off a 16-byte boundary is refused with the documented error, and nothing runs:
    the buffers and the step counter stay as they were."""
    g = torch.Generator().manual_seed(53)
    n = 64
    d = DevAdam(_params(n + 1, g))
    d.m += 0.5
    d.v += 0.25
    gr = _grad(n + 1, g).to(DEV)
    d.prep()  # a valid coef for apply; the counter is now 1
    before = {k: v.clone() for k, v in d.state().items()}
    bufs = {"param": d.p, "grad": gr, "exp_avg": d.m, "exp_avg_sq": d.v}
    args = [P(bufs[k][1:] if k == which else bufs[k][:n]) for k in ("param", "grad", "exp_avg", "exp_avg_sq")]
    assert args[("param", "grad", "exp_avg", "exp_avg_sq").index(which)].value % 16 == 4
    lr, b1, b2, eps, wd = HYPER
    tail = {"avt_adam_step": (lr, b1, b2, eps, wd, 1, S()),
            "avt_adam_step_dev": (P(d.hyper), P(d.t), P(d.coef), S()),
            "avt_adam_apply_dev": (P(d.coef), S())}[entry]
    with pytest.raises(RuntimeError, match="buffers must be 16-byte aligned"):
        call(entry, *args, n, 1.0, *tail)
    after = d.state()
    assert all(torch.equal(before[k], after[k]) for k in before) and d.t.item() == 1
