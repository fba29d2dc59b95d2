"""The classifier-head entry points of csrc/cls.hip and avt_sgd_step_dev (csrc/misc.hip) through the C ABI.

Every device buffer -- inputs, outputs, workspaces -- lies between two 256-byte guard bands of one NaN bit pattern
(0x7FC0 per 16 bits: a NaN as bf16 and as fp32); outputs and workspaces are pre-filled with it.  After a call the
guards must still hold the pattern and every output element must have been written.

* pool (avt_cls_pool_fwd / _bwd): integer values |v| <= 8, so every partial sum is exact in fp32 (sum |v| < 2^24,
  asserted) and the result must equal fp32(S) DIVIDED by fp32(per) -- the rule include/avt.h states, read from the
  header by clscheck.header_pool_rule -- bit for bit; the backward equals bf16_rne of the same expression everywhere.
* fc (avt_cls_fc_fwd / _bwd): feat in multiples of 2^-4, W and dlogits in {-1, 0, 1} 2^-5, sum |products| <= 1
  (asserted): results equal the fp64 products exactly.  Random fp32 draws: (K + 2) 2^-24 sum |a b| per element.
* CE (avt_softmax_ce): fp64 reference on the same fp32 logits; bound = the roundings counted in the source + 3 Y
  (clscheck.ce_reference), Y measured per case from torch's fp32 log_softmax / softmax on the CPU and printed.
* SGD (avt_sgd_step_dev): operands on which every product and sum of three steps is exact in fp32 (asserted by an
  fp32 and an fp64 run of the rule on the CPU): the device equals torch.optim.SGD on the CPU bit for bit."""
import ctypes
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import clscheck as cc  # noqa: E402
from avt_amd._lib import call, query  # noqa: E402

DEV = "cuda"
SENT = 0x7FC0
GUARD = 128  # int16 elements: 256 bytes
_KEEP = []


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _KEEP.clear()


class Guarded:
    """A tensor of ``shape`` / ``dtype`` inside a buffer of the sentinel, 256 bytes of it on either side; .t is the
    interior (16-byte aligned), holding ``init`` or the sentinel."""

    def __init__(self, shape, dtype, init=None):
        shape = tuple(shape) if not isinstance(shape, int) else (shape,)
        n = math.prod(shape)
        self.half = n * torch.empty(0, dtype=dtype).element_size() // 2
        self.buf = torch.full((2 * GUARD + self.half,), SENT, device=DEV, dtype=torch.int16)
        self.t = self.buf[GUARD:GUARD + self.half].view(dtype).view(shape)
        if init is not None:
            self.t.copy_(init.to(dtype))
        _KEEP.append(self.buf)

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.half:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())

    def written(self):
        """guards intact and no element left as the sentinel"""
        if not self.guards_intact():
            return False
        if self.t.is_floating_point():
            return not bool(torch.isnan(self.t).any())
        return not bool((self.t.view(torch.int16).view(-1, self.t.element_size() // 2) == SENT).all(1).any())


def P(x):
    if x is None:
        return None
    t = x.t if isinstance(x, Guarded) else x
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------------
# pool
# ---------------------------------------------------------------------------------------------------------------------
def _pool_fwd(v, b, per, C, ws="auto"):
    need = int(query("avt_cls_pool_ws_bytes", b, per, C))
    assert need == b * cc.pool_slots(per) * C * 4
    feat = Guarded((b, C), torch.float32)
    wsg = Guarded(need // 4, torch.float32) if ws == "auto" else ws
    call("avt_cls_pool_fwd", P(v), P(feat), b, per, C, P(wsg), need, S())
    torch.cuda.synchronize()
    return feat, wsg


@pytest.mark.parametrize("per", [1, 2, 63, 64, 65, 784, 3136])
def test_pool_exact(per):
    """forward and backward at every (b, C); per <= 64 uses exactly one partial slot per clip, per >= 65 more than one
    (784: 13, the last of 16 rows; 3136: 49)"""
    g = torch.Generator().manual_seed(per)
    assert (cc.pool_slots(per) == 1) == (per <= 64)
    for b, C in itertools.product([1, 3], [8, 512, 520]):
        vi = torch.randint(-8, 9, (b, per, C), generator=g)
        vi[:, -1].clamp_(min=1)  # the last row always counts
        v = Guarded((b, per, C), torch.bfloat16, vi.float())
        feat, ws = _pool_fwd(v, b, per, C)
        assert feat.written() and ws.written() and v.guards_intact(), (b, C)
        assert cc.check_pool_fwd(feat.t, vi) == [], (b, C)
        # the slots themselves: plain per-slot sums, exact
        want_ws = torch.stack([vi[:, k * 64:(k + 1) * 64].sum(1) for k in range(cc.pool_slots(per))], 1).float()
        assert torch.equal(ws.t.view(b, -1, C).cpu(), want_ws), (b, C)
        for gf in (vi.sum(1).float(), torch.randn(b, C, generator=g)):
            gfeat = Guarded((b, C), torch.float32, gf)
            gout = Guarded((b, per, C), torch.bfloat16)
            call("avt_cls_pool_bwd", P(gfeat), P(gout), b, per, C, S())
            torch.cuda.synchronize()
            assert gout.written() and gfeat.guards_intact(), (b, C)
            assert cc.check_pool_bwd(gout.t, gf, per) == [], (b, C)


def test_pool_workspace_refusals():
    b, per, C = 2, 130, 16
    v = Guarded((b, per, C), torch.bfloat16, torch.ones(b, per, C))
    feat = Guarded((b, C), torch.float32)
    need = int(query("avt_cls_pool_ws_bytes", b, per, C))
    ws = Guarded(need // 4, torch.float32)
    with pytest.raises(RuntimeError, match="workspace"):
        call("avt_cls_pool_fwd", P(v), P(feat), b, per, C, None, need, S())
    with pytest.raises(RuntimeError, match="workspace"):
        call("avt_cls_pool_fwd", P(v), P(feat), b, per, C, P(ws), need - 4, S())
    with pytest.raises(RuntimeError, match="workspace"):
        call("avt_cls_pool_fwd", P(v), P(feat), b, per, C, P(ws), 0, S())
    with pytest.raises(RuntimeError):
        call("avt_cls_pool_fwd", P(v), P(feat), b, per, 12, P(ws), need, S())  # C % 8 != 0
    torch.cuda.synchronize()
    assert feat.untouched() and ws.untouched()
    assert int(query("avt_cls_pool_ws_bytes", b, per, 12)) == 0


# ---------------------------------------------------------------------------------------------------------------------
# fc
# ---------------------------------------------------------------------------------------------------------------------
def _fc_run(feat, W, bias, dl):
    b, C = feat.shape
    n = W.shape[0]
    gi = [Guarded(x.shape, torch.float32, x) for x in (feat, W, bias, dl)]
    logits = Guarded((b, n), torch.float32)
    gW, gb, gf = Guarded((n, C), torch.float32), Guarded((n,), torch.float32), Guarded((b, C), torch.float32)
    call("avt_cls_fc_fwd", P(gi[0]), P(gi[1]), P(gi[2]), P(logits), b, C, n, S())
    call("avt_cls_fc_bwd", P(gi[3]), P(gi[0]), P(gi[1]), P(gW), P(gb), P(gf), b, C, n, S())
    torch.cuda.synchronize()
    for x in gi:
        assert x.guards_intact()
    for x in (logits, gW, gb, gf):
        assert x.written()
    return logits.t, gW.t, gb.t, gf.t


_FC_WORST = {}


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 400, 1039])
def test_fc_exact_and_bounded(n):
    g = torch.Generator().manual_seed(100 + n)
    for b, C in itertools.product([1, 2, 5, 8], [8, 512, 520]):
        # exact operands: feat in multiples of 2^-4 (three in four non-zero), W and dlogits in {-1, 0, 1} 2^-5
        feat = (torch.randint(0, 2, (b, C), generator=g) * 2 - 1) * (torch.rand(b, C, generator=g) < 0.75) / 16.0
        W = torch.randint(-1, 2, (n, C), generator=g) / 32.0
        bias = torch.randint(-64, 65, (n,), generator=g) / 512.0
        dl = torch.randint(-1, 2, (b, n), generator=g) / 32.0
        logits, gW, gb, gf = _fc_run(feat, W, bias, dl)
        assert cc.check_fc_fwd_exact(logits, feat, W, bias) == [], (b, C)
        assert cc.check_fc_bwd_exact(gW, gb, gf, dl, feat, W) == [], (b, C)
        # random fp32 draws
        feat, W, bias, dl = (torch.randn(s, generator=g) for s in ((b, C), (n, C), (n,), (b, n)))
        bad, worst = cc.check_fc_random(*_fc_run(feat, W, bias, dl), dl, feat, W, bias)
        for k, v in worst.items():
            _FC_WORST[k] = max(_FC_WORST.get(k, 0.0), v)
        assert bad == [], (b, C, bad)
    print(f"n={n}: worst error / bound so far {({k: round(v, 3) for k, v in _FC_WORST.items()})}")


# ---------------------------------------------------------------------------------------------------------------------
# CE
# ---------------------------------------------------------------------------------------------------------------------
_CE_WORST = {"loss": 0.0, "dlogits": 0.0}


def _ce_run(z, labels, scale, want_correct=True, want_dl=True):
    b, n = z.shape
    zg, lg = Guarded((b, n), torch.float32, z), Guarded((b,), torch.int64, labels)
    loss = Guarded((1,), torch.float32)
    dl = Guarded((b, n), torch.float32) if want_dl else None
    cor = Guarded((1,), torch.int32) if want_correct else None
    call("avt_softmax_ce", P(zg), P(lg), b, n, scale, P(loss), P(dl), P(cor), S())
    torch.cuda.synchronize()
    assert zg.guards_intact() and lg.guards_intact() and loss.written()
    assert dl is None or dl.written()
    assert cor is None or cor.written()
    return loss.t.cpu(), None if dl is None else dl.t.cpu(), None if cor is None else int(cor.t.item())


def _label_sets(b, n, g):
    edge = [0, n - 1, -100, n]
    if b == 1:
        return [[e] for e in edge]
    if b == 3:
        return [edge[:3], [n, n - 1, 0]]
    return [edge + torch.randint(0, n, (b - 5,), generator=g).tolist() + [0]]


@pytest.mark.parametrize("n", [1, 2, 64, 65, 1024, 1025, 1039, 2051])
def test_softmax_ce(n):
    g = torch.Generator().manual_seed(200 + n)
    for b in (1, 3, 8):
        draws = {"normal": torch.randn(b, n, generator=g),
                 "spread80": (torch.rand(b, n, generator=g) * 160 - 80),
                 "equal": torch.full((b, n), 1.5)}
        for (name, z), scale in zip(draws.items(), (1.0, 0.37, 1.0)):
            for labels in _label_sets(b, n, g):
                labels = torch.tensor(labels)
                loss, dl, cor = _ce_run(z, labels, scale)
                bad, ratios, ref = cc.check_ce(loss, dl, cor, z, labels, scale)
                print(f"ce n={n} b={b} {name} labels={labels.tolist()[:4]}: valid {ref['nvalid']} correct {cor} "
                      f"Y_loss {ref['Y_loss']:.2e} Y_dl {ref['Y_dl']:.2e} error/bound loss {ratios['loss']:.3f} "
                      f"dlogits {ratios['dlogits']:.3f}")
                for k in _CE_WORST:
                    _CE_WORST[k] = max(_CE_WORST[k], ratios[k])
                assert bad == [], (b, name, bad)
    print(f"n={n}: worst error / bound so far {_CE_WORST}")


def test_softmax_ce_edges():
    g = torch.Generator().manual_seed(7)
    n, b = 70, 5
    z = torch.randn(b, n, generator=g)
    # every row ignored: loss and gradients exactly +0, nothing counted (torch: NaN)
    for labels in ([-100] * b, [n, -1, -100, n + 5, -(2 ** 40)]):
        loss, dl, cor = _ce_run(z, torch.tensor(labels), 1.0)
        assert cc.check_ce(loss, dl, cor, z, torch.tensor(labels), 1.0)[0] == []
        assert cc.bits(loss)[0] == 0 and not cc.bits(dl).any() and cor == 0
    # ties for the argmax: the lowest index counts, whichever side of the wave's strided passes it lies on
    z = torch.zeros(b, n)
    z[0, [3, 67]] = 2.0   # lanes 3 and 3 (second pass): label 3 is right, 67 is not
    z[1, [3, 67]] = 2.0
    z[2, [10, 9]] = 5.0   # neighbouring lanes
    z[3, [69, 5]] = 1.0   # the later pass first in memory order of the lanes
    z[4, :] = -3.0        # all equal: index 0
    labels = torch.tensor([3, 67, 9, 69, 0])
    loss, dl, cor = _ce_run(z, labels, 1.0)
    assert cor == 3
    assert cc.check_ce(loss, dl, cor, z, labels, 1.0)[0] == []
    # optional outputs left out; the loss is the same bits
    loss2, dl2, cor2 = _ce_run(z, labels, 1.0, want_correct=False, want_dl=False)
    assert dl2 is None and cor2 is None and torch.equal(cc.bits(loss2), cc.bits(loss))
    # one row, many rows per wave (b > 16: a wave takes rows w, w + 16, ...)
    b2 = 37
    z2 = torch.randn(b2, 33, generator=g)
    lab2 = torch.randint(-1, 34, (b2,), generator=g)
    loss, dl, cor = _ce_run(z2, lab2, 2.0)
    assert cc.check_ce(loss, dl, cor, z2, lab2, 2.0)[0] == []


# ---------------------------------------------------------------------------------------------------------------------
# SGD
# ---------------------------------------------------------------------------------------------------------------------
LR = 2.0 ** -3
GRID_CAP_ELEMS = 2048 * 256 * 4  # kSgdGridCap blocks of 256 threads, four elements a thread
HYPERS = [dict(momentum=m, nesterov=nv, dampening=d, wd=wd, gs=gs)
          for m, nv, d, wd, gs in itertools.product([0.0, 0.5], [False, True], [0.0, 0.5], [0.0, 0.25], [1.0, 0.5])
          if not (nv and (m == 0.0 or d != 0.0))]


def _sgd_dev(p0, grads, h, lr=LR, buf_arg=True, step0=0, buf0=None, lrs=None):
    """run len(grads) device steps; returns (p, buf Guarded or None, step count)"""
    n = p0.numel()
    p = Guarded((n,), torch.float32, p0)
    buf = Guarded((n,), torch.float32, buf0) if buf_arg else None
    hyper = Guarded((5,), torch.float32, torch.tensor([lr, h["momentum"], h["dampening"], h["wd"],
                                                       float(h["nesterov"])]))
    step = Guarded((1,), torch.int32, torch.tensor([step0], dtype=torch.int32))
    for k, gr in enumerate(grads):
        if lrs is not None:
            hyper.t[0] = lrs[k]  # a stream-ordered write between launches
        gg = Guarded((n,), torch.float32, gr)
        call("avt_sgd_step_dev", P(p), P(gg), P(buf), n, h["gs"], P(hyper), P(step), S())
        torch.cuda.synchronize()
        assert gg.guards_intact()
    assert p.written() and hyper.guards_intact() and step.guards_intact()
    return p.t.cpu(), buf, int(step.t.item())


def _sgd_torch(p0, grads, h, lrs=None):
    """torch.optim.SGD on the CPU (grad_scale folded into the gradient: a power of two, exact)"""
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([p], lr=LR, momentum=h["momentum"], dampening=h["dampening"], weight_decay=h["wd"],
                          nesterov=h["nesterov"], foreach=False)
    for k, gr in enumerate(grads):
        if lrs is not None:
            opt.param_groups[0]["lr"] = lrs[k]
        p.grad = gr * h["gs"]
        opt.step()
    return p.detach(), opt.state[p].get("momentum_buffer")


def _exact_draw(n, g, steps=3):
    """multiples of 2^-2 (hence of 2^-8) with |x| <= 4: with lr = 2^-3, wd = 2^-2, momentum / dampening / grad_scale
    in {0, 1/2, 1} three steps stay on a 2^-20 grid below 8 -- 23 bits -- so fp32 is exact; the callers assert it"""
    draw = lambda: torch.randint(-16, 17, (n,), generator=g).float() / 4  # noqa: E731
    return draw(), [draw() for _ in range(steps)]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025, GRID_CAP_ELEMS + 1024 + 3])
def test_sgd_equals_torch_bitwise(n):
    g = torch.Generator().manual_seed(300 + n % 1000)
    hypers = HYPERS if n < GRID_CAP_ELEMS else [HYPERS[0], HYPERS[-1]]
    p0, grads = _exact_draw(n, g)
    for h in hypers:
        # the condition: every product and sum exact in fp32 -- the rule in fp32 and in fp64 agree
        a32, b32 = cc.sgd_rule(p0, grads, LR, h["momentum"], h["dampening"], h["wd"], h["nesterov"], h["gs"],
                               torch.float32)
        a64, b64 = cc.sgd_rule(p0, grads, LR, h["momentum"], h["dampening"], h["wd"], h["nesterov"], h["gs"],
                               torch.float64)
        assert torch.equal(a32.double(), a64) and (b32 is None or torch.equal(b32.double(), b64)), h
        want_p, want_buf = _sgd_torch(p0, grads, h)
        assert torch.equal(want_p.double(), a64), h  # the issue's rule is torch's
        p, buf, steps = _sgd_dev(p0, grads, h)
        assert steps == 3
        assert torch.equal(cc.bits(p), cc.bits(want_p)), h
        if h["momentum"] == 0.0:
            assert buf.untouched(), h  # neither read (it holds NaN) nor written
            p_nobuf, _, _ = _sgd_dev(p0, grads, h, buf_arg=False)
            assert torch.equal(cc.bits(p_nobuf), cc.bits(want_p)), h
        else:
            assert buf.written() and torch.equal(cc.bits(buf.t.cpu()), cc.bits(want_buf)), h


def test_sgd_first_step_and_lr_between_launches():
    g = torch.Generator().manual_seed(9)
    n = 1029
    p0, grads = _exact_draw(n, g)
    h = dict(momentum=0.5, nesterov=False, dampening=0.5, wd=0.25, gs=1.0)
    # the first step sets buf = g whatever the buffer held (NaN here) and in spite of the dampening
    p, buf, _ = _sgd_dev(p0, grads[:1], h)
    g1 = grads[0] + 0.25 * p0
    assert torch.equal(buf.t.cpu(), g1) and torch.equal(p, p0 - LR * g1)
    # a restored buffer (step count 1 on entry): blended, not replaced
    b0 = _exact_draw(n, g)[0]
    p, buf, steps = _sgd_dev(p0, grads[:1], h, step0=1, buf0=b0)
    assert steps == 2 and torch.equal(buf.t.cpu(), 0.5 * b0 + 0.5 * g1)
    # buf == NULL: plain SGD although hyper[1] says 0.5
    p, _, _ = _sgd_dev(p0, grads[:1], h, buf_arg=False)
    assert torch.equal(p, p0 - LR * g1)
    # an lr written between launches is seen by the next one
    lrs = [2.0 ** -3, 2.0 ** -4, 2.0 ** -2]
    want_p, want_buf = _sgd_torch(p0, grads, h, lrs=lrs)
    p, buf, _ = _sgd_dev(p0, grads, h, lrs=lrs)
    assert torch.equal(cc.bits(p), cc.bits(want_p)) and torch.equal(cc.bits(buf.t.cpu()), cc.bits(want_buf))
    assert not torch.equal(p, _sgd_torch(p0, grads, h)[0])
    # n == 0 is accepted; a misaligned buffer is refused
    x = Guarded((8,), torch.float32, torch.zeros(8))
    hyp = Guarded((5,), torch.float32, torch.zeros(5))
    st = Guarded((1,), torch.int32, torch.zeros(1, dtype=torch.int32))
    call("avt_sgd_step_dev", P(x), P(x), None, 0, 1.0, P(hyp), P(st), S())
    with pytest.raises(RuntimeError, match="aligned"):
        call("avt_sgd_step_dev", P(x.t[1:]), P(x), None, 4, 1.0, P(hyp), P(st), S())
    torch.cuda.synchronize()
    assert int(st.t.item()) == 0


@pytest.mark.parametrize("n", [5, 1025])
def test_sgd_random_draws_bounded(n):
    """one step from a random state vs the rule in fp64: |p| error <= 8 2^-24 (|p| + lr sum |terms|), the buffer's
    <= 8 2^-24 sum |its terms| (8: the roundings of the rule)"""
    g = torch.Generator().manual_seed(400 + n)
    lr = 0.0123
    for h in HYPERS:
        h = dict(h, wd=h["wd"] * 0.37, gs=h["gs"] * 0.9, momentum=h["momentum"] * 1.7, dampening=h["dampening"] * 0.3)
        p0, gr, b0 = (torch.randn(n, generator=g) for _ in range(3))
        for step0 in (0, 1):
            p, buf, _ = _sgd_dev(p0, [gr], h, lr=lr, step0=step0, buf0=b0)
            f = lambda x: torch.tensor(x, dtype=torch.float32).double()  # noqa: E731 (the constants as the device sees them)
            mu, keep, wd, gs = f(h["momentum"]), 1.0 - f(h["dampening"]), f(h["wd"]), f(h["gs"])
            P0, G, B0 = p0.double(), gr.double(), b0.double()
            gg = G * gs + wd * P0
            terms = (G * gs).abs() + (wd * P0).abs()
            if h["momentum"] != 0:
                nb = gg if step0 == 0 else mu * B0 + keep * gg
                tb = terms if step0 == 0 else (mu * B0).abs() + keep * terms
                assert bool(((buf.t.cpu().double() - nb).abs() <= 8 * cc.U * tb).all()), (h, step0)
                if h["nesterov"]:
                    gg, terms = gg + mu * nb, terms + mu * tb
                else:
                    gg, terms = nb, tb
            want = P0 - f(lr) * gg
            bound = 8 * cc.U * (P0.abs() + f(lr) * terms)
            assert bool(((p.double() - want).abs() <= bound).all()), (h, step0)
