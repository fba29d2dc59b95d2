"""The clip losses of csrc/head.hip called through the C ABI at their edges -- avt_propagation_loss, avt_npratio_loss,
avt_flip_l1_loss, avt_twoview_loss -- and their autograd wrappers in losses.py.

Every output and workspace lies inside a larger buffer filled with one NaN bit pattern, 256 bytes of it on either
side: after a call the guards must still hold that pattern and every output element must have been written.  The
workspace is exactly avt_loss_workspace_floats(n, rows) floats.

Inputs are integer multiples of 2^-8 with |x| < 4, so differences, |.| sums, NPRatio's row sums and squared
differences are exact in fp32 in ANY summation order as long as the fp64 totals stay below 2^24 units of the last
place (2^-8 for sums of |diff|, 2^-16 for sums of squares).  Each test asserts that on the CPU from the fp64 reference
before it looks at the device: a condition of the test, not a tolerance.  What it buys:

  * sgn on the device is sgn in fp64, with no near-tie exclusions, and ties between DIFFERENT frames can be built
    (NPRatio: frame s+1 a pixel rotation of frame s; Propagation: single equal pixels scattered through a clip);
  * the Propagation / NPRatio / Flip gradients are m * float32(1 / float32(b (t-1) P)) (resp. b (t-1), n) with an
    integer m in -2 .. 2 and are compared bitwise.  m = 0 is a zero of either sign: torch's own L1 backward hands the
    flipped operand -0, and so does -sgn(0) / n here; every other bit is pinned;
  * an exact sum makes the loss float32(sum) * k, one rounding after the rounding of k itself: the bound is
    4 * 2^-24 relative.  The two cases above the 1024-block cap, whose sums leave the exact range, keep
    test_twoview_gpu's 2e-5 relative bound on the loss (their gradients stay bitwise: the differences are exact).

The two-view gradients mix an MSE term with the sign terms under possible FMA contraction and keep the 1e-5
relative bound of test_twoview_loss_kernel; where the two views are equal the MSE term is exactly 0 and the entry is
compared bitwise as above."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import avenet_oracle as orc  # noqa: E402
from avt_amd._lib import call, lib, query  # noqa: E402

DEV = "cuda"
NAN_BITS = 0x7FC00000  # the sentinel of every fp32 output, workspace and guard
GUARD = 64             # floats on either side: 256 bytes
MAX_BLOCKS = 1024      # kLossMaxBlocks: partial sums at the head of the workspace, ~1024 elements per block
EXACT = float(2 ** 24)
_KEEP = []  # device temporaries passed to the C-ABI stay alive until the test ends


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _KEEP.clear()


def P(t):
    if t is None:
        return None
    if isinstance(t, Guarded):
        t = t.t
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """n floats inside a buffer of the sentinel, GUARD floats of it on either side; .t is the interior."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), NAN_BITS, device=DEV, dtype=torch.int32).view(torch.float32)
        self.t = self.buf[GUARD:GUARD + n]
        _KEEP.append(self.buf)

    def guards_intact(self):
        b = self.buf.view(torch.int32)
        return bool((b[:GUARD] == NAN_BITS).all()) and bool((b[GUARD + self.n:] == NAN_BITS).all())

    def untouched(self):
        return self.guards_intact() and bool((self.t.view(torch.int32) == NAN_BITS).all())

    def written(self):
        """guards intact and no element of the interior left as it was"""
        return self.guards_intact() and not bool(torch.isnan(self.t).any())


def _workspace(n, rows=0):
    return Guarded(int(query("avt_loss_workspace_floats", n, rows)))


def _check_workspace(ws, n, rows=0):
    """exactly the per-block partials (and NPRatio's row sums) were written, nothing else"""
    nb = min(max(-(-n // 1024), 1), MAX_BLOCKS)
    assert ws.n == MAX_BLOCKS + rows
    assert ws.guards_intact(), "a write outside avt_loss_workspace_floats"
    w = ws.t.view(torch.int32)
    assert not torch.isnan(ws.t[:nb]).any() and bool((w[nb:MAX_BLOCKS] == NAN_BITS).all())
    assert not torch.isnan(ws.t[MAX_BLOCKS:]).any()


def _draw(g, shape, q=1023):
    """integer multiples of 2^-8, |x| <= q / 256 < 4"""
    return torch.randint(-q, q + 1, shape, generator=g).float() / 256


def _k32(count):
    """float32(1 / float32(count)), as the entry points form it on the host"""
    assert count < 2 ** 24  # the product of the float factors is exact
    return np.float32(1.0) / np.float32(count)


def _same_bits(got, want):
    """bitwise, but for the sign of a zero (see the module docstring)"""
    got, want = got.detach().cpu().float().reshape(-1) + 0.0, want.detach().float().reshape(-1) + 0.0
    return torch.equal(got.view(torch.int32), want.view(torch.int32))


def _expect_grad(m, k):
    """m * k in fp32, m integer-valued"""
    assert m.abs().max() <= 2 and torch.equal(m, m.round())
    return m.float() * torch.tensor(k, dtype=torch.float32)


def _check_loss(tag, loss, total, count, unit, exact=True):
    """loss = total / count.  exact: the sum's precondition is asserted and the bound is two roundings plus slack."""
    ref = total / count
    got = float(loss)
    if exact:
        assert total / unit < EXACT, (tag, "the fp64 total leaves the exact range: shrink the values", total)
        bound = 4 * 2.0 ** -24 * abs(ref)
    else:
        bound = 2e-5 * abs(ref)
    print(f"{tag}: loss {got!r} ref {ref!r} |d| {abs(got - ref):.3e} bound {bound:.3e} exact={exact}")
    assert abs(got - ref) <= bound, (tag, got, ref, bound)


def _rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ----------------------------------------------------------------------------------------------- PropagationLoss
def _prop_ref(x):
    """x [b, t, P] -> (sum |diff| in fp64, integer m [b, t, P] with d(loss)/dx = m / (b (t-1) P))"""
    xd = x.double()
    d = xd[:, 1:] - xd[:, :-1]
    sg = torch.sign(d)
    m = torch.zeros_like(xd)
    m[:, :-1] -= sg
    m[:, 1:] += sg
    return d.abs().sum().item(), m


def _run_prop(x, want_dx=True):
    b, t, Pn = x.shape
    n = x.numel()
    xd = x.to(DEV)
    loss, ws = Guarded(1), _workspace(n)
    dx = Guarded(n) if want_dx else None
    call("avt_propagation_loss", P(xd), b, t, Pn, P(loss), P(dx), P(ws), S())
    torch.cuda.synchronize()
    assert loss.written()
    _check_workspace(ws, n)
    if want_dx:
        assert dx.written(), "a gradient element was skipped, or a write went past the buffer"
    return loss.t.cpu(), None if dx is None else dx.t.cpu()


# (b, t, P, ties, exact): ties = share of the frame pairs' pixels that are made equal
PROP_CASES = [
    (1, 2, 1, 0.0, True), (1, 2, 1, 1.0, True),
    (1, 2, 63, 0.2, True),
    (2, 3, 341, 0.1, True),      # n = 2046: a block boundary inside a frame
    (1, 2, 512, 0.1, True),      # n = 1024: one block of 4 elements per thread, exactly
    (1, 2, 513, 0.1, True),      # n = 1026: a second block of two elements
    (2, 3, 174763, 0.05, False),  # n = 1 048 578 > 1024 * 1024: the grid-stride loop wraps
]


@pytest.mark.parametrize("b,t,Pn,ties,exact", PROP_CASES)
def test_propagation_loss_abi(b, t, Pn, ties, exact):
    g = torch.Generator().manual_seed(7000 + Pn)
    x = _draw(g, (b, t, Pn))
    for s in range(t - 1):  # equal pixels at scattered positions, frame to frame
        tie = torch.rand(b, Pn, generator=g) < ties
        x[:, s + 1] = torch.where(tie, x[:, s], x[:, s + 1])
    total, m = _prop_ref(x)
    count = b * (t - 1) * Pn
    assert ties == 0.0 or (m.abs() < 2).any()
    loss, dx = _run_prop(x)
    _check_loss(f"prop {b, t, Pn}", loss, total, count, 2.0 ** -8, exact)
    assert _same_bits(dx, _expect_grad(m, _k32(count)))
    loss_n, _ = _run_prop(x, want_dx=False)  # dx = NULL: the same loss bits
    loss_2, dx_2 = _run_prop(x)              # and again: the same bits everywhere
    assert torch.equal(loss_n.view(torch.int32), loss.view(torch.int32))
    assert torch.equal(loss_2.view(torch.int32), loss.view(torch.int32))
    assert torch.equal(dx_2.view(torch.int32), dx.view(torch.int32))


# ----------------------------------------------------------------------------------------------------- NPRatio
def _npr_ref(x):
    """x [b, t, P] -> (row sums S [b, t] fp64, sum |dS|, integer m [b, t] with d(loss)/dx[b, s, :] = m / (b (t-1)))"""
    Sd = x.double().sum(dim=2)
    d = Sd[:, 1:] - Sd[:, :-1]
    sg = torch.sign(d)
    m = torch.zeros_like(Sd)
    m[:, :-1] -= sg
    m[:, 1:] += sg
    return Sd, d.abs().sum().item(), m


def _run_npr(x, want_dx=True):
    b, t, Pn = x.shape
    n, rows = x.numel(), b * t
    xd = x.to(DEV)
    loss, ws = Guarded(1), _workspace(n, rows)
    dx = Guarded(n) if want_dx else None
    call("avt_npratio_loss", P(xd), b, t, Pn, P(loss), P(dx), P(ws), S())
    torch.cuda.synchronize()
    assert loss.written()
    _check_workspace(ws, n, rows)
    if want_dx:
        assert dx.written(), "a gradient element was skipped, or a write went past the buffer"
    return loss.t.cpu(), None if dx is None else dx.t.cpu(), ws.t[MAX_BLOCKS:].cpu()


# (b, t, P, q, exact): rows = b t is never a multiple of 4 (a partial last block of npratio_rows_kernel); q / 256
# bounds |x|, shrunk where the sum of |dS| would leave the exact range
NPR_CASES = [
    (1, 2, 1, 1023, True),
    (8193, 2, 1, 1023, True),    # rows = 16 386 > 4 * 4096 (the rb cap) and > 256 * 17 blocks (the row loop wraps)
    (3, 3, 2, 1023, True),
    (5462, 3, 3, 255, True),     # rows = 16 386 again, n = 49 158: 49 blocks of 256 rows
    (5, 3, 63, 1023, True),      # one short of a wave per row
    (3, 2, 64, 1023, True),      # exactly a wave, t = 2
    (7, 3, 65, 1023, True),      # a second trip of the lane loop for lane 0 alone
    (3, 5, 196, 1023, True),
    (2677, 2, 196, 1023, False),  # rows P = 1 049 384 > 1024 * 1024: the gradient loop wraps
]


@pytest.mark.parametrize("b,t,Pn,q,exact", NPR_CASES)
def test_npratio_loss_abi(b, t, Pn, q, exact):
    g = torch.Generator().manual_seed(7100 + Pn + b)
    x = _draw(g, (b, t, Pn), q)
    tie = torch.rand(b, t - 1, generator=g) < 0.3
    tie.view(-1)[0] = True
    if tie.numel() > 1:
        tie.view(-1)[1] = False
    for s in range(t - 1):  # a true tie between different frames: the next frame is this one, rotated by a pixel
        x[:, s + 1] = torch.where(tie[:, s, None], x[:, s].roll(1, dims=1), x[:, s + 1])
    Sd, total, m = _npr_ref(x)
    assert Sd.abs().max().item() * 256 < EXACT  # every row sum, and so every difference of two, is exact in fp32
    if Pn > 1:
        assert (x[:, 1:][tie] != x[:, :-1][tie]).any()  # the tied frames do differ
    assert (m.abs() < 2).any()
    count = b * (t - 1)
    loss, dx, Sdev = _run_npr(x)
    assert torch.equal(Sdev.double().reshape(b, t), Sd), "npratio_rows_kernel: a row sum is not the exact sum"
    _check_loss(f"npratio {b, t, Pn}", loss, total, count, 2.0 ** -8, exact)
    assert _same_bits(dx, _expect_grad(m, _k32(count))[:, :, None].expand(b, t, Pn))
    loss_n, _, _ = _run_npr(x, want_dx=False)
    loss_2, dx_2, _ = _run_npr(x)
    assert torch.equal(loss_n.view(torch.int32), loss.view(torch.int32))
    assert torch.equal(loss_2.view(torch.int32), loss.view(torch.int32))
    assert torch.equal(dx_2.view(torch.int32), dx.view(torch.int32))


# ---------------------------------------------------------------------------------------------------- FlipLoss
def _run_flip(x, y, want_dx, want_dy):
    rows, W = x.shape
    n = x.numel()
    xd, yd = x.to(DEV), y.to(DEV)
    loss, ws = Guarded(1), _workspace(n)
    dx = Guarded(n) if want_dx else None
    dy = Guarded(n) if want_dy else None
    call("avt_flip_l1_loss", P(xd), P(yd), rows, W, P(loss), P(dx), P(dy), P(ws), S())
    torch.cuda.synchronize()
    assert loss.written()
    _check_workspace(ws, n)
    for o in (dx, dy):
        assert o is None or o.written(), "a gradient element was skipped, or a write went past the buffer"
    return loss.t.cpu(), None if dx is None else dx.t.cpu(), None if dy is None else dy.t.cpu()


# (rows, W): W = 1 and odd W flip the centre column onto itself; n = 1023 / 1024 / 1025 around one block's 4 per thread
FLIP_CASES = [(1, 1), (1, 2), (1, 3), (1, 7), (1, 224), (1023, 1), (1024, 1), (1025, 1), (341, 3), (512, 2),
              (147, 7), (5, 224)]


@pytest.mark.parametrize("rows,W", FLIP_CASES)
def test_flip_l1_loss_abi(rows, W):
    g = torch.Generator().manual_seed(7200 + 300 * rows + W)
    x, y = _draw(g, (rows, W)), _draw(g, (rows, W))
    tie = torch.rand(rows, W, generator=g) < 0.15  # exact zeros of y - hflip(x), scattered ...
    if W % 2 == 1:
        tie[::2, W // 2] = True                    # ... and at the centre column, which flips onto itself
    y = torch.where(tie, x.flip(1), y)
    d = y.double() - x.double().flip(1)
    total, n = d.abs().sum().item(), rows * W
    sg = torch.sign(d)
    assert (sg == 0).any()
    k = _k32(n)
    want_dy, want_dx = _expect_grad(sg, k), _expect_grad(-sg.flip(1), k)
    losses = []
    for wdx, wdy in [(True, True), (False, True), (True, False), (False, False), (True, True)]:
        loss, dx, dy = _run_flip(x, y, wdx, wdy)
        losses.append(loss)
        assert dx is None or _same_bits(dx, want_dx)
        assert dy is None or _same_bits(dy, want_dy)
    _check_loss(f"flip {rows, W}", losses[0], total, n, 2.0 ** -8)
    for other in losses[1:]:  # the same loss bits whichever gradients are asked for, and run to run
        assert torch.equal(other.view(torch.int32), losses[0].view(torch.int32))


# ------------------------------------------------------------------------------------------------ two-view loss
def _run_twoview(ce, w1, w2, b, t, Pn, lw):
    n = b * t * Pn
    ced, w1d, w2d = ce.to(DEV), w1.to(DEV), w2.to(DEV)
    out, d1, d2 = Guarded(5), Guarded(n), Guarded(n)
    call("avt_twoview_loss", P(ced[0:1]), P(ced[1:2]), P(w1d), P(w2d), b, t, Pn, lw, P(out), P(d1), P(d2), S())
    torch.cuda.synchronize()
    assert out.written() and d1.written() and d2.written()
    return out.t.cpu(), d1.t.cpu(), d2.t.cpu()


# (b, t, P): one element per frame; n below one wave; n = 1024 (one element per thread); n = 1026; two clips of t = 2
TWOVIEW_SHAPES = [(1, 2, 1), (1, 2, 31), (1, 2, 512), (1, 3, 342), (2, 2, 196)]


@pytest.mark.parametrize("lw", [0.1, 0.0, 100.0])
@pytest.mark.parametrize("b,t,Pn", TWOVIEW_SHAPES)
def test_twoview_loss_abi(b, t, Pn, lw):
    g = torch.Generator().manual_seed(7300 + Pn)
    n = b * t * Pn
    w1 = _draw(g, (b, t, Pn))
    for s in range(t - 1):  # ties between frames
        tie = torch.rand(b, Pn, generator=g) < 0.2
        w1[:, s + 1] = torch.where(tie, w1[:, s], w1[:, s + 1])
    # the second view a few 2^-8 steps away, so the MSE and the sign terms of the gradient are of one size; equal
    # to the first (df = 0) at about a third of the pixels
    w2 = w1 + torch.randint(-3, 4, (b, t, Pn), generator=g).float() / 256
    if n == 2:
        w2[0, 1, 0] = w1[0, 1, 0]
    same = w1 == w2
    assert same.any()
    ce = torch.tensor([1.7, 2.3])

    (t1, m1), (t2, m2) = _prop_ref(w1), _prop_ref(w2)
    se = ((w1.double() - w2.double()) ** 2).sum().item()
    assert t1 * 2 ** 8 < EXACT and t2 * 2 ** 8 < EXACT and se * 2 ** 16 < EXACT

    # the fp64 restatement of test_twoview_gpu.test_twoview_loss_kernel
    x1, x2 = w1.double().requires_grad_(True), w2.double().requires_grad_(True)
    l2 = F.mse_loss(x1, x2) * (100 - lw)
    cons = orc.propagation_loss(x1.reshape(b, t, 1, Pn)) + orc.propagation_loss(x2.reshape(b, t, 1, Pn))
    hard, aug = lw * ce[0].double(), lw * ce[1].double()
    comb = (hard + aug) / 2 + l2 + cons
    comb.backward()
    ref = torch.stack([comb, hard, aug, l2, cons]).detach()

    out, d1, d2 = _run_twoview(ce, w1, w2, b, t, Pn, lw)
    print(f"twoview {b, t, Pn} lw={lw}: out {out.tolist()} ref {ref.tolist()}")
    np.testing.assert_allclose(out.double().numpy(), ref.numpy(), rtol=2e-5, atol=1e-8)
    if lw == 100.0:
        assert out[3].item() == 0.0  # the MSE weight 100 - lw is exactly 0
    e1, e2 = _rel_err(d1, x1.grad.reshape(-1)), _rel_err(d2, x2.grad.reshape(-1))
    print(f"twoview {b, t, Pn} lw={lw}: rel_err d1 {e1:.3e} d2 {e2:.3e} bound 1e-5")
    assert e1 < 1e-5 and e2 < 1e-5
    # sign-only entries: the views agree (or the MSE weight is 0), what is left is m * kprop exactly
    k = _k32(b * (t - 1) * Pn)
    sel = torch.ones_like(same) if lw == 100.0 else same
    assert _same_bits(d1.reshape(b, t, Pn)[sel], _expect_grad(m1, k)[sel])
    assert _same_bits(d2.reshape(b, t, Pn)[sel], _expect_grad(m2, k)[sel])
    out_2, d1_2, d2_2 = _run_twoview(ce, w1, w2, b, t, Pn, lw)
    for a, c in ((out, out_2), (d1, d1_2), (d2, d2_2)):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))


# --------------------------------------------------------------------------------------------------- refusals
def _refused(name, needle, args, outputs):
    """the call returns non-zero with avt_last_error() naming it, and no output or guard has changed"""
    rc = getattr(lib(), name)(*args)
    msg = query("avt_last_error").decode(errors="replace")
    torch.cuda.synchronize()
    assert rc != 0, (name, needle)
    assert needle in msg, (name, needle, msg)
    for o in outputs:
        assert o.untouched(), (name, needle)


def test_loss_refusals():
    """t = 1, b = 0, P = 0, rows = 0, W = 0 and a NULL required pointer: refused before any launch.  NULL and shape
    cases alternate, so each message read back is the one this refusal wrote."""
    x = torch.ones(64, device=DEV)
    ce = torch.ones(2, device=DEV)
    loss, dx, dy, ws, out = Guarded(1), Guarded(64), Guarded(64), _workspace(64, 64), Guarded(5)
    outs = (loss, dx, dy, ws, out)
    for name in ("avt_propagation_loss", "avt_npratio_loss"):
        cases = [((2, 1, 4), None), (None, 0), ((0, 2, 4), None), (None, 4), ((2, 2, 0), None), (None, 6)]
        for dims, null in cases:
            b, t, Pn = dims or (2, 2, 4)
            args = [P(x), b, t, Pn, P(loss), P(dx), P(ws), S()]
            if null is not None:
                args[null] = None
            needle = "null pointer" if dims is None else f"(b={b} t={t} P={Pn})"
            _refused(name, needle, args, outs)
    for dims, null in [((2, 1, 4), None), (None, 0), ((0, 2, 4), None), (None, 1), ((2, 2, 0), None), (None, 2),
                       ((1, 1, 1), None), (None, 3), ((2, 0, 4), None), (None, 8), ((0, 0, 0), None), (None, 9),
                       ((2, -1, 4), None), (None, 10)]:
        b, t, Pn = dims or (2, 2, 4)
        args = [P(ce[0:1]), P(ce[1:2]), P(x), P(x), b, t, Pn, 0.1, P(out), P(dx), P(dy), S()]
        if null is not None:
            args[null] = None
        needle = "null pointer" if dims is None else f"(b={b} t={t} P={Pn})"
        _refused("avt_twoview_loss", needle, args, outs)
    for dims, null in [((0, 4), None), (None, 0), ((4, 0), None), (None, 1), ((0, 0), None), (None, 4),
                       ((-1, 4), None), (None, 7)]:
        rows, W = dims or (4, 4)
        args = [P(x), P(x), rows, W, P(loss), P(dx), P(dy), P(ws), S()]
        if null is not None:
            args[null] = None
        _refused("avt_flip_l1_loss", "null pointer" if dims is None else "empty input", args, outs)


# ------------------------------------------------------------------------------------- the wrappers of losses.py
def _modules():
    from avt_amd.losses import FlipLoss, NPRatio, PropagationLoss

    return {"prop": (PropagationLoss(), orc.propagation_loss), "npratio": (NPRatio(), orc.npratio_loss),
            "flip": (FlipLoss(), orc.flip_loss)}


def _views(kind, dtype, seed):
    """non-contiguous inputs of `dtype` on the CPU: a transposed view (and, for FlipLoss, a sliced one too)"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(3, 4, 9, 7, generator=g).to(dtype)
    base[:, 2] = base[:, 1]  # a tie, transposed or not
    xs = [base.transpose(2, 3)]
    if kind == "flip":
        xs.append(torch.randn(3, 4, 7, 18, generator=g).to(dtype)[..., ::2])
    assert not any(x.is_contiguous() for x in xs)
    return xs


def _wrapper_run(kind, xs_cpu, upstream, needs_grad=None):
    """(loss, grads) of the module on device views equal to xs_cpu (same strides), and of the fp64 oracle"""
    mod, ref_fn = _modules()[kind]
    needs_grad = needs_grad or [True] * len(xs_cpu)
    xd = []
    for x, ng in zip(xs_cpu, needs_grad):
        d = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=DEV)
        d.copy_(x)
        assert d.stride() == x.stride()
        xd.append(d.requires_grad_(ng))
    loss = mod(*xd)
    if upstream is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(upstream, device=DEV, dtype=loss.dtype))
    xr = [x.double().requires_grad_(ng) for x, ng in zip(xs_cpu, needs_grad)]  # the values as rounded to the dtype
    ref = ref_fn(*xr)
    (ref * (1.0 if upstream is None else upstream)).backward()
    torch.cuda.synchronize()
    return loss, [d.grad for d in xd], ref.detach(), [r.grad for r in xr]


@pytest.mark.parametrize("upstream", [None, 2.5])
@pytest.mark.parametrize("kind", ["prop", "npratio", "flip"])
def test_wrappers_noncontiguous_upstream(kind, upstream):
    """A transposed / sliced view and an upstream gradient other than 1, fp32, against avenet_oracle in fp64 (the
    bounds of the module tests in test_twoview_gpu)."""
    loss, grads, ref, rgrads = _wrapper_run(kind, _views(kind, torch.float32, 7400), upstream)
    assert loss.dtype == torch.float32 and loss.shape == ()
    e = abs(loss.item() - ref.item()) / abs(ref.item())
    print(f"{kind} upstream={upstream}: loss rel err {e:.3e}")
    assert e < 1e-5
    for gd, gr in zip(grads, rgrads):
        assert gd.dtype == torch.float32 and gd.shape == gr.shape
        assert _rel_err(gd, gr) < 1e-6


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind", ["prop", "npratio", "flip"])
def test_wrappers_half_inputs(kind, dtype):
    """bf16 / fp16 inputs: the loss and the gradients come back in the input's dtype and are the fp32 results of
    the same (rounded) values, cast; the fp32 results are held to the fp64 oracle."""
    xs = _views(kind, dtype, 7500)
    loss, grads, ref, rgrads = _wrapper_run(kind, xs, None)
    loss32, grads32, _, _ = _wrapper_run(kind, [x.float() for x in xs], None)
    assert loss.dtype == dtype and loss32.dtype == torch.float32
    assert abs(loss32.item() - ref.item()) < 1e-5 * abs(ref.item())
    assert torch.equal(loss.view(torch.int16), loss32.to(dtype).view(torch.int16))
    for gd, g32, gr in zip(grads, grads32, rgrads):
        assert gd.dtype == dtype and g32.dtype == torch.float32
        assert _rel_err(g32, gr) < 1e-6
        assert torch.equal(gd.contiguous().view(torch.int16), g32.to(dtype).contiguous().view(torch.int16))


@pytest.mark.parametrize("needs", [(True, False), (False, True)])
def test_flip_wrapper_one_sided_grad(needs):
    loss, grads, ref, rgrads = _wrapper_run("flip", _views("flip", torch.float32, 7600), 0.7, list(needs))
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
    for ng, gd, gr in zip(needs, grads, rgrads):
        if ng:
            assert _rel_err(gd, gr) < 1e-6
        else:
            assert gd is None and gr is None


def test_wrapper_errors():
    """The documented refusals of losses.py, an empty FlipLoss input among them (a ValueError, where the row count
    n / W would divide by zero)."""
    mods = _modules()
    ok = torch.ones(2, 3, 4, 5, device=DEV)
    for kind in ("prop", "npratio"):
        mod = mods[kind][0]
        with pytest.raises(ValueError, match="t >= 2"):
            mod(torch.ones(2, 1, 4, 5, device=DEV))
        with pytest.raises(ValueError, match=r"expects \[b, t, h, w\]"):
            mod(torch.ones(2, 3, 20, device=DEV))
        with pytest.raises(ValueError, match=r"expects \[b, t, h, w\]"):
            mod(torch.ones(2, 3, 4, 5, 1, device=DEV))
        with pytest.raises(RuntimeError, match="no CPU path"):
            mod(torch.ones(2, 3, 4, 5))
        with pytest.raises(RuntimeError):  # refused by the entry point: nothing to average
            mod(torch.ones(2, 3, 0, 5, device=DEV))
    flip = mods["flip"][0]
    with pytest.raises(ValueError, match="one shape"):
        flip(ok, torch.ones(2, 3, 5, 4, device=DEV))
    with pytest.raises(ValueError, match="one shape"):
        flip(ok, torch.ones(6, 4, 5, device=DEV))
    with pytest.raises(ValueError, match="one shape"):
        flip(torch.ones((), device=DEV), torch.ones((), device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        flip(ok.cpu(), ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        flip(ok, ok.cpu())
    for shape in [(2, 3, 4, 0), (0, 5), (0,)]:
        with pytest.raises(ValueError, match="empty"):
            flip(torch.ones(shape, device=DEV), torch.ones(shape, device=DEV))
