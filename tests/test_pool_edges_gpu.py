"""The pooling kernels of pool.hip and the fused stem of bn.hip against independent references (torch's CPU pools, fp64
autograd, tests/bncheck.py's bounds) at the inputs the first-generation tests never build: signed values (a pool that
pads with 0 instead of -inf), ties away from 0, -0.0 / +0.0, NaN, extents of 1 and 2, C / 8 no power of two.

Left out, with the reason:
  * the second grid-stride trip of maxpool3s2_fwd / bwd: the grid is capped at 8192 blocks of 256 threads, so it takes
    more than 16.7 M output vectors, a 67 M-element input; the index arithmetic is `long long` and the same on every
    trip.
  * the four-row unrolled reduce loop under avt_stem_maxpool_bn_relu_bwd: it takes N P Q > 49,152 pooled rows at
    C = 64, a 12.6 M-element input; it is the bn_bwd_reduce_kernel with the recomputed mask that
    test_bn_edges_gpu.py runs through avt_bn_relu_bwd at (66001, 64).

Stem inputs: c = bf16(1.5 randn - 0.3), seed 24, gamma = 2 + 0.02 randn, beta = 1.5 + 0.1 randn.  The argmax is compared
where the reference window's maximum is clear of its runner-up by more than the two elements' forward bounds; the
windows skipped (ties of the ReLU's zeros, and maxima closer than a bf16 rounding) are, on the reference alone,
1.90 % at (2, 12, 14, 64), 1.64 % at (1, 7, 9, 64), 1.78 % at (2, 9, 192, 64), 0.78 % at (1, 3, 1, 64); the test asserts
<= 2 %.  (With gamma = 1, beta = 0.1 randn the two-pixel windows of (1, 3, 1, 64) alone are all-zero 22 % of the time.)"""
import ctypes
import functools
import types

import pytest
import torch
import torch.nn.functional as F

import bncheck as bc

pytestmark = pytest.mark.gpu

from avt_amd._lib import call, query  # noqa: E402

DEV = "cuda"
_KEEP = []


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _KEEP.clear()


def P(t):
    if t is None:
        return None
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def D(t):
    d = t.to(DEV)
    _KEEP.append(d)
    return d


def pooled(n):
    return (n + 2 - 3) // 2 + 1


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def window_pos(ind, H, W):
    """torch's max_pool2d index (h W + w of the input plane, [N][C][P][Q]) as the window position r * 3 + s."""
    Pn, Qn = ind.shape[2], ind.shape[3]
    h, w = ind // W, ind % W
    r = h - (2 * torch.arange(Pn).view(1, 1, Pn, 1) - 1)
    s = w - (2 * torch.arange(Qn).view(1, 1, 1, Qn) - 1)
    assert ((r >= 0) & (r < 3) & (s >= 0) & (s < 3)).all()
    return r * 3 + s


def same_bits_or_nan(got, ref):
    return torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(
        got.nan_to_num().view(torch.int16), ref.nan_to_num().view(torch.int16))


def bf16_ulp(x):
    """Spacing of the bf16 numbers at |x| (fp64 in and out; 0 at 0)."""
    _, e = torch.frexp(x.abs())
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 8))


# ------------------------------------------------------------------------------------------ MaxPool2d(3, 2, 1)
POOL_SHAPES = [(2, 12, 14, 64), (1, 7, 9, 24), (3, 1, 5, 8), (2, 5, 1, 8), (1, 2, 2, 16), (1, 1, 1, 8), (2, 33, 38, 128)]


def pool_input(N, H, W, C):
    g = torch.Generator().manual_seed(50)
    x = torch.round(torch.randn(N, H, W, C, generator=g) * 2) / 2  # halves: many ties away from 0
    hw = torch.arange(H).view(H, 1) + torch.arange(W).view(1, W)
    x[..., 0] = torch.where(hw % 2 == 0, torch.tensor(-0.0), torch.tensor(0.0))  # alternating -0.0 / +0.0
    x[..., 1] = -x[..., 1].abs() - 0.5  # all negative: a 0 padding would win every border window
    x = x.to(torch.bfloat16)
    clean = x.clone()
    if H >= 5 and W >= 5:
        x[0, H // 2, W // 2, 3] = float("nan")  # away from the borders
    x[N - 1, H - 1, W - 1, 5] = float("nan")  # at a corner
    return x, clean


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool3s2_matches_torch(shape):
    N, H, W, C = shape
    Pn, Qn = pooled(H), pooled(W)
    x, clean = pool_input(*shape)

    def fwd(t):
        y = torch.full((N, Pn, Qn, C), 7.0, device=DEV, dtype=torch.bfloat16)
        idx = torch.full((N, Pn, Qn, C), 0xEE, device=DEV, dtype=torch.uint8)
        call("avt_maxpool3s2_fwd", P(D(t)), P(y), P(idx), N, H, W, C, S())
        torch.cuda.synchronize()
        return y, idx

    for t in (x, clean):
        y, idx = fwd(t)
        yr, ind = F.max_pool2d(nchw(t.float()), 3, 2, 1, return_indices=True)
        assert same_bits_or_nan(y.cpu(), nhwc(yr).to(torch.bfloat16).contiguous())
        assert torch.equal(idx.cpu().long(), nhwc(window_pos(ind, H, W)).contiguous())
    # backward on the NaN-free input (idx is that of `clean`, just verified): every element, to one bf16 ulp (an
    # element is the sum of at most four bf16 values)
    g = torch.Generator().manual_seed(51)
    gy = torch.randn(N, Pn, Qn, C, generator=g).to(torch.bfloat16)
    gx = torch.full((N, H, W, C), 7.0, device=DEV, dtype=torch.bfloat16)
    call("avt_maxpool3s2_bwd", P(D(gy)), P(idx), P(gx), N, H, W, C, S())
    torch.cuda.synchronize()
    xn = nchw(clean.double()).clone().requires_grad_(True)
    F.max_pool2d(xn, 3, 2, 1).backward(nchw(gy.double()))
    ref = nhwc(xn.grad)
    err = (gx.cpu().double() - ref).abs()
    assert (err <= bf16_ulp(ref)).all(), (err / bf16_ulp(ref).clamp_min(1e-300)).max().item()
    with pytest.raises(RuntimeError):
        call("avt_maxpool3s2_fwd", P(D(x)), P(y), P(idx), N, H, W, 12, S())


# ------------------------------------------------------------------------------------------ fused stem
STEM_SHAPES = [(2, 12, 14, 64), (1, 7, 9, 64), (2, 9, 192, 64), (1, 3, 1, 64)]
STEM_SKIP_CAP = 0.02


def windows(t, pad):
    """[N][H][W][C] -> [N][C][9][P Q]: the 3x3 / stride 2 / pad 1 windows, position r * 3 + s along dim 2."""
    N, H, W, C = t.shape
    u = F.unfold(F.pad(nchw(t), (1, 1, 1, 1), value=pad), 3, stride=2)
    return u.view(N, C, 9, -1)


@functools.lru_cache(maxsize=None)
def stem_case(shape):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(24)
    k = types.SimpleNamespace()
    k.c = bc.bf16(1.5 * torch.randn(N, H, W, C, generator=g) - 0.3)
    k.gamma, k.beta = 2 + 0.02 * torch.randn(C, generator=g), 1.5 + 0.1 * torch.randn(C, generator=g)
    k.st = bc.batch_stats(k.c.reshape(-1, C), k.gamma, k.beta)
    r, T = bc.fwd_ref(k.c, k.st[0], k.st[1])
    k.r = r.relu()
    k.bound = bc.BF16_REL * k.r.abs() + bc.A_FWD * T
    # the independent reference: h in bf16 through fp64, then torch's pool
    k.h = bc.bf16(k.r.float())
    k.y, ind = F.max_pool2d(nchw(k.h.float()), 3, 2, 1, return_indices=True)
    k.idx = nhwc(window_pos(ind, H, W)).contiguous()
    # windows whose maximum is clear of the runner-up by more than the two elements' bounds
    top, ti = windows(k.r, float("-inf")).topk(2, dim=2)
    b = windows(k.bound, 0.0).gather(2, ti)
    clear = (top[:, :, 0] - top[:, :, 1]) > (b[:, :, 0] + b[:, :, 1])
    Pn, Qn = pooled(H), pooled(W)
    k.clear = nhwc(clear.view(N, C, Pn, Qn)).contiguous()
    k.argmax = nhwc(ti[:, :, 0].view(N, C, Pn, Qn)).contiguous()
    k.gen = g
    return k


@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_stem_fused_independent_reference(shape):
    N, H, W, C = shape
    Pn, Qn = pooled(H), pooled(W)
    k = stem_case(shape)
    # on the reference alone: few windows are skipped, and on the clear ones torch's first maximum is the maximum
    skipped = 1 - k.clear.double().mean().item()
    print(f"{shape}: {100 * skipped:.2f} % of the windows skipped")
    assert skipped <= STEM_SKIP_CAP
    assert torch.equal(k.idx[k.clear], k.argmax[k.clear])
    cd, st = D(k.c), D(k.st)
    y = torch.full((N, Pn, Qn, C), 7.0, device=DEV, dtype=torch.bfloat16)
    idx = torch.full((N, Pn, Qn, C), 0xEE, device=DEV, dtype=torch.uint8)
    carg = torch.full_like(y, 7.0)
    call("avt_stem_bn_relu_maxpool_fwd", P(cd), P(st[0]), P(st[1]), P(y), P(idx), P(carg), N, H, W, C, S())
    torch.cuda.synchronize()
    # y: |max_k h_k - max_k r_k| <= max_k |h_k - r_k|, so the window's bound is the largest of its elements' bounds
    ry = nhwc(F.max_pool2d(nchw(k.r), 3, 2, 1))
    by = nhwc(F.max_pool2d(nchw(k.bound), 3, 2, 1))
    err = (y.cpu().double() - ry).abs()
    print(f"{shape}: y worst error / bound {(err / by.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= by).all()
    ii = idx.cpu().long()
    assert ((ii >= 0) & (ii < 9)).all()
    assert torch.equal(ii[k.clear], k.idx[k.clear])
    # carg = c at the kernel's argmax, everywhere
    hh = 2 * torch.arange(Pn).view(1, Pn, 1, 1) - 1 + ii // 3
    ww = 2 * torch.arange(Qn).view(1, 1, Qn, 1) - 1 + ii % 3
    assert ((hh >= 0) & (hh < H) & (ww >= 0) & (ww < W)).all()
    nn_ = torch.arange(N).view(N, 1, 1, 1).expand_as(ii)
    cc = torch.arange(C).view(1, 1, 1, C).expand_as(ii)
    cat = k.c[nn_, hh, ww, cc]
    assert torch.equal(carg.cpu().view(torch.int16), cat.view(torch.int16))

    # backward: the pool routed through the kernel's own idx; gy correlated with xhat of the picked pre-activation
    g = torch.Generator().manual_seed(26)
    gy = bc.correlated_grad(cat.reshape(-1, C), k.st, g).view(N, Pn, Qn, C)
    rows = N * H * W
    ws = torch.full((int(query("avt_bn_bwd_workspace", rows, C)),), 255, device=DEV, dtype=torch.uint8)
    sg, sb = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dgamma, dbeta = D(sg), D(sb)
    gc = torch.full_like(cd, 777.0)
    call("avt_stem_maxpool_bn_relu_bwd", P(D(gy)), P(idx), P(carg), P(cd), P(st[0]), P(st[1]), P(st[2]), P(st[3]),
         P(D(k.gamma)), P(dgamma), P(dbeta), P(gc), P(ws), N, H, W, C, S())
    h = torch.full_like(cd, 7.0)
    call("avt_bn_apply", P(cd), P(st[0]), P(st[1]), None, None, None, P(h), rows, C, 1, S())
    torch.cuda.synchronize()
    mask = (h.cpu() > 0).reshape(rows, C)  # the ReLU mask as the kernels' forward expression stores it
    flat = ((nn_ * H + hh) * W + ww) * C + cc
    gfull = torch.zeros(rows * C, dtype=torch.float64).index_add_(0, flat.reshape(-1), gy.double().reshape(-1))
    gfull = gfull.view(rows, C)
    c2 = k.c.reshape(rows, C)
    ref = bc.bwd_eval(gfull, mask, c2, k.st, k.gamma)
    yard = bc.bwd_eval(gfull, mask, c2, k.st, k.gamma, torch.float32)
    # the kernel sums over the pooled grid, one term per window: the sums of absolute values of that form
    mpool = mask.reshape(-1)[flat.reshape(-1)].view(-1, C)
    gp = torch.where(mpool, gy.double().view(-1, C), torch.zeros((), dtype=torch.float64))
    ref.abs1, ref.abs2 = gp.abs().sum(0), (gp * bc.xhat_of(cat.reshape(-1, C), k.st)).abs().sum(0)
    # one input pixel in four receives a gradient, so the means are a quarter of bncheck's: VISIBLE / 4
    assert ref.k1.abs().max().item() >= bc.VISIBLE / 4 and ref.k2.abs().max().item() >= bc.VISIBLE / 4
    a, a_yard = bc.a_bwd(ref, yard)
    tag = f"stem bwd {shape}"
    print(f"{tag}: a_yard {a_yard:.2e} max|k1| {ref.k1.abs().max():.3f} max|k2| {ref.k2.abs().max():.3f}")
    bc.check_elements(tag + " gc", gc, ref.gc, ref.T, a)
    bc.check_sums(tag, dgamma, dbeta, ref, sg, sb)
    kk = ws[64:64 + 8 * C].cpu().view(torch.float32)
    okk, rk = bc.k_ok(kk[:C], kk[C:], ref, rows)
    print(f"{tag}: worst (k1, k2) error / bound {rk:.3f}")
    assert okk.all()


# ------------------------------------------------------------------------------------------ audio pool + normalize
# (B, HW, C, sample 0 all zeros); RG = 1024 / (C / 8) row groups, four rows per unrolled pass
AUDIO_CASES = [
    (3, 1, 512, False),                           # a one-row map
    (2, 16, 512, False), (2, 17, 512, True),      # RG = 16: one tail row per group; two rows in the first group only
    (2, 64, 512, False), (2, 65, 512, False),     # exactly one unrolled pass (4 RG); one more row
    (2, 9, 64, True),                             # the backward's slices: rps = 2, three of the eight empty
    (2, 128, 64, False), (2, 513, 64, False),     # RG = 128: tail only; unrolled + tail
    (2, 40, 128, False), (2, 40, 256, False),     # the two channel widths
]


@pytest.mark.parametrize("B,HW,C,zero0", AUDIO_CASES)
def test_audio_pool_norm_edges(B, HW, C, zero0):
    g = torch.Generator().manual_seed(60)
    # post-ReLU, quantised to quarters, small enough (values 0 .. 1.25) that most channels have a tied maximum
    a = torch.round((0.25 * torch.randn(B, HW, C, generator=g)).relu() * 4) / 4
    a[:, :, 2] = 0
    a[:, :, C - 1] = 0  # whole channels of zeros
    if zero0:
        a[0] = 0  # norm 0
    a = a.to(torch.bfloat16)
    gan = torch.randn(B, C, generator=g)
    an = torch.full((B, C), 7.0, device=DEV)
    amax = torch.full((B, C), -7, device=DEV, dtype=torch.int32)
    anorm = torch.full((B,), 7.0, device=DEV)
    ad = D(a)
    ga = torch.full_like(ad, 7.0)
    call("avt_audio_pool_norm_fwd", P(ad), P(an), P(amax), P(anorm), B, HW, C, S())
    call("avt_audio_pool_norm_bwd", P(D(gan)), P(an), P(amax), P(anorm), P(ga), B, HW, C, S())
    torch.cuda.synchronize()
    at = a.double().permute(0, 2, 1).reshape(B, C, HW, 1).clone().requires_grad_(True)
    pool, ind = F.adaptive_max_pool2d(at, 1, return_indices=True)
    pool, ind = pool.flatten(1), ind.flatten(1)
    r = F.normalize(pool, dim=1)
    r.backward(gan.double())
    norm = pool.detach().norm(dim=1)
    ties = (a.double() == pool.detach().view(B, 1, C)).sum(1) > 1
    print(f"({B}, {HW}, {C}): {100 * ties.double().mean().item():.0f} % of the channels have a tied maximum")
    assert HW < 9 or ties.double().mean().item() >= 0.5  # on the reference alone: the input does have the ties
    assert torch.equal(amax.cpu().long(), ind)
    assert (anorm.cpu().double() - norm).abs().max().item() <= 1e-6 * norm.abs().max().clamp_min(1e-30).item()
    assert (an.cpu().double() - r.detach()).abs().max().item() <= 1e-6 * r.detach().abs().max().clamp_min(1e-30).item()
    gref = at.grad.reshape(B, C, HW).permute(0, 2, 1)  # [B][HW][C]
    on = torch.zeros(B, HW, C, dtype=torch.bool).scatter_(1, ind.view(B, 1, C), True)
    got = ga.cpu().double()
    assert (got[~on] == 0).all()
    assert (gref[~on] == 0).all()
    rr = gref.gather(1, ind.view(B, 1, C)).view(B, C)
    gg = got.gather(1, ind.view(B, 1, C)).view(B, C)
    dot = (gan.double() * r.detach()).sum(1, keepdim=True)
    T = (gan.double().abs() + (r.detach() * dot).abs()) / norm.clamp_min(1e-12).view(B, 1)
    bound = bc.BF16_REL * rr.abs() + 2.0 ** -20 * T
    err = (gg - rr).abs()
    print(f"({B}, {HW}, {C}): ga worst error / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= bound).all()
    if zero0:
        # below F.normalize's eps the gradient is g / eps: on the reference, and bit for bit in the kernel (fp32
        # g / 1e-12f rounded to bf16; the fp64 quotient rounds to the same bf16 for these g, asserted first)
        assert norm[0].item() == 0 and (ind[0] == 0).all()
        want = gan[0].double() / 1e-12
        assert ((rr[0] - want).abs() <= 1e-12 * want.abs()).all()
        w32 = (gan[0] / torch.tensor(1e-12, dtype=torch.float32)).to(torch.bfloat16)
        assert torch.equal(w32, want.to(torch.bfloat16))
        assert torch.equal(ga[0, 0].cpu().view(torch.int16), w32.view(torch.int16))
