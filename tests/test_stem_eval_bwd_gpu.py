"""``avt_stem_maxpool_bn_relu_eval_bwd``: the stem backward (MaxPool2d(3,2,1) -> ReLU -> bn1) under running
statistics, one pass from the pooled gradient gy [N,P,Q,C] to gc [N,H,W,C].

idx and carg come from a real ``avt_stem_bn_relu_maxpool_fwd`` on running statistics; idx is decoded as
tests/test_pool_edges_gpu.py decodes it (window position r*3+s -> input pixel (2p-1+r, 2q-1+s)).  The reference is built
in fp64 on the CPU from the decoded idx: gfull = scatter-add of gy onto the selected pixels, g' = gfull * mask (the ReLU
mask as the kernels' forward expression stores it: avt_bn_apply's output > 0), gc = gamma invstd g'; the sums run over
the pooled rows, one term per window, dbeta = sum gy*mask, dgamma = sum gy*mask*(carg - mean) invstd.

Bounds (tests/bncheck.py).  Element: |gc - r| <= 2^-8 |r| + a T, T = |gamma invstd| * scatter-add of |gy| * mask,
a = max(4 a_yard, 2^-20) with a_yard from a torch fp32 CPU evaluation of the same formula.  Sum: 2^-15 of the sum of
absolute values (at these shapes a block's thread sums one pooled row, then the block's <= 32 partials: far under the
272-term chain that rule allows) + the one fp32 addition into the pre-filled gradient.

Every fifth gamma is negative, so a pixel with g' = 0 would come out as -0 if the kernel merely multiplied: it must be
exactly +0 where no window selects the pixel.

Measured on one MI355X: gc at most 0.91-0.995 of its bound (the bf16 rounding itself; a = 2^-20 at every shape), dbeta /
dgamma at most 0.009 / 0.073 of theirs."""
import ctypes

import pytest
import torch

import bncheck as bc
from avt_amd._lib import call, query

pytestmark = pytest.mark.gpu
DEV = "cuda"
_KEEP = []

SHAPES = [(1, 1, 1), (2, 7, 9), (1, 33, 38), (2, 32, 32)]
C = 64


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


@pytest.mark.parametrize("shape", SHAPES)
def test_stem_eval_bwd(shape):
    N, H, W = shape
    Pn, Qn = pooled(H), pooled(W)
    rows = N * H * W
    g = torch.Generator().manual_seed(240 + H)
    c = bc.bf16(1.5 * torch.randn(N, H, W, C, generator=g) - 0.3)
    gamma, beta = 2 + 0.02 * torch.randn(C, generator=g), 1.5 + 0.1 * torch.randn(C, generator=g)
    gamma[::5] = -gamma[::5]
    rm, rv = 0.3 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    inv = torch.rsqrt(rv + bc.EPS)
    scale = gamma * inv
    st = torch.stack([scale, beta - rm * scale, rm, inv])  # as trunk._bn_finalize(training=False)
    cd, std, gam = D(c), D(st), D(gamma)
    y = torch.full((N, Pn, Qn, C), 7.0, device=DEV, dtype=torch.bfloat16)
    idx = torch.full((N, Pn, Qn, C), 0xEE, device=DEV, dtype=torch.uint8)
    carg = torch.full_like(y, 7.0)
    call("avt_stem_bn_relu_maxpool_fwd", P(cd), P(std[0]), P(std[1]), P(y), P(idx), P(carg), N, H, W, C, S())
    h = torch.full_like(cd, 7.0)
    call("avt_bn_apply", P(cd), P(std[0]), P(std[1]), None, None, None, P(h), rows, C, 1, S())
    torch.cuda.synchronize()
    ii = idx.cpu().long()
    assert ((ii >= 0) & (ii < 9)).all()
    hh = 2 * torch.arange(Pn).view(1, Pn, 1, 1) - 1 + ii // 3
    ww = 2 * torch.arange(Qn).view(1, 1, Qn, 1) - 1 + ii % 3
    assert ((hh >= 0) & (hh < H) & (ww >= 0) & (ww < W)).all()
    nn_ = torch.arange(N).view(N, 1, 1, 1).expand_as(ii)
    cc = torch.arange(C).view(1, 1, 1, C).expand_as(ii)
    cat = c[nn_, hh, ww, cc]
    assert torch.equal(carg.cpu().view(torch.int16), cat.view(torch.int16))
    mask = (h.cpu() > 0).reshape(rows, C)
    assert mask.any() and (~mask).any()
    flat = (((nn_ * H + hh) * W + ww) * C + cc).reshape(-1)

    gy = bc.correlated_grad(cat.reshape(-1, C), st, g).view(N, Pn, Qn, C)
    gy64 = gy.double().reshape(-1)
    gfull = torch.zeros(rows * C, dtype=torch.float64).index_add_(0, flat, gy64).view(rows, C)
    gabs = torch.zeros(rows * C, dtype=torch.float64).index_add_(0, flat, gy64.abs()).view(rows, C)
    selected = torch.zeros(rows * C, dtype=torch.bool).index_fill_(0, flat, True).view(rows, C)
    gi = gamma.double() * inv.double()
    zero = torch.zeros((), dtype=torch.float64)
    r = gi * torch.where(mask, gfull, zero)
    T = gi.abs() * torch.where(mask, gabs, zero)
    yard = (gamma * inv) * torch.where(mask, gfull.float(), torch.zeros(()))  # the fp32 yardstick of the same formula
    d = (yard.double() - r).abs()
    a_yard = torch.where(T > 0, d / T.clamp_min(1e-300), d * 1e300).max().item()
    a = max(4 * a_yard, bc.A_BWD_MIN)
    # the sums, over the pooled rows (one term per window)
    mpool = mask.reshape(-1)[flat].view(-1, C)
    gp = torch.where(mpool, gy.double().view(-1, C), zero)
    xh = bc.xhat_of(cat.reshape(-1, C), st)
    ref = type("R", (), {})()
    ref.dbeta, ref.dgamma = gp.sum(0), (gp * xh).sum(0)
    ref.abs1, ref.abs2 = gp.abs().sum(0), (gp * xh).abs().sum(0)
    # the two forms of the sums agree (pooled rows vs input pixels), on the reference alone
    full = torch.where(mask, gfull, zero)
    assert torch.allclose(full.sum(0), ref.dbeta, rtol=1e-12, atol=1e-12)
    assert torch.allclose((full * bc.xhat_of(c.reshape(rows, C), st)).sum(0), ref.dgamma, rtol=1e-12, atol=1e-12)

    sg, sb = torch.randn(C, generator=g), torch.randn(C, generator=g)
    gyd = D(gy)

    def run(with_params):
        gc = torch.full_like(cd, float("nan"))
        dg = db = ws = None
        if with_params:
            dg, db = D(sg), D(sb)
            ws = torch.full((int(query("avt_bn_bwd_workspace", rows, C)),), 255, device=DEV, dtype=torch.uint8)
        call("avt_stem_maxpool_bn_relu_eval_bwd", P(gyd), P(idx), P(carg) if with_params else None, P(cd), P(std[0]),
             P(std[1]), P(std[2]) if with_params else None, P(std[3]), P(gam), P(dg), P(db), P(gc), P(ws), N, H, W, C,
             S())
        torch.cuda.synchronize()
        return gc, dg, db

    tag = f"stem eval bwd {shape}"
    gc, dg, db = run(True)
    print(f"{tag}: a_yard {a_yard:.2e}; {100 * selected.double().mean().item():.1f} % of the pixels selected")
    bc.check_elements(tag + " gc", gc.reshape(rows, C), r, T, a)
    bc.check_sums(tag, dg, db, ref, sg, sb)
    # a pixel no window selects: exactly +0 (the bits), whatever gamma's sign
    bits = gc.cpu().view(torch.int16).reshape(rows, C)
    assert (bits[~selected] == 0).all(), tag
    if rows > 1:
        assert (~selected).any() and (~selected)[:, ::5].any()
    gc2, dg2, db2 = run(True)
    assert torch.equal(bits, gc2.cpu().view(torch.int16).reshape(rows, C)), tag
    assert torch.equal(dg, dg2) and torch.equal(db, db2), tag
    gc3, _, _ = run(False)  # NULL dgamma / dbeta: no workspace, carg and mean not read
    assert torch.equal(bits, gc3.cpu().view(torch.int16).reshape(rows, C)), tag


def test_stem_eval_bwd_refusals():
    """The train-mode entry's shape limits, and parameter gradients without a workspace."""
    N, H, W = 1, 2, 2
    z16 = lambda *s: torch.zeros(*s, device=DEV, dtype=torch.bfloat16)
    gy, idx, c, gc = z16(N, 1, 1, C), torch.zeros(N, 1, 1, C, device=DEV, dtype=torch.uint8), z16(N, H, W, C), z16(N, H, W, C)
    v = torch.ones(4, C, device=DEV)
    dg = torch.zeros(C, device=DEV)
    args = lambda Wn, Cn, dgamma: ("avt_stem_maxpool_bn_relu_eval_bwd", P(gy), P(idx), P(gy), P(c), P(v[0]), P(v[1]),
                                   P(v[2]), P(v[3]), P(v[0]), P(dgamma), None, P(gc), None, N, H, Wn, Cn, S())
    call(*args(W, C, None))  # the frozen form needs no workspace
    with pytest.raises(RuntimeError):
        call(*args(W, C, dg))  # dgamma wanted, no workspace
    with pytest.raises(RuntimeError):
        call(*args(4096, C, None))  # too wide
    with pytest.raises(RuntimeError):
        call(*args(W, 60, None))  # unsupported channel count
