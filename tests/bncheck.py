"""BatchNorm checks shared by tests/test_bn_bounds_cpu.py, tests/test_bn_edges_gpu.py and tests/test_pool_edges_gpu.py:
inputs that make the mean terms of the BN backward visible, the fp64 references, their fp32 CPU yardstick, and bounds
per ELEMENT (a whole-tensor max|a - b| / max|b| cannot see k1 = mean(g') and k2 = mean(g' xhat): with an upstream
gradient independent of the activations both shrink like 1 / sqrt(rows), and a backward that drops them passes).

Inputs.  c as the first-generation tests build it, bf16(1.3 randn - 0.2); the upstream gradient is correlated with
the activations, gy = bf16(0.5 randn + 0.6 xhat + 0.4) per channel, so k1 and k2 are O(0.5) at every row count.
assert_visible() asserts max|k1| and max|k2| over the channels >= 0.25 on the reference alone.  (One row is the
exception for k2 only: its xhat is identically 0, so k2 = 0 whatever the gradient.)

Reference r.  The fp64 value of the kernel's own formula on the kernel's own inputs: the bf16 tensors and the fp32
(scale, shift, mean, invstd) it is handed, widened.  bwd_autograd() is the fp64 F.batch_norm autograd of the same
graph (its statistics are the fp64 batch statistics, not their fp32 roundings: it differs from r by < 2^-22 T, which
test_bn_bounds_cpu.py asserts).  The ReLU mask is always the one the kernel stored (its bf16 output or its mask
bits): the comparison is about arithmetic, not about a sign decision at a rounding boundary.

Element bound.  |out - r| <= 2^-8 |r| + a T.  2^-8 |r| is the round-to-nearest into bf16 (8 significant bits); T is
the sum of the absolute values of the summands,
    forward : |x scale| + |shift| (+ |res rscale| + |rshift|, or + |res|)
    backward: |gamma invstd| (|g'| + |k1| + |xhat k2|),
so that a T covers what fp32 arithmetic can lose where the summands cancel.  Forward a = 2^-22: four fp32 roundings
(the fma, the residual's product, its two additions), each <= 2^-24 of a partial sum that T bounds -- derived.
Backward a = max(4 a_yard, 2^-20), a_yard the largest |yard - r| / T of a torch fp32 CPU evaluation of the same
formula before the bf16 rounding (k1, k2 by fp32 torch.sum): measured per case on the CPU, never from the kernel.

Sum bound.  |dbeta - ref| <= 2^-15 sum|g'| and |dgamma - ref| <= 2^-15 sum|g' xhat| per channel: the longest fp32
chain of either reduce kernel at the cases of these tests is under 272 terms (<= 16 rows per thread, then the
<= 256 = rstep partials of the block), recursive summation costs < 272 * 2^-24 < 2^-15 of the sum of absolute values,
and from the block sums on everything is fp64.  The entries ADD the sums into fp32 gradients: that one addition
rounds to nearest, <= 2^-24 |start + ref| more (sums_ok's `start`).  A case with a longer per-thread chain has to
recompute this from its own rows and C."""
import types

import torch
import torch.nn.functional as F

EPS = 1e-5
BF16_REL = 2.0 ** -8
A_FWD = 2.0 ** -22
A_BWD_MIN = 2.0 ** -20
SUM_REL = 2.0 ** -15
ADD_REL = 2.0 ** -24
VISIBLE = 0.25


def bf16(t):
    return t.to(torch.bfloat16)


def batch_stats(c, gamma, beta):
    """fp32 [4][C] (scale, shift, mean, invstd) of train-mode BN over the rows of c [rows][C], as avt_bn_finalize
    makes them."""
    x = c.double()
    mean = x.mean(0)
    inv = (x.var(0, unbiased=False) + EPS).rsqrt()
    scale = (gamma.double() * inv).float()
    shift = (beta.double() - mean * scale.double()).float()
    return torch.stack([scale, shift, mean.float(), inv.float()])


def xhat_of(x, st):
    """fp64 (x - mean) invstd with the fp32 statistics the kernel gets."""
    return (x.double() - st[2].double()) * st[3].double()


def make_case(rows, C, seed=0):
    """c, a second pre-activation cd (the downsample branch / the residual), their BN parameters and fp32 statistics,
    and the correlated upstream gradient gy; all [rows][C], CPU."""
    g = torch.Generator().manual_seed(1000 + seed)
    k = types.SimpleNamespace(rows=rows, C=C)
    k.c = bf16(torch.randn(rows, C, generator=g) * 1.3 - 0.2)
    k.cd = bf16(torch.randn(rows, C, generator=g) * 0.9 + 0.1)
    k.gamma, k.beta = 1 + 0.02 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    k.gamma2, k.beta2 = 1 + 0.02 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    k.st, k.st2 = batch_stats(k.c, k.gamma, k.beta), batch_stats(k.cd, k.gamma2, k.beta2)
    k.gy = correlated_grad(k.c, k.st, g)
    # the two-BN block's gradient carries the same 0.6 xhat of its second BN, so that BN's k2 is visible too
    # (with the first BN's xhat alone, max|k2| of the second is 0.15 .. 0.23)
    k.gy2 = bf16(k.gy.float() + 0.6 * xhat_of(k.cd, k.st2).float())
    return k


def correlated_grad(c, st, gen):
    """bf16(0.5 randn + 0.6 xhat + 0.4): E[g'] and E[g' xhat] stay O(0.5) however many rows there are."""
    return bf16(0.5 * torch.randn(c.shape, generator=gen) + 0.6 * xhat_of(c, st).float() + 0.4)


# ---------------------------------------------------------------------------------------------- forward
def fwd_ref(x, scale, shift, res=None, rscale=None, rshift=None):
    """(r, T) of x scale + shift (+ res rscale + rshift | + res) BEFORE the ReLU, fp64; relu(r) is the reference of a
    relu call (|relu(a) - relu(b)| <= |a - b|, so T serves both)."""
    a, b = x.double() * scale.double(), shift.double().expand(x.shape)
    r, T = a + b, a.abs() + b.abs()
    if res is not None:
        if rscale is not None:
            ra, rb = res.double() * rscale.double(), rshift.double().expand(x.shape)
            r, T = r + (ra + rb), T + ra.abs() + rb.abs()
        else:
            r, T = r + res.double(), T + res.double().abs()
    return r, T


# ---------------------------------------------------------------------------------------------- backward
def bwd_eval(g, mask, x, st, gamma, dtype=torch.float64, fault=None, xhat_k2=None):
    """gc = gamma invstd (g' - k1 - xhat k2), g' = g mask (mask: bool or None), in `dtype` on the bf16 inputs and the
    fp32 statistics st; fp64 is the reference r, fp32 (sums by torch.sum) its yardstick.  fault (test_bn_bounds_cpu.py's
    simulated kernels): "drop_k1", "drop_k2", "rows_minus_1" (k1, k2 divided by rows - 1), "skip_last_row" (the last
    row left out of both sums); xhat_k2: k2 summed with another BN's xhat.  Returns a namespace: gc (unrounded), T,
    gp, xhat, k1, k2, dbeta, dgamma and the sums of absolute values abs1, abs2."""
    rows = x.shape[0]
    mean, inv, gm = st[2].to(dtype), st[3].to(dtype), gamma.to(dtype)
    gp = g.to(dtype) if mask is None else torch.where(mask, g.to(dtype), torch.zeros((), dtype=dtype))
    xh = (x.to(dtype) - mean) * inv
    p1, p2 = gp, gp * (xh if xhat_k2 is None else xhat_k2.to(dtype))
    if fault == "skip_last_row":
        p1, p2 = p1[:-1], p2[:-1]
    o = types.SimpleNamespace(gp=gp, xhat=xh)
    o.dbeta, o.dgamma = torch.sum(p1, 0), torch.sum(p2, 0)
    o.abs1, o.abs2 = torch.sum(p1.abs(), 0), torch.sum(p2.abs(), 0)
    n = rows - 1 if fault == "rows_minus_1" else rows
    o.k1, o.k2 = o.dbeta / n, o.dgamma / n
    k1 = torch.zeros_like(o.k1) if fault == "drop_k1" else o.k1
    k2 = torch.zeros_like(o.k2) if fault == "drop_k2" else o.k2
    gi = gm * inv
    o.gc = gi * (gp - k1 - xh * k2)
    o.T = gi.abs() * (gp.abs() + k1.abs() + (xh * k2).abs())
    return o


def assert_visible(ref, rows, tag=""):
    """The precondition of the element bound, on the reference alone: the mean terms are large."""
    k1, k2 = ref.k1.abs().max().item(), ref.k2.abs().max().item()
    assert k1 >= VISIBLE, (tag, "max|k1|", k1)
    if rows > 1:  # one row: xhat = 0 identically, k2 = 0 for any gradient
        assert k2 >= VISIBLE, (tag, "max|k2|", k2)
    return k1, k2


def a_bwd(ref, yard):
    """(a, a_yard): the backward's a = max(4 a_yard, 2^-20), a_yard = max |yard - r| / T over the elements."""
    d = (yard.gc.double() - ref.gc).abs()
    a_yard = torch.where(ref.T > 0, d / ref.T.clamp_min(1e-300), d * 1e300).max().item()
    return max(4 * a_yard, A_BWD_MIN), a_yard


def outside(out, r, T, a):
    """(mask of the elements of out outside 2^-8 |r| + a T, the largest |out - r| / bound).  NaN is outside."""
    err = (out.double().cpu() - r).abs()
    bound = BF16_REL * r.abs() + a * T
    bad = ~(err <= bound)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, err * 1e300, err))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    return bad, (ratio.max().item() if ratio.numel() else 0.0)


def check_elements(tag, out, r, T, a):
    """Assert every element of out within the bound; prints and returns the worst error / bound."""
    bad, ratio = outside(out.reshape(r.shape), r, T, a)
    print(f"{tag}: worst |out - r| / bound {ratio:.3f}  (a = {a:.3e})")
    assert not bad.any(), (tag, "outside the bound:", int(bad.sum()), "of", bad.numel(), "worst ratio", ratio)
    return ratio


def sums_ok(got, ref_sum, ref_abs, start=None):
    """(per-channel mask of got within SUM_REL ref_abs (+ the fp32 addition into `start`), worst error / bound)."""
    want = ref_sum if start is None else start.double() + ref_sum
    bound = SUM_REL * ref_abs + (0 if start is None else ADD_REL * want.abs())
    err = (got.double().cpu() - want).abs()
    ok = err <= bound
    ratio = torch.nan_to_num(torch.where(bound > 0, err / bound.clamp_min(1e-300), err * 1e300), nan=float("inf"))
    return ok, ratio.max().item()


def check_sums(tag, dgamma, dbeta, ref, start_dgamma=None, start_dbeta=None):
    okb, rb = sums_ok(dbeta, ref.dbeta, ref.abs1, start_dbeta)
    okg, rg = sums_ok(dgamma, ref.dgamma, ref.abs2, start_dgamma)
    print(f"{tag}: worst dbeta error / bound {rb:.3f}, dgamma {rg:.3f}")
    assert okb.all() and okg.all(), (tag, "dbeta ratio", rb, "dgamma ratio", rg)
    return max(rb, rg)


def k_ok(k1, k2, ref, rows):
    """(per-channel mask of the fp32 (k1, k2) a kernel keeps within the sum bound / rows + their fp32 rounding, worst
    error / bound).  A gc in bf16 cannot show a relative error of 1 / rows in them once rows >> 2^8; this does."""
    ok, worst = None, 0.0
    for got, want, sabs in ((k1, ref.k1, ref.abs1), (k2, ref.k2, ref.abs2)):
        bound = SUM_REL * sabs / rows + ADD_REL * want.abs()
        err = (got.double().cpu() - want).abs()
        o = err <= bound
        ok = o if ok is None else ok & o
        ratio = torch.nan_to_num(torch.where(bound > 0, err / bound.clamp_min(1e-300), err * 1e300), nan=float("inf"))
        worst = max(worst, ratio.max().item())
    return ok, worst


def bwd_autograd(form, gy, mask, c, gamma, beta, cd=None, gamma2=None, beta2=None):
    """fp64 F.batch_norm autograd of  bn(c) ("bn"),  relu(bn(c)) ("relu"),  relu(bn2(c) + cd) ("res") or
    relu(bn2(c) + bnd(cd)) ("two"), the ReLU given as its mask (a constant 0/1 factor has the ReLU's gradient).
    Returns (gc, dgamma, dbeta[, gcd, dgamma2, dbeta2]); tensors are [rows][C]."""
    def leaf(t):
        return t.double().clone().requires_grad_(True)

    def bn(x, g_, b_):  # [rows][C] is (N, C): batch statistics over the rows
        return F.batch_norm(x, None, None, g_, b_, True, 0.1, EPS)

    x, gm, bt = leaf(c), leaf(gamma), leaf(beta)
    y = bn(x, gm, bt)
    leaves = [x, gm, bt]
    if form == "res":
        xd = leaf(cd)
        y = y + xd
        leaves.append(xd)
    elif form == "two":
        xd, gm2, bt2 = leaf(cd), leaf(gamma2), leaf(beta2)
        y = y + bn(xd, gm2, bt2)
        leaves += [xd, gm2, bt2]
    if form != "bn":
        y = y * mask.double()
    y.backward(gy.double())
    return [t.grad for t in leaves]
