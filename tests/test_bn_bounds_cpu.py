"""The bounds of tests/bncheck.py bite: on simulated kernel outputs (CPU only), the fp32 yardstick rounded to bf16 lies
inside them and every fault a BN backward could plausibly have lies outside.

Measured here (seed of bncheck.make_case, masks of an fp32 forward): a_yard 1.6e-7 .. 3.3e-7; max|k1| 0.42 .. 0.60,
max|k2| 0.43 .. 0.68; share of gc elements outside the bound with k1 dropped 100 %, with k2 dropped 99.6 .. 99.8 %.

k1 and k2 divided by rows - 1 moves gc by 1 / (rows - 1) of the mean terms.  At 198 rows that is above the bf16
rounding (71 .. 81 % of the elements outside); at 8197 rows it is 1.2e-4 of them, a thirtieth of the 2^-8 that any bf16
output is allowed, and only 2 .. 4 % of the elements leave the bound -- no bound on a bf16 gc can see it there.  The
kernels keep k1, k2 as fp32 in their workspace, so the tests bound those as well (bncheck.k_ok: the sum bound divided
by rows, plus the fp32 rounding of the quotient), and that bound sees the wrong divisor in every channel at any row
count."""
import pytest
import torch

import bncheck as bc

SHAPES = [(198, 64), (8197, 512)]
_CACHE = {}


def _fwd32(x, st, res=None, st2=None):
    """bf16 relu(x scale + shift [+ res rscale + rshift | + res]) in fp32: a stand-in for the kernel's stored output,
    which the masks are taken from."""
    f = x.float() * st[0] + st[1]
    if res is not None:
        f = f + (res.float() * st2[0] + st2[1] if st2 is not None else res.float())
    return bc.bf16(f.relu())


def _case(shape):
    if shape not in _CACHE:
        k = bc.make_case(*shape)
        k.y = _fwd32(k.c, k.st)
        k.y_res = _fwd32(k.c, k.st, k.cd)
        k.y_two = _fwd32(k.c, k.st, k.cd, k.st2)
        _CACHE[shape] = k
    return _CACHE[shape]


def _targets(k):
    """name -> (gy, mask, x, stats, gamma): every (entry, BN) pair of the GPU tests."""
    return {
        "bn": (k.gy, None, k.c, k.st, k.gamma),
        "relu": (k.gy, k.y > 0, k.c, k.st, k.gamma),
        "res": (k.gy, k.y_res > 0, k.c, k.st, k.gamma),
        "two-a": (k.gy2, k.y_two > 0, k.c, k.st, k.gamma),
        "two-b": (k.gy2, k.y_two > 0, k.cd, k.st2, k.gamma2),
    }


NAMES = ["bn", "relu", "res", "two-a", "two-b"]


def _ref_yard(k, name):
    gy, mask, x, st, gm = _targets(k)[name]
    ref = bc.bwd_eval(gy, mask, x, st, gm)
    yard = bc.bwd_eval(gy, mask, x, st, gm, torch.float32)
    a, a_yard = bc.a_bwd(ref, yard)
    return ref, yard, a, a_yard


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", SHAPES)
def test_yardstick_inside_and_inputs_visible(shape, name):
    k = _case(shape)
    ref, yard, a, a_yard = _ref_yard(k, name)
    k1, k2 = bc.assert_visible(ref, k.rows, name)
    bad, ratio = bc.outside(bc.bf16(yard.gc), ref.gc, ref.T, a)
    print(f"{shape} {name}: max|k1| {k1:.3f} max|k2| {k2:.3f} a_yard {a_yard:.2e} yardstick worst ratio {ratio:.3f}")
    assert not bad.any()
    assert a_yard < 2.0 ** -20  # fp32 arithmetic: a few roundings of 2^-24 each
    assert bc.sums_ok(yard.dbeta, ref.dbeta, ref.abs1)[0].all()
    assert bc.sums_ok(yard.dgamma, ref.dgamma, ref.abs2)[0].all()
    okk, _ = bc.k_ok(yard.k1, yard.k2, ref, k.rows)
    assert okk.all()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fault", ["drop_k1", "drop_k2", "rows_minus_1"])
def test_k_faults_leave_the_bound(fault, shape, name):
    k = _case(shape)
    gy, mask, x, st, gm = _targets(k)[name]
    ref, _, a, _ = _ref_yard(k, name)
    f = bc.bwd_eval(gy, mask, x, st, gm, torch.float32, fault=fault)
    bad, _ = bc.outside(bc.bf16(f.gc), ref.gc, ref.T, a)
    share = bad.double().mean().item()
    okk, _ = bc.k_ok(f.k1, f.k2, ref, k.rows)
    kshare = (~okk).double().mean().item()
    print(f"{shape} {name} {fault}: {100 * share:.1f} % of gc outside, {100 * kshare:.1f} % of channels' (k1, k2)")
    if fault == "rows_minus_1":
        # (k1, k2) themselves: every channel, at any row count; gc: where 1 / (rows - 1) clears the bf16 rounding
        assert kshare >= 0.5
        if k.rows <= 198:
            assert share >= 0.5
    else:
        assert share >= 0.5


@pytest.mark.parametrize("shape", SHAPES)
def test_sum_faults_leave_the_bound(shape):
    k = _case(shape)
    for name in NAMES:
        gy, mask, x, st, gm = _targets(k)[name]
        ref, _, a, _ = _ref_yard(k, name)
        # the last row left out of both sums
        f = bc.bwd_eval(gy, mask, x, st, gm, torch.float32, fault="skip_last_row")
        assert not (bc.sums_ok(f.dbeta, ref.dbeta, ref.abs1)[0].all() and
                    bc.sums_ok(f.dgamma, ref.dgamma, ref.abs2)[0].all()), name
        if mask is None:
            continue
        # the mask taken as y >= 0 (every element of a ReLU output: no mask at all)
        f = bc.bwd_eval(gy, torch.ones_like(mask), x, st, gm, torch.float32)
        assert not bc.sums_ok(f.dbeta, ref.dbeta, ref.abs1)[0].all(), name
        assert not bc.sums_ok(f.dgamma, ref.dgamma, ref.abs2)[0].all(), name
    # the second BN's k2 summed with the first BN's xhat
    gy, mask, x, st, gm = _targets(k)["two-b"]
    ref, _, a, _ = _ref_yard(k, "two-b")
    f = bc.bwd_eval(gy, mask, x, st, gm, torch.float32, xhat_k2=bc.xhat_of(k.c, k.st))
    bad, _ = bc.outside(bc.bf16(f.gc), ref.gc, ref.T, a)
    assert bad.any() and not bc.sums_ok(f.dgamma, ref.dgamma, ref.abs2)[0].all()
    assert bad.double().mean().item() >= 0.5


@pytest.mark.parametrize("shape", SHAPES)
def test_formula_is_the_autograd_of_batch_norm(shape):
    """bncheck's r (the kernel's formula on the fp32 statistics, in fp64) against the fp64 F.batch_norm autograd of
    the same graph: they differ by the fp32 rounding of mean and invstd alone, < 2^-22 T (and the sums by as much
    of their sums of absolute values)."""
    k = _case(shape)
    t = _targets(k)

    def close(name, gc, dgamma, dbeta):
        ref = _ref_yard(k, name)[0]
        assert ((gc - ref.gc).abs() <= 2.0 ** -22 * ref.T).all(), name
        assert ((dbeta - ref.dbeta).abs() <= 2.0 ** -22 * ref.abs1).all(), name
        assert ((dgamma - ref.dgamma).abs() <= 2.0 ** -22 * (ref.abs1 + ref.abs2)).all(), name

    close("bn", *bc.bwd_autograd("bn", k.gy, None, k.c, k.gamma, k.beta))
    close("relu", *bc.bwd_autograd("relu", k.gy, t["relu"][1], k.c, k.gamma, k.beta))
    gc, dg, db, gcd = bc.bwd_autograd("res", k.gy, t["res"][1], k.c, k.gamma, k.beta, k.cd)
    close("res", gc, dg, db)
    assert torch.equal(gcd, bc.bwd_eval(k.gy, t["res"][1], k.c, k.st, k.gamma).gp)  # the residual gets g'
    gc, dg, db, gcd, dg2, db2 = bc.bwd_autograd("two", k.gy2, t["two-a"][1], k.c, k.gamma, k.beta, k.cd, k.gamma2,
                                                k.beta2)
    close("two-a", gc, dg, db)
    close("two-b", gcd, dg2, db2)
