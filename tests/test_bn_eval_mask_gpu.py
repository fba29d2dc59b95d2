"""``avt_bn_eval_bwd_mask``: the running-statistics BatchNorm backward of a 2-D block output, g' = g * the mask bits
of ``avt_bn_apply_mask`` ([rows][C/8] u8, bit e of byte j is channel 8j+e).

Two references.  (1) The sibling ``avt_bn_eval_bwd(y = out)``: the rows are dealt to blocks and threads identically and
the sums ordered identically, so with bits = [out > 0] every output -- gc, gc2, dgamma, dbeta -- is the SAME BITS.
(2) Independently of the sibling, fp64 autograd through ``F.batch_norm(training=False)`` at test_r3d_eval_grad_gpu's
bounds (tests/bncheck.py: an element within one bf16 rounding of the fp64 value + a T, a = max(4 a_yard, 2^-20); a sum
within 2^-15 of its sum of absolute values + the one fp32 addition into the pre-filled gradient), once with the bits of
[out > 0] and once with random bits unrelated to out: the bits, not out, drive the result.

Rows 1, 31, 300, 4097 sit on either side of the row-dealing switches (one row; fewer rows than a block's row step;
several blocks; a ragged last block)."""
import ctypes
import types

import pytest
import torch

import bncheck as bc
from avt_amd._lib import BnBwdTarget, call, query
from test_r3d_eval_grad_gpu import _ref, _running_stats

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
_KEEP = []


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _KEEP.clear()


def D(t):
    t = t.to(DEV)
    _KEEP.append(t)
    return t


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def pack_bits(mask):
    """bool [rows][C] -> u8 [rows][C/8]: bit e of byte j = mask[.][8j+e] (avt_bn_apply_mask's layout)."""
    rows, C = mask.shape
    w = (1 << torch.arange(8)).view(1, 1, 8)
    return (mask.view(rows, C // 8, 8).long() * w).sum(-1).to(torch.uint8)


def _target(xc, st, gamma, dgamma, dbeta, rows, C):
    t = BnBwdTarget()
    gc = torch.full((rows, C), float("nan"), device=DEV, dtype=torch.bfloat16)
    _KEEP.append(gc)
    t.xc, t.mean, t.invstd, t.gamma, t.gc = xc.data_ptr(), st[2].data_ptr(), st[3].data_ptr(), gamma.data_ptr(), gc.data_ptr()
    if dgamma is not None:
        ws = torch.full(((int(query("avt_bn_bwd_workspace", rows, C)) + 7) // 8,), float("nan"), device=DEV,
                        dtype=torch.float64)  # any contents
        _KEEP.append(ws)
        t.dgamma, t.dbeta, t.workspace = dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr()
    return t, gc


@pytest.mark.parametrize("C", [64, 128, 512])
@pytest.mark.parametrize("rows", [1, 31, 300, 4097])
def test_bn_eval_bwd_mask(rows, C):
    k = bc.make_case(rows, C, seed=rows + C)
    gen = torch.Generator().manual_seed(7 + rows + C)
    st, rm, rv = _running_stats(k.gamma, k.beta, gen)
    st2, rm2, rv2 = _running_stats(k.gamma2, k.beta2, gen)
    # a block output relu(bn2(c) + bnd(cd)) stored in bf16, as test_r3d_eval_grad_gpu.test_bn_eval_bwd builds it
    pre = k.c.double() * st[0].double() + st[1].double()
    out = (pre + k.cd.double() * st2[0].double() + st2[1].double()).clamp_min(0).to(torch.bfloat16)
    mask_out = out > 0
    assert mask_out.any() and (~mask_out).any()
    mask_rnd = torch.rand(rows, C, generator=gen) < 0.5
    assert mask_rnd.any() and (~mask_rnd).any() and not torch.equal(mask_rnd, mask_out)
    g, c, cd, y = D(k.gy), D(k.c), D(k.cd), D(out)
    bits_out, bits_rnd = D(pack_bits(mask_out)), D(pack_bits(mask_rnd))
    std, st2d, gam, gam2 = D(st), D(st2), D(k.gamma), D(k.gamma2)

    def run(entry, mk, two, with_params):
        dg, db = (torch.full((4, C), 0.25, device=DEV).unbind(0)[:2] if with_params else (None, None))
        dg2, db2 = (torch.full((4, C), 0.25, device=DEV).unbind(0)[2:] if with_params else (None, None))
        t1, gc1 = _target(c, std, gam, dg, db, rows, C)
        t2 = gc2 = None
        if two:
            t2, gc2 = _target(cd, st2d, gam2, dg2, db2, rows, C)
        if entry == "mask":
            call("avt_bn_eval_bwd_mask", g.data_ptr(), mk.data_ptr(), ctypes.byref(t1),
                 ctypes.byref(t2) if two else None, rows, C, S())
        else:  # the sibling, masking from the stored output
            call("avt_bn_eval_bwd", g.data_ptr(), mk.data_ptr(), None, None, ctypes.byref(t1),
                 ctypes.byref(t2) if two else None, None, rows, C, S())
        torch.cuda.synchronize()
        return types.SimpleNamespace(gc=gc1, gc2=gc2, dg=dg, db=db, dg2=dg2, db2=db2)

    def same(a, b, tag, sums=True):
        assert torch.equal(a.gc.view(torch.int16), b.gc.view(torch.int16)), tag
        if a.gc2 is not None:
            assert torch.equal(a.gc2.view(torch.int16), b.gc2.view(torch.int16)), tag
        if sums:
            assert torch.equal(a.dg, b.dg) and torch.equal(a.db, b.db), tag
            if a.gc2 is not None:
                assert torch.equal(a.dg2, b.dg2) and torch.equal(a.db2, b.db2), tag

    start = torch.full((C,), 0.25)
    for two in (False, True):
        tag = f"rows={rows} C={C} two={two}"
        o = run("mask", bits_out, two, True)
        assert not torch.isnan(o.gc.float()).any()
        same(o, run("y", y, two, True), tag + " vs avt_bn_eval_bwd(y=out)")
        same(o, run("mask", bits_out, two, True), tag + " repeat")
        same(o, run("mask", bits_out, two, False), tag + " frozen", sums=False)  # NULL dgamma / dbeta / workspace
        for name, bits, mask in (("[out>0]", bits_out, mask_out), ("random bits", bits_rnd, mask_rnd)):
            o = run("mask", bits, two, True)
            r = _ref(k.gy, mask, k.c, rm, rv, k.gamma, k.beta)
            bc.check_elements(f"{tag} {name} gc", o.gc.cpu(), r.gc, r.T, r.a)
            bc.check_sums(f"{tag} {name}", o.dg.cpu(), o.db.cpu(), r, start, start)
            if two:
                r2 = _ref(k.gy, mask, k.cd, rm2, rv2, k.gamma2, k.beta2)
                bc.check_elements(f"{tag} {name} gc2", o.gc2.cpu(), r2.gc, r2.T, r2.a)
                bc.check_sums(f"{tag} {name} (2)", o.dg2.cpu(), o.db2.cpu(), r2, start, start)


def test_bn_eval_bwd_mask_refusals():
    """NULL mask, an unsupported channel count and parameter gradients without a workspace are refused."""
    rows, C = 8, 64
    k = bc.make_case(rows, C, seed=1)
    st, _, _ = _running_stats(k.gamma, k.beta, torch.Generator().manual_seed(1))
    g, c, std, gam = D(k.gy), D(k.c), D(st), D(k.gamma)
    bits = D(torch.zeros(rows, C // 8, dtype=torch.uint8))
    t1, _ = _target(c, std, gam, None, None, rows, C)
    with pytest.raises(RuntimeError):
        call("avt_bn_eval_bwd_mask", g.data_ptr(), None, ctypes.byref(t1), None, rows, C, S())
    with pytest.raises(RuntimeError):
        call("avt_bn_eval_bwd_mask", g.data_ptr(), bits.data_ptr(), ctypes.byref(t1), None, rows, 60, S())
    dg = D(torch.zeros(C))
    t1.dgamma = dg.data_ptr()  # wanted, but no workspace
    with pytest.raises(RuntimeError):
        call("avt_bn_eval_bwd_mask", g.data_ptr(), bits.data_ptr(), ctypes.byref(t1), None, rows, C, S())
