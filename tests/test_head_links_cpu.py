"""tests/headlink.py on the CPU: the reference emulation (torch fp32) stays inside every link's bound on the cases
tests/test_head_links_gpu.py runs, each injected fault falls out of bound first at the link it touches, and the
reading of the older end-to-end tolerances (tests/test_head_edges_gpu.TOL) on the same faults.

Measured here (emulation, worst ratio to the bound over all cases): norm 0.17, a0 0.33, logits 0.37, logits_bwd
0.30, wa_bwd 0.80, aux_bwd 0.54 (0.99 in the attention form, where the update is one addition), dvh 0.48, gan 0.98
(accumulating: the one rounding of gan0 + . reaches its half ulp), norm_bwd 1.000 (so does the bf16 rounding).

The older instrument on the twelve faults, positive draw at (130, 3, 3), all cotangents dense at the CE gradient's
magnitude, accumulating split-K: it passes ONE, `dm_not_in_dot` (0.46 of the gv tolerance; the unfaulted emulation
reads 0.20), and catches the other eleven, single k-tail elements included -- the nearly parallel features amplify
them (a k-tail element of the dvh GEMM reads 55 x the gv tolerance).  What the link checks add is therefore that
one fault, the attribution to a launch, per-element bounds, and the branches no older test runs.
test_old_instrument_reading prints the table and asserts that subset."""
import pytest
import torch

import headlink as hl

C = 512
SHAPES = [(1, 1, 1), (3, 1, 1), (65, 2, 2), (130, 3, 3), (1024, 1, 1), (1025, 1, 1)]
CASES = [(d, s, C, True, True) for d in hl.DRAWS for s in SHAPES]
CASES += [("positive", (65, 2, 2), 8, True, True), ("positive", (65, 2, 2), 520, True, True)]
CASES += [(d, s, C, t, n) for d in ("positive", "mixed") for s in ((65, 2, 2), (1025, 1, 1))
          for t, n in ((False, True), (True, False), (False, False))]
CASES += [("positive", (2051, 1, 1), C, True, True)]

WORST = {}


def _case(draw, shape, c, seed=None):
    B, h, w = shape
    v, an = hl.DRAWS[draw](B, h, w, c, 1000 + B if seed is None else seed)
    return v.reshape(B, h * w, c), an


@pytest.mark.parametrize("draw,shape,c,trimap,neg", CASES)
def test_emulation_within_bounds(draw, shape, c, trimap, neg):
    v, an = _case(draw, shape, c)
    B, P, _ = v.shape
    splits = hl.expected_splits(B * P)[0]
    gan0 = torch.randn(B, c, generator=torch.Generator().manual_seed(7))
    tp = hl.emulate_head(v, an, hl.draw_cotangents(B, P, 5), trimap=trimap, neg=neg, splits=splits, gan0=gan0)
    rec, yard = hl.head_links(tp, c, trimap, neg, splits=splits, gan0=gan0)
    print(hl.report(f"{draw} {shape} C={c} trimap={int(trimap)} neg={int(neg)}", rec, yard))
    for k, r in hl.worst_by_link(rec).items():
        WORST[k] = max(WORST.get(k, 0.0), r[2])
    assert set(hl.worst_by_link(rec)) == set(hl.LINKS)
    assert not hl.failures(rec), hl.failures(rec)[:5]
    print("worst so far:", {k: round(x, 3) for k, x in WORST.items()})


@pytest.mark.parametrize("shape", [(65, 2, 2), (1025, 1, 1)])
def test_attention_emulation_within_bounds(shape):
    v, an = _case("positive", shape, C)
    v = torch.nn.functional.normalize(v.float(), dim=2)
    B, P, _ = v.shape
    tp = hl.emulate_head(v, an, {"gA": hl.draw_cotangents(B, P, 5)["gA"]}, attention=True)
    rec, yard = hl.head_links(tp, C, attention=True)
    print(hl.report(f"attention {shape}", rec, yard))
    assert not hl.failures(rec), hl.failures(rec)[:5]


def test_mixed_draw_reaches_the_clamp_and_threshold_draw_the_thresholds():
    """What the draws are for: (b) spans [-0.9, 0.9] with whole rows of Pos below 1e-20, (c) sits within +-2 tau
    (and the bf16 rounding of v) of eps1 and eps2."""
    v, an = _case("mixed", (65, 2, 2), C)
    tp = hl.emulate_head(v, an)
    assert tp["A"].min() < -0.85 and tp["A"].max() > 0.85
    assert (tp["Pos"].max(1).values < 1e-20).sum() >= 65 // 2
    v, an = _case("threshold", (65, 2, 2), C)
    A = hl.emulate_head(v, an)["A"]
    near = torch.minimum((A - hl.EPS1).abs(), (A - hl.EPS2).abs())
    assert near.max() <= 2 * hl.TAU + 0.01
    assert ((A - hl.EPS1).abs() < 2.1 * hl.TAU).any() and ((A - hl.EPS2).abs() < 2.1 * hl.TAU).any()


@pytest.mark.parametrize("shape", [(3, 1, 1), (65, 2, 2), (1025, 1, 1)])
def test_clamp_rows_agree_with_normalize(shape):
    """On the clamp rows of the mixed draw ||Pos|| <= 1e-12 in fp64 AND in fp32 (where w * w underflows), so
    F.normalize and the kernels' 1 / max(||Pos||, 1e-12) are the same formula, Pos * 1e12; the link oracle takes the
    clamp there, and the wa_bwd projection is 0 as clamp_min's backward."""
    v, an = _case("mixed", shape, C)
    B, P, _ = v.shape
    cot = {"dwA": hl.draw_cotangents(B, P, 5)["dwA"]}
    tp = hl.emulate_head(v, an, cot)
    rows = tp["Pos"].max(1).values < 1e-20
    assert rows.sum() >= B // 2
    for dt in (torch.float64, torch.float32):
        pos = torch.sigmoid((tp["A"].to(dt) - hl.EPS1) / hl.TAU)
        nrm = (pos * pos).sum(1).sqrt()
        assert (nrm[rows] <= 1e-12).all()
        assert torch.equal(torch.nn.functional.normalize(pos, dim=1)[rows], (pos / 1e-12)[rows])
    ref = hl.oracle_e2e(v, an, cot)
    m = (tp["vsum"] * tp["inv"] / C).double()
    want = m * torch.sigmoid((tp["A"].double() - hl.EPS1) / hl.TAU) * 1e12
    assert torch.allclose(ref["wA"][rows], want[rows], rtol=1e-4, atol=0)
    assert torch.allclose(tp["wA"].double()[rows], want[rows], rtol=1e-4, atol=0)


# ---------------------------------------------------------------------------------------------------- faults
FSHAPE = (130, 3, 3)


def _fault_run(fault, draw="positive"):
    v, an = _case(draw, FSHAPE, C)
    B, P, _ = v.shape
    splits = hl.expected_splits(B * P)[0]
    assert splits == 4
    gan0 = torch.randn(B, C, generator=torch.Generator().manual_seed(7)) * 1e-3
    cot = hl.draw_cotangents(B, P, 5)
    cot = {k: t * 1e-3 for k, t in cot.items()}  # of the CE gradient's own magnitude
    tp = hl.emulate_head(v, an, cot, faults=(fault,) if fault else (), splits=splits, gan0=gan0)
    return v, an, cot, gan0, splits, tp


@pytest.mark.parametrize("fault", hl.FAULTS)
def test_fault_caught_at_its_link(fault):
    v, an, cot, gan0, splits, tp = _fault_run(fault)
    rec, _ = hl.head_links(tp, C, splits=splits, gan0=gan0)
    bad = hl.failures(rec)
    print(fault, "->", [(r[0], r[1], f"{r[2]:.3g}") for r in bad[:6]])
    assert bad, f"{fault} passes every link"
    assert bad[0][1] == hl.FAULT_LINK[fault], (fault, bad[0])
    # a fault shows only where the tape does not carry it on (the lost diagonal updates are two kernels')
    also = {"diag_before_store": {"wa_bwd", "aux_bwd"}}.get(fault, {hl.FAULT_LINK[fault]})
    assert {r[1] for r in bad} <= also, bad


OLD_PASSES = {"dm_not_in_dot"}


def test_old_instrument_reading():
    """Every fault as tests/test_head_edges_gpu.TOL reads it on the same draw (fp64 autograd end to end, errors as
    that file's _err): the faults it passes are the gap the link checks close."""
    passes = set()
    ref = None
    for fault in (None,) + hl.FAULTS:
        v, an, cot, gan0, splits, tp = _fault_run(fault)
        if ref is None:
            ref = hl.oracle_e2e(v, an, cot)
        rd = hl.old_reading(tp, ref, gan0)
        over = {n: e / t for n, (e, t) in rd.items() if not e <= t}
        print(f"{str(fault):18s} " + " ".join(f"{n} {e / t:8.2e}" for n, (e, t) in rd.items()) +
              ("   PASSES" if not over else f"   caught by {sorted(over)}"))
        if not over:
            passes.add(fault)
    assert None in passes, "the old tolerance fails the unfaulted emulation"
    assert passes - {None} == OLD_PASSES, passes
