"""Trunk.backward (the 2-D ResNet-18 trunk, both modalities) as a whole against fp64 autograd on the GPU's OWN forward
state (the "teacher-forced" oracle avenet_oracle.resnet18_forward_forced).  For a fixed forward state the backward is a
linear map of the upstream gradient, so forcing the oracle's conv outputs, ReLU masks and outputs to the tape's takes
the forward's rounding noise out of the comparison and leaves what only the composition can get wrong: in the default
graph avt_bn_bwd_mask feeding two BNs from one g', an identity block's residual entering conv1's dgrad as (g, mask
bits), the 1x1/s2 downsample dgrad accumulated in place over conv1's, the stem's fused max-pool/ReLU/BN backward, the
input gradient and which tape tensor feeds which wgrad; in the FUSE_BN_BWD graph the BN reductions carried by the dgrad
epilogues (skip_class00 on a strided conv1 dgrad, append_slots on the downsample dgrad that finishes the same BN),
avt_bn_bwd_premasked and the premasked flag across the HI_BLOCK boundary; with AVEngine.splitk the layer3/4 convs
through the split-K kernels.  The engine-only ways of issuing the same launches (deferred wgrad reduces, one stream,
two segments) are held bitwise to the default engine.  tests/test_trunk2d_forced_oracle_cpu.py shows on the CPU that
the oracle is sound, that its yardstick meets the cap below and that five wiring faults fall out of bound.

One known difference is left in the comparison: the stem kernel rounds relu(bn1(c0)) to bf16 before its max-pool picks
a window's first maximum, the oracle picks among the fp64 values; where two of a window's values round to one bf16
number the two route the gradient to different pixels.  Simulated on the CPU (same shapes) that alone is an error of
3.2e-2 / 2.0e-2 on the vision / audio stem weight and 3.3e-2 / 3.7e-2 on the input gradient, inside the 5e-2 floor,
and nothing anywhere else."""
import numpy as np
import pytest
import torch

import avenet_oracle as orc
from gradcheck import rule_full

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
E_REF_CAP, MAX_OVER_CAP = 0.1, 6  # test_r3d_backward_forced_gpu.py's condition on the yardstick
MODALS = ("vision", "audio")
_REFS = {}  # modal -> [(tape, ref, yard)]: the oracle's gradients, computed once per distinct GPU tape


def _inputs(modal):
    """Vision: frames 16 x 16 in layer1, 8 x 8 in layer2, 4 x 4 in layer3/4 (M below one tile).  Audio: 33 x 38 ->
    17 x 19 -> 9 x 10 -> 5 x 5, odd sizes (ragged stride-2 parity classes), the Cp = 1 stem."""
    if modal == "audio":
        return orc.make_spectrogram(2, 65, 76), orc.make_gout(2, 5, 5)
    return orc.make_image(3, 64), orc.make_gout(3, 4, 4)


def _nchw(t):
    """[N, H, W, C] bf16 on the GPU -> [N, C, H, W] fp32 on the CPU."""
    return t.permute(0, 3, 1, 2).float().cpu()


def _forced(sd, x, modal, tape, g_out):
    """(ref, yard) of the forced oracle on this tape; shared by the runs whose forward gave the same bits."""
    def same(a, b):
        return torch.equal(a["c0"], b["c0"]) and torch.equal(a["p0"], b["p0"]) and all(
            sorted(ta) == sorted(tb) and all(torch.equal(ta[k], tb[k]) for k in ta)
            for ta, tb in zip(a["blocks"], b["blocks"]))

    for t, ref, yard in _REFS.setdefault(modal, []):
        if same(t, tape):
            return ref, yard
    ref = orc.resnet18_forced_grads(sd, x, modal, tape, g_out)
    yard = orc.resnet18_forced_grads(sd, x, modal, tape, g_out, round_grads=True)
    _REFS[modal].append((tape, ref, yard))
    return ref, yard


def _run_and_check(modal, tag, splitk=False):
    """A standalone resnet18(modal) on the seeded weights: engine.forward, engine.backward with the input gradient,
    the mask bits against the stored outputs, every gradient against the forced oracle fed the tape.  Returns the
    engine."""
    from avt_amd.model import resnet18

    sd = orc.make_state(0)
    prefix = "audnet." if modal == "audio" else "imgnet."
    net = resnet18(modal=modal)
    net.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
    net = net.to(DEV).train()
    engine, flat, _, _ = net._engine_and_params()
    engine.splitk = splitk
    x, g_out = _inputs(modal)
    _, tp = engine.forward(x.to(DEV), True)
    tp["want_dx"] = True
    gflat = torch.zeros(flat.n_train, device=DEV, dtype=torch.float32)
    engine.backward(tp, g_out.to(DEV), gflat)
    torch.cuda.synchronize()
    grads = {n: g.detach().double().cpu() for n, g in flat.param_grad_views(gflat).items()}
    grads["input"] = tp["dx"].double().cpu()

    # the block-output mask bits the backward reads instead of `out`: bit e of byte j <-> channel 8 j + e
    assert len(tp["blocks"]) == 8
    for i, tb in enumerate(tp["blocks"]):
        C = tb["out"].shape[-1]
        om = tb["om"].view(-1, C // 8).cpu().int()
        bits = ((om[:, :, None] >> torch.arange(8, dtype=torch.int32)) & 1).reshape(-1, C).bool()
        assert torch.equal(bits, tb["out"].reshape(-1, C).cpu() > 0), f"{tag}: block {i} mask bits != [out > 0]"

    tape = {"c0": _nchw(tp["c0"]), "p0": _nchw(tp["blocks"][0]["x"]), "blocks": []}
    for tb in tp["blocks"]:
        tape["blocks"].append({k: _nchw(tb[k]) for k in ("c1", "h1", "c2", "cd", "out") if k in tb})
    assert tuple(tape["blocks"][7]["out"].shape) == tuple(g_out.shape)
    ref, yard = _forced(sd, x, modal, tape, g_out)
    assert len(ref) == 61 and sorted(ref) == sorted(grads)
    bad, over, e_refs, worst = [], [], [], (None, 0.0)
    for n, r in ref.items():
        assert tuple(grads[n].shape) == tuple(r.shape), n
        viol, e, e_ref, ratio = rule_full(grads[n], r, yard[n])
        print(f"  {n}: e {e:.3e} e_ref {e_ref:.3e} ({ratio:.2f} of its bound)")
        e_refs.append(e_ref)
        if e_ref > E_REF_CAP:
            over.append((n, round(e_ref, 4)))
        if ratio > worst[1]:
            worst = (n, ratio)
        bad += [(n,) + v for v in viol]
    e_refs = np.array(e_refs)
    print(f"{tag}: forced yardstick e_ref max {e_refs.max():.3e} median {np.median(e_refs):.3e}; above {E_REF_CAP}: "
          f"{over}; largest error {worst[1]:.2f} of its bound ({worst[0]})")
    for b in bad:
        print("OUT OF BOUND", b)
    assert len(over) <= MAX_OVER_CAP, over
    assert not bad, bad
    return engine


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("modal", MODALS)
def test_forced_tape(modal, fuse, monkeypatch):
    """engine.forward(x, True), then engine.backward(tape, g_out, gflat) with tape["want_dx"] for a fixed dense
    standard normal g_out (loss = (layer4 map * g_out).sum()), in the default backward graph (fuse 0) and the
    FUSE_BN_BWD one (fuse 1), against the forced oracle fed the tape (c0, p0, per block c1, h1, c2, cd, out).

    Yardstick: the same forced oracle with every activation gradient the GPU stores in bf16 rounded to bf16 (autograd
    hooks on c0, p0, c1, h1, c2, cd and each block's output).  Every one of the 60 parameter gradients and the input
    gradient, on the whole tensor, by gradcheck's rule: error vector <= max(5e-2, 3 e_ref), cosine >= min(0.999,
    1 - 3 (1 - cos_ref)), norm deviation <= max(5e-2, 3 d_ref, e_ref).  Condition: the yardstick's own e_ref is at
    most 0.1 for all but at most 6 tensors (printed; still checked).  In the same run: the unpacked mask bits `om` of
    all 8 blocks equal [out > 0] exactly.

    Measured on one MI355X (the tape, hence the yardstick, is the same for both graphs): the forced yardstick's e_ref
    is 0 (layer4.1.bn2.bias) to 1.32e-2, median 6.0e-3, for vision and 0 to 1.58e-2, median 6.1e-3, for audio -- no
    tensor above the cap, so every bound is the 5e-2 floor.  This build's largest error, in both graphs: vision 0.76
    of its bound (input, e 3.8e-2) and 0.73 (conv1.weight, e 3.65e-2), audio 0.65 (input, e 3.2e-2) -- the stem's
    routing among bf16 ties (module docstring) -- and, everything else, 0.30 (vision bn1.bias, e 1.5e-2 against e_ref
    1.3e-2) and 0.27 (audio bn1.weight); layer2-4's gradients are at 0.04-0.18 of their bounds."""
    import avt_amd.trunk

    monkeypatch.setattr(avt_amd.trunk, "FUSE_BN_BWD", bool(fuse))
    _run_and_check(modal, f"{modal} fuse={fuse}")


@pytest.mark.parametrize("modal", MODALS)
def test_forced_tape_splitk(modal, monkeypatch):
    """The same check (default graph) with engine.splitk: the layer3/4 3x3/s1 convs run avt_conv2d_fwd_ws and
    avt_conv2d_dgrad_ws (the residual as add / add_mask inside the split-K finish).  At least one layer3/4 call site
    planned a split, and every ticket array is left zero.

    Measured on one MI355X: the planner itself splits ten call sites at these shapes, forward and dgrad each
    (layer2.0.conv2 to layer4.1.conv2, every 3x3/s1 conv of layer2-4); yardstick e_ref up to 1.27e-2 (median
    5.6e-3) for vision and 1.52e-2 (6.2e-3) for audio; largest error 0.78 (vision input) and 0.65 (audio input) of
    its bound, everything but the stem weight and the input at most 0.30 (vision bn1.bias)."""
    import avt_amd.trunk
    from avt_amd._lib import call

    monkeypatch.setattr(avt_amd.trunk, "FUSE_BN_BWD", False)

    def tickets(engine):
        return {k: cnt for k, (_, cnt) in engine._splitk_cnt.items() if cnt is not None}

    try:
        engine = _run_and_check(modal, f"{modal} splitk", splitk=True)
        if not tickets(engine):  # the planner splits nothing at these shapes: force two splits
            call("avt_set_halo_splitk", 2, 0)
            engine = _run_and_check(modal, f"{modal} splitk (forced 2)", splitk=True)
        tk = tickets(engine)
        sites = sorted({(k[0], "dgrad" if k[1] else "fwd") for k in tk})
        print(f"{modal}: split-K call sites {sites}")
        assert any(k[0].startswith(("layer3.", "layer4.")) for k in tk), sorted(engine._splitk_cnt)
        torch.cuda.synchronize()
        assert all(int(cnt.abs().sum()) == 0 for cnt in tk.values()), "split-K tickets not left zero"
    finally:
        call("avt_set_halo_splitk", 0, 0)


def test_engine_variants_bitwise(monkeypatch):
    """The full AVEngine (both trunks and the head, forward with CE, backward from dlogits) at make_image(4, 64),
    make_spectrogram(4, 65, 76): the flat gradient of the default engine against the same step with the wgrads'
    slab reduces deferred to one batched launch per trunk and segment (defer_wgrad), issued on one stream
    (concurrent = False), and in two segments (a listening on_boundary) -- bitwise, as include/avt.h and
    test_train_step_is_deterministic promise; a fresh model from the same seed each time.  The deferred runs must
    have had slabs pending and have left none.  This anchors the engine-only paths to the trunk code that
    test_forced_tape holds to fp64.

    Measured on one MI355X: all variants bitwise equal.  At 4 clips the planner's own splits leave no slab to defer
    (0 pending), so the deferred comparison runs again, with its own baseline, under avt_set_wgrad_policy(0, 1):
    12 slabs pending in the one-segment run and 12 in the two-segment run, none left."""
    import avt_amd.trunk
    from avt_amd._lib import call
    from avt_amd.model import AVENet, HardWayArgs

    monkeypatch.setattr(avt_amd.trunk, "FUSE_BN_BWD", False)
    img, aud, sd = orc.make_image(4, 64), orc.make_spectrogram(4, 65, 76), orc.make_state(0)

    def run(defer=False, concurrent=True, on_boundary=None):
        m = AVENet(HardWayArgs(), False)
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        eng = m.engine()
        eng.defer_wgrad, eng.concurrent, eng.splitk = defer, concurrent, False
        seen = []  # (slabs pending before, after) each flush
        for tr in (eng.img, eng.aud):
            def flush(store, tr=tr, orig=tr.flush_wgrad):
                pend = store.wgrad_pending(tr.prefix)
                before = None if pend is None else len(pend)
                orig(store)
                seen.append((before, None if pend is None else len(pend)))
            monkeypatch.setattr(tr, "flush_wgrad", flush)
        out, tape = eng.forward(img.to(DEV), aud.to(DEV), training=True, with_ce=True)
        gflat = torch.zeros(eng.flat.n_train, device=DEV, dtype=torch.float32)
        eng.backward(tape, out["dlogits"], gflat, on_boundary=on_boundary)
        torch.cuda.synchronize()
        assert eng.store.pending is None and eng.store.grads is None
        return out["loss"].item(), gflat.cpu(), seen

    def compare(every):
        """The default engine's bits against the variants'; returns the slabs the deferred runs saw pending."""
        loss0, g0, seen0 = run()
        assert np.isfinite(loss0) and torch.isfinite(g0).all() and g0.abs().sum() > 0
        assert all(s == (None, None) for s in seen0), seen0
        loss, g, seen = run(defer=True)
        assert all(a == 0 for _, a in seen), seen  # every flush left no slab pending
        assert loss == loss0 and torch.equal(g, g0), "defer_wgrad changes the gradient bits"
        loss, g, seen2 = run(defer=True, on_boundary=lambda t: None)
        assert len(seen2) == 4 and all(a == 0 for _, a in seen2), seen2  # a flush per trunk and segment
        assert loss == loss0 and torch.equal(g, g0), "defer_wgrad in two segments changes the gradient bits"
        if every:
            loss, g, _ = run(concurrent=False)
            assert loss == loss0 and torch.equal(g, g0), "one-stream issue changes the gradient bits"
            tags = []
            loss, g, _ = run(on_boundary=tags.append)
            assert tags == [("imgnet.hi", "audnet.hi"), ("imgnet.lo", "audnet.lo")], tags
            assert loss == loss0 and torch.equal(g, g0), "the two-segment backward changes the gradient bits"
        return sum(b for b, _ in seen), sum(b for b, _ in seen2)

    try:
        pending = compare(True)
        print(f"deferred wgrad slabs, the planner's own splits: {pending}")
        if not all(pending):
            # the wave model splits no deferrable wgrad at 4 clips (a slab is deferred where it has >= 2 splits and
            # >= 16 tiles: layer3.0.conv1 and layer4's 3x3 convs, whose 64-100 rows are 2-4 k-tiles, under the
            # default minimum of 4 per split): let a split be one k-tile deep, and compare under that plan
            call("avt_set_wgrad_policy", 0, 1)
            pending = compare(False)
            print(f"deferred wgrad slabs, splits of one k-tile: {pending}")
        assert all(pending), pending  # slabs were pending at some point, in one segment and in two
    finally:
        call("avt_set_wgrad_policy", 0, 4)  # the library's defaults
