"""The hard-way head (csrc/head.hip), link by link, on the GPU's own tape.

tests/test_head_edges_gpu.py compares the head end to end with one number per output.  Here every launch is checked
on its own: its inputs are taken from the tape the GPU wrote (inv, vsum, A0, save, dA0 before and after the diagonal
kernels, dm, dvh), the one link is recomputed in fp64 (tests/headlink.py) and every element is held to the bound of
that launch's own arithmetic; the fp32 MFMA GEMMs are also run on exactly summable operands and compared for
equality.  Every output, tape and workspace buffer starts as NaN.  tests/test_head_links_cpu.py shows that the
bounds hold for the reference emulation and that twelve injected faults fall out of bound at their own link.

Draws: (a) test_head_edges_gpu's positive features, (b) mixed -- half the pairs aligned, half opposed, so that A
spans [-0.9, 0.9] and whole rows of Pos lie below 1e-20 (the 1e-12 clamp of weighted_A and of its backward), (c) A
within +-2 tau of eps1 / eps2.  Shapes: (1, 1, 1), (3, 1, 1), (65, 2, 2), (130, 3, 3) (split-K with a short last
split), (1024, 1, 1) / (1025, 1, 1) / (2051, 1, 1) (one, two and three passes of hardway_logits_kernel's column
loop, the last ragged; the CE kernel at L = 1026 / 1027 / 2053), C = 8 and C = 520 once each.

The sigmoid: the kernels' __expf is bounded by 3 x the error of torch's fp32 sigmoid on the CPU against fp64 in
the sigmoid's own unit (headlink.py); each test prints that yardstick Y and the kernel's own error in the same unit.

Each test prints its worst ratio per link.  Measured on one MI355X, the worst ratio to its bound over all 80 cases:
norm 0.173 and a0 0.328 (both at C = 8), logits 0.327 ((3, 1, 1)), ce 0.379 ((1025, 1, 1)), logits_bwd 0.300,
wa_bwd 0.964 (threshold draw, (130, 3, 3)), aux_bwd 0.990 (the attention form, where the update is one addition
that reaches its half ulp), dvh 0.422, gan 0.943 (accumulating at (1, 1, 1): the one rounding of gan0 + .),
norm_bwd 1.000 (a bf16 rounding reaches its half ulp), every exact record 0.  The sigmoid: the kernels' error is
at most 2.59 units (mixed draw, (130, 3, 3)) where the yardstick allows 4 + 3 Y = 9.08; __expf fits under the
fp32 CPU oracle's rule and no figure of its own had to be measured.  The whole file takes 6 s."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import headlink as hl

pytestmark = pytest.mark.gpu

from avt_amd._lib import call, query  # noqa: E402

DEV = "cuda"
EPS = (hl.EPS1, hl.EPS2, hl.TAU)
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


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _forward(v, an, trimap=True, neg=True, attention=False):
    """avt_hardway_fwd (or avt_hardway_attention_fwd) + avt_hardway_ce into NaN-filled buffers; v [B, P, C]."""
    B, Pn, C = v.shape
    L = B + (2 if neg else 1)
    s = {"B": B, "P": Pn, "C": C, "L": L, "trimap": int(trimap), "neg": int(neg), "attention": attention,
         "v": _dev(v), "an": _dev(an), "inv": _nan(B, Pn), "vsum": _nan(B, Pn), "A0": _nan(B, Pn, B),
         "save": _nan(int(query("avt_hardway_save_floats", B))), "logits": _nan(B, L), "A": _nan(B, Pn),
         "Pos": _nan(B, Pn), "Neg": _nan(B, Pn), "wA": _nan(B, Pn), "loss": _nan(), "dl": _nan(B, L)}
    tail = (P(s["inv"]), P(s["vsum"]), P(s["A0"]), P(s["save"]), P(s["logits"]), P(s["A"]), P(s["Pos"]),
            P(s["Neg"]), P(s["wA"]), S())
    if attention:
        assert trimap and neg and v.dtype == torch.float32
        call("avt_hardway_attention_fwd", P(s["v"]), P(s["an"]), B, Pn, C, *EPS, *tail)
    else:
        assert v.dtype == torch.bfloat16
        call("avt_hardway_fwd", P(s["v"]), P(s["an"]), B, Pn, C, *EPS, int(trimap), int(neg), *tail)
    call("avt_hardway_ce", P(s["logits"]), B, L, 1.0, P(s["loss"]), P(s["dl"]), S())
    torch.cuda.synchronize()
    return s


def _backward(s, cot=None, dl=None, gan0=None, accumulate=0, ws=None, detached=False):
    """One avt_hardway_bwd_ex (avt_hardway_attention_bwd) into NaN-filled buffers -> dict of what it wrote."""
    cot = cot or {}
    B, Pn, C = s["B"], s["P"], s["C"]
    dl = s["dl"] if dl is None else dl
    o = {"dA0": _nan(B, Pn, B), "gan": _nan(B, C) if gan0 is None else _dev(gan0).clone()}
    dev = {k: _dev(cot.get(k)) for k in ("dwA", "gA", "gPos", "gNeg")}
    if s["attention"]:
        o.update(dvh=_nan(B, Pn, C), gv=_nan(B, Pn, C))
        call("avt_hardway_attention_bwd", P(s["v"]), P(s["an"]), P(s["inv"]), P(s["A0"]), P(s["save"]), P(dl),
             P(dev["gA"]), B, Pn, C, *EPS, P(o["dA0"]), P(o["dvh"]), P(o["gv"]), P(o["gan"]), P(ws), S())
    else:
        if not detached:
            o.update(dvh=_nan(B, Pn, C), gv=_nan(B, Pn, C, dtype=torch.bfloat16))
        if dev["dwA"] is not None:
            o["dm"] = _nan(B, Pn)
        call("avt_hardway_bwd_ex", P(s["v"]), P(s["an"]), P(s["inv"]), P(s["A0"]), P(s["save"]), P(dl), B, Pn, C,
             *EPS, s["trimap"], s["neg"], P(dev["dwA"]), P(s["vsum"]), P(o.get("dm")), P(dev["gA"]), P(dev["gPos"]),
             P(dev["gNeg"]), P(o["dA0"]), P(o.get("dvh")), P(o.get("gv")), P(o["gan"]), accumulate, P(ws), S())
    torch.cuda.synchronize()
    return o


def _tape(s, cot=None, dl=None, gan0=None, accumulate=0, use_ws=False, detached=False):
    """The whole tape on the CPU in headlink.head_links' form: the backward runs once with dlogits alone (dA0 before
    the diagonal kernels), once more with dwA alone when both diagonal kernels run (dA0 between them), and once
    with everything.  Returns (tape, splits, ws)."""
    cot = {k: t for k, t in (cot or {}).items() if t is not None}
    B, Pn, C = s["B"], s["P"], s["C"]
    nws = int(query("avt_hardway_bwd_ws_floats", B, C))
    assert nws == 64 * B * C
    splits = hl.expected_splits(B * Pn)[0] if use_ws else 1
    tp = {k: s[k].cpu() for k in ("v", "an", "inv", "vsum", "A0", "save", "logits", "A", "Pos", "Neg", "wA")}
    tp["dl"] = (s["dl"] if dl is None else dl).cpu()
    tp["loss"] = s["loss"].cpu() if dl is None else None
    tp["dA0_pre"] = _backward(s, None, dl, detached=True)["dA0"].cpu()
    aux = {k: cot[k] for k in ("gA", "gPos", "gNeg") if k in cot}
    if "dwA" in cot and aux:
        tp["dA0_wa"] = _backward(s, {"dwA": cot["dwA"]}, dl)["dA0"].cpu()
    ws = _nan(nws) if use_ws else None
    o = _backward(s, cot, dl, gan0, accumulate, ws, detached)
    tp.update({k: t.cpu() for k, t in o.items()})
    if "dwA" in cot and not aux:
        tp["dA0_wa"] = tp["dA0"]
    tp.update({k: cot.get(k) for k in ("dwA", "gA", "gPos", "gNeg")})
    return tp, splits, ws


def _finish(tag, tp, rec, yard):
    """Print the worst ratio per link, the sigmoid yardstick next to the kernel's own sigmoid error in the same
    unit, and fail on any record out of bound."""
    e1, _, it = hl._consts(EPS)
    z = (tp["A"].double() - e1) * it
    w = torch.sigmoid(z)
    k = float(((tp["Pos"].double() - w).abs() / hl._sig_unit(z, w)).max())
    print(hl.report(tag, rec, yard) + f"  kernel sigmoid error {k:.2f} units (bound {hl.K_SIG + 3 * yard[0]:.2f})")
    bad = hl.failures(rec)
    for r in bad[:20]:
        print("OUT OF BOUND", r)
    assert not bad, (tag, bad[:5])
    # nothing the launches own is left unwritten
    for n in ("inv", "vsum", "A0", "save", "logits", "A", "Pos", "Neg", "wA", "dl", "loss", "dA0_pre", "dA0", "gan",
              "dvh", "gv", "dm"):
        if tp.get(n) is not None:
            assert torch.isfinite(tp[n].float()).all(), (tag, n)


def _inputs(draw, B, h, w, C):
    v, an = hl.DRAWS[draw](B, h, w, C, 1000 + B)
    return v.reshape(B, h * w, C), an


def _scaled_cot(B, Pn, scale=1e-3):
    return {k: t * scale for k, t in hl.draw_cotangents(B, Pn, 5).items()}


def _run_case(tag, draw, B, h, w, C=512, trimap=True, neg=True, cot="dense", use_ws=True, accumulate=1):
    v, an = _inputs(draw, B, h, w, C)
    s = _forward(v, an, trimap, neg)
    cot = _scaled_cot(B, h * w) if cot == "dense" else cot
    gan0 = torch.randn(B, C, generator=torch.Generator().manual_seed(7)) * 1e-3 if accumulate else None
    tp, splits, _ = _tape(s, cot, None, gan0, accumulate, use_ws)
    rec, yard = hl.head_links(tp, C, trimap, neg, splits=splits, gan0=gan0)
    _finish(tag, tp, rec, yard)
    return s, tp


SHAPES = [(1, 1, 1), (3, 1, 1), (65, 2, 2), (130, 3, 3), (1024, 1, 1), (1025, 1, 1)]


def test_old_tolerances_are_the_ones_read_on_the_cpu():
    import test_head_edges_gpu as he

    assert he.TOL == hl.OLD_TOL and (he.EPS1, he.EPS2, he.TAU) == EPS
    for rows in (1, 255, 260, 1170, 1200, 2051, 16640):
        assert he._expected_splits(rows) == hl.expected_splits(rows)
    assert hl.expected_splits(1170) == (4, 320)  # (130, 3, 3): the last split is short (210 rows)


@pytest.mark.parametrize("draw,B,h,w", [(d, *s) for d in hl.DRAWS for s in SHAPES] + [("positive", 2051, 1, 1)])
def test_links(draw, B, h, w):
    """Every link on every draw and shape, all cotangents dense, gan accumulated through the split-K workspace (the
    third, ragged pass of the column loop, B = 2051, once)."""
    _run_case(f"{draw} ({B}, {h}, {w})", draw, B, h, w)


@pytest.mark.parametrize("C", [8, 520])
def test_links_channel_edges(C):
    """C = 8: one lane of vis_norm's loop; C = 520: a second trip for one lane and an 8-element GEMM k-tail."""
    _run_case(f"positive (65, 2, 2) C={C}", "positive", 65, 2, 2, C=C)


@pytest.mark.parametrize("B,h,w", [(65, 2, 2), (1025, 1, 1)])
@pytest.mark.parametrize("trimap,neg", [(False, True), (True, False), (False, False)])
@pytest.mark.parametrize("draw", ["positive", "mixed"])
def test_links_trimap_neg(draw, trimap, neg, B, h, w):
    _run_case(f"{draw} ({B}, {h}, {w}) trimap={int(trimap)} neg={int(neg)}", draw, B, h, w, trimap=trimap, neg=neg)


COTS = ["dlogits", "dwA", "gA", "gPos", "gNeg", "dense"]


@pytest.mark.parametrize("B,h,w", [(65, 2, 2), (130, 3, 3)])
@pytest.mark.parametrize("trimap", [True, False])
@pytest.mark.parametrize("which", COTS)
def test_links_single_cotangents(which, trimap, B, h, w):
    """dlogits alone, then each of dwA / gA / gPos / gNeg alone on a zero dlogits (so that the diagonal kernel's
    update is all there is on the diagonal), then all dense; hardway_aux_bwd_kernel with trimap = 0 too."""
    Pn, C = h * w, 512
    v, an = _inputs("mixed", B, h, w, C)
    s = _forward(v, an, trimap, True)
    full = _scaled_cot(B, Pn)
    cot = {} if which == "dlogits" else full if which == "dense" else {which: full[which]}
    dl = None if which in ("dlogits", "dense") else torch.zeros_like(s["dl"])
    tp, splits, _ = _tape(s, cot, dl, None, 0, True)
    rec, yard = hl.head_links(tp, C, trimap, True, splits=splits, forward=False)
    _finish(f"mixed ({B}, {h}, {w}) trimap={int(trimap)} {which} alone", tp, rec, yard)
    if dl is not None:  # off the diagonal a zero dlogits leaves zeros
        off = ~torch.eye(B, dtype=torch.bool)[:, None, :].expand(B, Pn, B)
        assert (tp["dA0"][off] == 0).all()


@pytest.mark.parametrize("B,h,w", [(65, 2, 2), (130, 3, 3)])
def test_detached_form(B, h, w):
    """dvh = gv = NULL (the tube's detached video features): dA0 and gan bitwise as with the vision gradient, the
    same workspace floats written, every link in bound."""
    C = 512
    v, an = _inputs("positive", B, h, w, C)
    s = _forward(v, an)
    cot = {k: t for k, t in _scaled_cot(B, h * w).items() if k != "dwA"}
    tp, splits, ws = _tape(s, cot, None, None, 0, True)
    td, _, wsd = _tape(s, cot, None, None, 0, True, detached=True)
    assert "dvh" not in td and "gv" not in td
    assert torch.equal(tp["gan"], td["gan"]) and torch.equal(tp["dA0"], td["dA0"])
    assert torch.equal(torch.isnan(ws), torch.isnan(wsd)) and torch.equal(ws.nan_to_num(), wsd.nan_to_num())
    rec, yard = hl.head_links(td, C, splits=splits, forward=False)
    _finish(f"detached ({B}, {h}, {w})", td, rec, yard)


@pytest.mark.parametrize("B,h,w", [(65, 2, 2), (130, 3, 3)])
@pytest.mark.parametrize("use_ws", [False, True])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_gan_accumulate(accumulate, use_ws, B, h, w):
    """gan_accumulate 0 / 1 with and without the workspace: the gan link in bound (one more rounding when
    accumulating), two runs bitwise equal, and exactly splits * B * C workspace floats written when the GEMM splits
    ((130, 3, 3): 4 splits of 320 rows, the last 210; (65, 2, 2): one split, which writes gan itself and leaves the
    workspace alone)."""
    C = 512
    v, an = _inputs("positive", B, h, w, C)
    s = _forward(v, an)
    gan0 = torch.randn(B, C, generator=torch.Generator().manual_seed(7)) * 1e-3 if accumulate else None
    runs = [_tape(s, _scaled_cot(B, h * w), None, gan0, accumulate, use_ws) for _ in range(2)]
    (tp, splits, ws), (tp2, _, ws2) = runs
    assert splits == ({260: 1, 1170: 4}[B * h * w] if use_ws else 1)
    assert torch.equal(tp["gan"], tp2["gan"]), "gan is not repeatable"
    assert torch.equal(tp["gv"].view(torch.int16), tp2["gv"].view(torch.int16))
    if use_ws:
        n = splits * B * C if splits > 1 else 0
        assert torch.isfinite(ws[:n]).all() and torch.isnan(ws[n:]).all()
        assert torch.equal(ws[:n], ws2[:n])
    rec, yard = hl.head_links(tp, C, splits=splits, gan0=gan0, forward=False)
    _finish(f"gan accumulate={accumulate} ws={int(use_ws)} ({B}, {h}, {w})", tp, rec, yard)


@pytest.mark.parametrize("B,h,w", [(65, 2, 2), (1025, 1, 1)])
def test_attention_links(B, h, w):
    """avt_hardway_attention_fwd / _bwd: the same links with inv == 1 exactly and gv == dvh (fp32)."""
    C = 512
    v, an = _inputs("positive", B, h, w, C)
    v = F.normalize(v.float(), dim=2)
    s = _forward(v, an, attention=True)
    tp, splits, _ = _tape(s, {"gA": _scaled_cot(B, h * w)["gA"]}, None, None, 0, True)
    rec, yard = hl.head_links(tp, C, attention=True, splits=splits)
    _finish(f"attention ({B}, {h}, {w})", tp, rec, yard)


# (B, P, C): rows = B P in {63, 64, 65, 129}, B in {63, 64, 65}, every C, B mod 4 in {0, 1, 2, 3}
EXACT = [(63, 1, 512), (64, 1, 520), (65, 1, 8), (66, 1, 24), (129, 1, 32), (43, 3, 40), (13, 5, 512), (64, 2, 32)]


@pytest.mark.parametrize("B,Pn,C", EXACT)
def test_gemms_exact(B, Pn, C):
    """The three GEMMs on exactly summable operands through the attention entry points (fp32 v): v in {-1, 0, 1} 2^-5,
    an in {-1, 0, 1} 2^-4, so every product is a multiple of 2^-9 and sum |products| <= 1: any fp32 summation order
    is exact and A0 must EQUAL the fp64 product.  With dlogits = 0 and integer gA, dA0 is gA on the diagonal and 0
    elsewhere, so dvh[(i, p)] == gA[i, p] an[i] and gan[j] == sum_p gA[j, p] v[(j, p)] exactly: the placement of
    every k index in both backward GEMMs and the split-K sum, with no tolerance."""
    g = torch.Generator().manual_seed(B * 1000 + C)
    v = torch.randint(-1, 2, (B, Pn, C), generator=g).float() * 2.0 ** -5
    an = torch.randint(-1, 2, (B, C), generator=g).float() * 2.0 ** -4
    gA = torch.randint(-3, 4, (B, Pn), generator=g).float()
    rows = B * Pn
    # the conditions (conditions, not tolerances)
    mag = v.double().abs().reshape(rows, C) @ an.double().abs().T
    assert mag.max() <= 1.0 and (mag * 2 ** 9 == (mag * 2 ** 9).round()).all()
    assert (v != 0).float().mean() > 0.5 and (an != 0).float().mean() > 0.5
    ref = (v.double().reshape(rows, C) @ an.double().T).reshape(B, Pn, B)
    assert torch.equal(ref.float().double(), ref)
    s = _forward(v, an, attention=True)
    assert torch.equal(s["A0"].cpu().double(), ref), "A0 is not the exact product"
    assert torch.equal(s["inv"].cpu(), torch.ones(B, Pn)) and torch.equal(s["vsum"].cpu().double(), v.double().sum(2))
    assert torch.isfinite(s["logits"]).all() and torch.equal(s["A"].cpu(), hl._diag(s["A0"].cpu()))
    outs = []
    for use_ws in (False, True):
        ws = _nan(int(query("avt_hardway_bwd_ws_floats", B, C))) if use_ws else None
        o = _backward(s, {"gA": gA}, torch.zeros_like(s["dl"]), ws=ws)
        want = torch.zeros(B, Pn, B)
        hl._diag(want).copy_(gA)
        assert torch.equal(o["dA0"].cpu(), want)
        assert torch.equal(o["dvh"].cpu().double(), gA.double()[..., None] * an.double()[:, None, :])
        assert torch.equal(o["gv"].cpu(), o["dvh"].cpu())
        assert torch.equal(o["gan"].cpu().double(), (gA.double()[..., None] * v.double()).sum(1))
        outs.append(o)
    assert torch.equal(outs[0]["gan"], outs[1]["gan"])


@pytest.mark.parametrize("B,h,w", [(65, 2, 2), (300, 2, 2)])
def test_consistent_with_the_end_to_end_check(B, h, w):
    """On the positive draw the per-link checks and test_head_edges_gpu._check pass on the same run."""
    import test_head_edges_gpu as he

    v, an, r64, r32 = he._reference(B, h, w, True, True)
    s = _forward(v.reshape(B, h * w, 512), an)
    tp, splits, _ = _tape(s, None, None, None, 0, False)
    rec, yard = hl.head_links(tp, 512, splits=splits)
    _finish(f"positive ({B}, {h}, {w}), CE only", tp, rec, yard)
    got = dict(tp, loss=s["loss"])
    he._check(f"old check B={B} P={h * w}", got, r64, r32)
