"""The hard-way head (csrc/head.hip) and its cross-entropy at the batch sizes where their kernels change shape,
against the fp64 oracle (oracle/avenet_oracle.py) on the same bf16-rounded features.

  * sgemm_kernel: 64x64 tiles, 32-deep k-tiles, 16-byte fetches only where aligned -- in the `gan` GEMM the
    unit-stride dimension of dA0 is B, so B mod 4 decides the alignment and B mod 64 the tile tails;
  * the ordered split-K of the `gan` GEMM (avt_hardway_bwd_ex with a workspace): rows / 256 splits, capped at
    64, k_per_split rounded up to 32 and the split count re-derived from it;
  * hardway_logits_kernel: 1024 / min(B, 1024) sub-threads per column, combined through LDS;
  * hardway_ce_kernel: the register-resident body for rows of L <= 256 logits, the strided loop above.

Tolerances: the project's own (test_kernels_gpu.test_hardway_head), which hold at every size here, 16,640 rows
included.  Each check also prints the error of THE SAME ORACLE run in fp32 on the CPU against fp64, the yardstick a
bound would fall back on (tests/gradcheck.py: 3 x the reference's own error, never the kernel's): on the logits
that fp32 oracle is itself up to 3.1e-3 off (B = 255) -- the -99 / 0.07 diagonal is about 1400 -- while the
kernel's largest error is 1.5e-3 (B = 600)."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from avt_amd._lib import call, query  # noqa: E402

DEV = "cuda"
C = 512
EPS1, EPS2, TAU = 0.65, 0.4, 0.03
# test_hardway_head's tolerances: absolute for the maps and the logits, relative to max(1, |loss|) for the loss,
# relative to the reference's largest element for the two gradients
TOL = {"A": 1e-5, "logits": 2e-3, "loss": 1e-5, "Pos": 1e-3, "Neg": 1e-3, "wA": 1e-5, "gan": 2e-3, "gv": 1e-2}
ALL = ("A", "logits", "loss", "Pos", "Neg", "wA", "gan", "gv")

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
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(*shape):
    """An output buffer filled with NaN: an element the kernel leaves unwritten fails its comparison."""
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def _head_inputs(B, h, w, seed):
    """test_kernels_gpu._head_inputs: positive features, so the similarities sit near the epsilon thresholds
    instead of saturating every sigmoid."""
    g = torch.Generator().manual_seed(seed)
    v = (torch.randn(B, h, w, C, generator=g).abs() + 0.3 * torch.rand(B, 1, 1, C, generator=g)).to(torch.bfloat16)
    an = F.normalize(torch.randn(B, C, generator=g).abs() + 0.5, dim=1)
    return v, an


@functools.lru_cache(maxsize=None)
def _reference(B, h, w, trimap, neg, attention=False):
    """(v, an, fp64 oracle outputs, fp32 oracle outputs) of one case, computed once and shared.  attention: the
    standalone HardWayAttention takes fp32 features as given (no normalisation inside), so they are normalised
    here first -- unnormalised ones would saturate every sigmoid -- and the oracle runs with img_n = v."""
    import avenet_oracle as orc

    v, an = _head_inputs(B, h, w, 1000 + B)
    if attention:
        v = F.normalize(v.float(), dim=3)
    Pn = h * w
    outs = []
    for dt in (torch.float64, torch.float32):
        vt = v.to(dt).permute(0, 3, 1, 2).requires_grad_(True)
        at = an.to(dt).clone().requires_grad_(True)
        img_n = vt if attention else F.normalize(vt, dim=1)
        rA, rlog, rwA, rPos, rNeg = orc.hardway_head(img_n, at, EPS1, EPS2, TAU, trimap, neg)
        rloss = orc.hardway_ce(rlog)
        rloss.backward()
        outs.append({"A": rA.detach().reshape(B, Pn), "logits": rlog.detach(), "loss": rloss.detach(),
                     "Pos": rPos.detach().reshape(B, Pn), "Neg": rNeg.detach().reshape(B, Pn),
                     "wA": rwA.detach().reshape(B, Pn), "gan": at.grad,
                     "gv": vt.grad.permute(0, 2, 3, 1).reshape(B, Pn, C)})
    return v, an, outs[0], outs[1]


def _err(name, got, ref):
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.double()
    d = (got - ref).abs().max().item()
    if name == "loss":
        return d / max(1.0, abs(ref.item()))
    if name in ("gan", "gv"):
        return d / max(ref.abs().max().item(), 1e-30)
    return d


def _check(tag, got, r64, r32, names=ALL):
    """Every named output within the project's tolerance of the fp64 oracle; the fp32 oracle's own error is printed
    next to the kernel's."""
    bad = []
    for n in names:
        e, y = _err(n, got[n], r64[n]), _err(n, r32[n], r64[n])
        print(f"{tag} {n}: kernel {e:.3e}  fp32 oracle {y:.3e}  tolerance {TOL[n]:.1e}")
        if not e <= TOL[n]:
            bad.append((n, e, TOL[n]))
    assert not bad, (tag, bad)


def _forward(v, an, trimap, neg, attention=False):
    """avt_hardway_fwd (or avt_hardway_attention_fwd) + avt_hardway_ce; every buffer of the tape in a dict."""
    B, h, w, _ = v.shape
    Pn, L = h * w, B + (2 if neg else 1)
    s = {"B": B, "P": Pn, "L": L, "trimap": int(trimap), "neg": int(neg), "v": v.to(DEV).reshape(B, Pn, C),
         "an": an.to(DEV), "inv": _f32(B, Pn), "vsum": _f32(B, Pn), "A0": _f32(B, Pn, B),
         "save": _f32(int(query("avt_hardway_save_floats", B))), "logits": _f32(B, L), "A": _f32(B, Pn),
         "Pos": _f32(B, Pn), "Neg": _f32(B, Pn), "wA": _f32(B, Pn), "loss": _f32(), "dl": _f32(B, L)}
    if attention:
        assert trimap and neg
        call("avt_hardway_attention_fwd", P(s["v"]), P(s["an"]), B, Pn, C, EPS1, EPS2, TAU, P(s["inv"]), P(s["vsum"]),
             P(s["A0"]), P(s["save"]), P(s["logits"]), P(s["A"]), P(s["Pos"]), P(s["Neg"]), P(s["wA"]), S())
    else:
        call("avt_hardway_fwd", P(s["v"]), P(s["an"]), B, Pn, C, EPS1, EPS2, TAU, int(trimap), int(neg), P(s["inv"]),
             P(s["vsum"]), P(s["A0"]), P(s["save"]), P(s["logits"]), P(s["A"]), P(s["Pos"]), P(s["Neg"]), P(s["wA"]),
             S())
    call("avt_hardway_ce", P(s["logits"]), B, L, 1.0, P(s["loss"]), P(s["dl"]), S())
    return s


def _backward(s, gan=None, accumulate=0, ws=None, ex=False):
    """avt_hardway_bwd, or avt_hardway_bwd_ex with a split-K workspace; returns (gan, gv)."""
    B, Pn = s["B"], s["P"]
    dA0, dvh = _f32(B, Pn, B), _f32(B, Pn, C)
    gv = torch.full((B, Pn, C), float("nan"), device=DEV, dtype=torch.bfloat16)
    gan = _f32(B, C) if gan is None else gan
    head = (P(s["v"]), P(s["an"]), P(s["inv"]), P(s["A0"]), P(s["save"]), P(s["dl"]), B, Pn, C, EPS1, EPS2, TAU,
            s["trimap"], s["neg"], None, None, None)
    if ex:
        call("avt_hardway_bwd_ex", *head, None, None, None, P(dA0), P(dvh), P(gv), P(gan), accumulate, P(ws), S())
    else:
        call("avt_hardway_bwd", *head, P(dA0), P(dvh), P(gv), P(gan), accumulate, S())
    torch.cuda.synchronize()
    return gan, gv


# (B, h, w, tri-map, Neg column)
HEAD_CASES = [
    (63, 2, 2, True, True),    # sgemm tile tails, B mod 4 = 3
    (64, 2, 2, True, True),    # exactly one tile, aligned
    (65, 2, 2, True, True),    # a one-column tail, B mod 4 = 1
    (65, 2, 2, False, True),
    (129, 1, 3, True, True),   # a third row of tiles, odd P
    (254, 1, 2, True, True),   # L = 256: the last width of the CE kernel's register-resident body
    (255, 1, 2, True, True),   # L = 257: the first strided width
    (255, 1, 2, True, False),  # L = 256 without the Neg column
    (256, 1, 2, True, False),  # L = 257 without the Neg column
    (300, 2, 2, True, True),   # 1024 / 300 = 3 sub-threads per column, 124 idle threads
    (300, 2, 2, False, True),
    (600, 1, 1, True, True),   # 512 < B <= 1024: one sub-thread, the block's tail idles; P = 1
]


@pytest.mark.parametrize("B,h,w,trimap,neg", HEAD_CASES)
def test_head_at_batch_edges(B, h, w, trimap, neg):
    v, an, r64, r32 = _reference(B, h, w, trimap, neg)
    s = _forward(v, an, trimap, neg)
    s["gan"], s["gv"] = _backward(s)
    _check(f"head B={B} P={h * w} trimap={int(trimap)} neg={int(neg)}", s, r64, r32)


def _expected_splits(rows):
    """The split count the `gan` GEMM must arrive at: rows / 256, at most 64, then k_per_split rounded up to a
    multiple of the 32-deep k-tile and the count re-derived from it."""
    splits = min(max(rows // 256, 1), 64)
    kps = -(-rows // splits)
    kps = -(-kps // 32) * 32
    return -(-rows // kps), kps


@pytest.mark.parametrize("B,h,w", [(300, 2, 2), (65, 16, 16)])
def test_gan_split_k_ordered(B, h, w):
    """The split-K `gan` GEMM of avt_hardway_bwd_ex: (300, 2, 2) is 1200 rows in 4 splits; (65, 16, 16) is 16,640
    rows, which asks for 65 splits, is capped to 64, and after k_per_split is rounded to 288 runs 58 splits, the
    last one short (224 rows).  Workspace and gan start as NaN, so a partial that is summed without having been
    written, or an output element that is skipped, shows."""
    v, an, r64, r32 = _reference(B, h, w, True, True)
    rows = B * h * w
    splits, kps = _expected_splits(rows)
    assert (splits, kps) == {1200: (4, 320), 16640: (58, 288)}[rows] and rows % kps != 0
    nws = int(query("avt_hardway_bwd_ws_floats", B, C))
    assert nws == 64 * B * C
    s = _forward(v, an, True, True)
    tag = f"split-K B={B} rows={rows} splits={splits}"
    bound = TOL["gan"]

    gan_u, gv_u = _backward(s)  # avt_hardway_bwd: no workspace, one split
    runs = []
    for _ in range(2):
        ws = _f32(nws)
        gan, gv = _backward(s, ws=ws, ex=True)
        # exactly `splits` dense B x C partials were written, nothing behind them
        assert torch.isfinite(ws[:splits * B * C]).all() and torch.isnan(ws[splits * B * C:]).all()
        runs.append((gan, gv))
    assert torch.equal(runs[0][0], runs[1][0]), "the ordered split-K sum is not repeatable"
    assert torch.equal(runs[0][1].view(torch.int16), runs[1][1].view(torch.int16))
    _check(tag + " accumulate=0", {"gan": runs[0][0], "gv": runs[0][1]}, r64, r32, ("gan", "gv"))
    _check(tag + " unsplit", {"gan": gan_u, "gv": gv_u}, r64, r32, ("gan", "gv"))
    e_su = _err("gan", runs[0][0], gan_u.cpu())
    print(f"{tag}: split vs unsplit {e_su:.3e}  bound {bound:.3e}")
    assert e_su <= bound

    # gan_accumulate = 1 onto a known gan0 of the gradient's own magnitude: gan0 + gan_ref, up to the bound on the
    # gradient plus the one fp32 rounding of the final addition
    gscale = r64["gan"].abs().max().item()
    gan0 = torch.randn(B, C, generator=torch.Generator().manual_seed(7)) * gscale
    want = gan0.double() + r64["gan"]
    acc = []
    for _ in range(2):
        gan, _ = _backward(s, gan=gan0.to(DEV).clone(), accumulate=1, ws=_f32(nws), ex=True)
        acc.append(gan)
    assert torch.equal(acc[0], acc[1]), "the accumulating split-K sum is not repeatable"
    e_acc = (acc[0].double().cpu() - want).abs().max().item() / gscale
    b_acc = bound + 2.0 ** -24 * want.abs().max().item() / gscale
    print(f"{tag} accumulate=1: kernel {e_acc:.3e}  bound {b_acc:.3e}")
    assert e_acc <= b_acc
    # and without a workspace (one split, the GEMM's own read-modify-write epilogue)
    gan_a1, _ = _backward(s, gan=gan0.to(DEV).clone(), accumulate=1)
    e_a1 = (gan_a1.double().cpu() - want).abs().max().item() / gscale
    print(f"{tag} accumulate=1 unsplit: kernel {e_a1:.3e}  bound {b_acc:.3e}")
    assert e_a1 <= b_acc


@pytest.mark.parametrize("B,h,w", [(65, 2, 2), (255, 1, 2)])
def test_attention_head_at_batch_edges(B, h, w):
    """avt_hardway_attention_fwd / _bwd (fp32 features taken as given) against the same oracle with img_n = v."""
    v, an, r64, r32 = _reference(B, h, w, True, True, attention=True)
    s = _forward(v, an, True, True, attention=True)
    Pn = h * w
    dA0, dvh, gv, gan = _f32(B, Pn, B), _f32(B, Pn, C), _f32(B, Pn, C), _f32(B, C)
    ws = _f32(int(query("avt_hardway_bwd_ws_floats", B, C)))
    call("avt_hardway_attention_bwd", P(s["v"]), P(s["an"]), P(s["inv"]), P(s["A0"]), P(s["save"]), P(s["dl"]), None,
         B, Pn, C, EPS1, EPS2, TAU, P(dA0), P(dvh), P(gv), P(gan), P(ws), S())
    torch.cuda.synchronize()
    s["gan"], s["gv"] = gan, gv
    assert torch.equal(s["inv"], torch.ones_like(s["inv"]))  # no normalisation inside
    _check(f"attention B={B} P={Pn}", s, r64, r32)


# ------------------------------------------------------------------------------------------ cross-entropy alone
CE_CASES = [(1, 3), (5, 7), (3, 64), (64, 65), (17, 256), (17, 257), (66, 300), (70, 1000)]


@functools.lru_cache(maxsize=None)
def _ce_logits(B, L, fill):
    g = torch.Generator().manual_seed(100 * B + L)
    if fill == "randn":
        return torch.randn(B, L, generator=g)
    # the head's profile: everything in [-14, 14] (a similarity in [-1, 1] over 0.07) but one column per row at
    # +-1414 (the -99 / 0.07 diagonal), never column 0
    x = torch.rand(B, L, generator=g) * 28 - 14
    col = torch.randint(1, L, (B,), generator=g)
    sign = torch.where(torch.arange(B) % 3 == 1, 1.0, -1.0)  # mostly negative, as the head's; some positive
    x[torch.arange(B), col] = 1414.0 * sign
    return x


def _ce_ref(x, scale, dtype):
    t = x.to(dtype).clone().requires_grad_(True)
    loss = F.cross_entropy(t, torch.zeros(x.shape[0], dtype=torch.long))
    loss.backward()
    return loss.detach().double(), t.grad.double() * scale


def _ce_check(B, L, fill, scale=1.0, want_loss=True, want_grad=True):
    x = _ce_logits(B, L, fill)
    rl, rg = _ce_ref(x, scale, torch.float64)
    yl, yg = _ce_ref(x, scale, torch.float32)
    loss = _f32() if want_loss else None
    dl = _f32(B, L) if want_grad else None
    call("avt_hardway_ce", P(x.to(DEV)), B, L, scale, P(loss), P(dl), S())
    torch.cuda.synchronize()
    tag = f"ce B={B} L={L} {fill} scale={scale}"
    if want_loss:
        assert torch.isfinite(loss).all()
        e, y = abs(loss.item() - rl.item()), abs(yl.item() - rl.item())
        bound = max(1e-5 * abs(rl.item()), 3 * y)
        print(f"{tag} loss {rl.item():.6g}: kernel {e:.3e}  torch fp32 {y:.3e}  bound {bound:.3e}")
        assert e <= bound
    if want_grad:
        assert torch.isfinite(dl).all()
        d = dl.double().cpu()
        gmax = rg.abs().max().item()
        e, y = (d - rg).abs().max().item() / gmax, (yg - rg).abs().max().item() / gmax
        bound = max(1e-5, 3 * y)
        print(f"{tag} dlogits: kernel {e:.3e}  torch fp32 {y:.3e}  bound {bound:.3e}")
        assert e <= bound
        # each row is (softmax - onehot) * scale / B and sums to zero up to the fp32 roundings that form it: the
        # log-sum-exp is held in fp32 (a few ulps of |lse|: its own rounding, logf, the shuffle sum of up to 1024
        # terms), every x - lse and expf rounds once more (weighted by the softmax, at most the row's entropy
        # <= log L in total), and the - 1, * scale and / B round the result
        lse = torch.logsumexp(x.double(), dim=1).abs()
        rs_bound = scale / B * 2.0 ** -24 * (4 * lse + math.log(L) + 16)
        rs = d.sum(dim=1).abs()
        print(f"{tag} row sums: max {rs.max().item():.3e}  (bound of that row "
              f"{rs_bound[rs.argmax()].item():.3e})")
        assert (rs <= rs_bound).all()


@pytest.mark.parametrize("fill", ["randn", "head"])
@pytest.mark.parametrize("B,L", CE_CASES)
def test_ce_alone(B, L, fill):
    """avt_hardway_ce on synthetic logits against F.cross_entropy in fp64 and its autograd gradient: both sides of
    the L = 256 boundary, a partial last group of four rows, more than 64 rows (a wave's second row group), and
    the head's +-1414 entries, where a slip in the max subtraction or the log-sum-exp would show."""
    _ce_check(B, L, fill)


@pytest.mark.parametrize("fill", ["randn", "head"])
@pytest.mark.parametrize("B,L", [(5, 7), (17, 256), (17, 257), (66, 300)])
@pytest.mark.parametrize("variant", ["scale", "loss_only", "grad_only"])
def test_ce_variants(B, L, fill, variant):
    """scale = 0.5 (dlogits scaled, the loss not: the two-view step scales the CE itself), dlogits = NULL,
    loss = NULL."""
    if variant == "scale":
        _ce_check(B, L, fill, scale=0.5)
    elif variant == "loss_only":
        _ce_check(B, L, fill, want_grad=False)
    else:
        _ce_check(B, L, fill, want_loss=False)
