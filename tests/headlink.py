"""The link oracle of the hard-way head (csrc/head.hip): CPU, fp64, torch + numpy only; nothing from the library.

The head is eleven launches joined by a tape (inv, vsum, A0, save, dA0, dm, dvh).  Each function here takes ONE
launch's inputs as the GPU left them (its own bits, moved to the CPU), recomputes that one link in fp64 and compares
with what the launch wrote, element by element, against a bound that follows from the launch's own arithmetic.
Nothing is amplified: the normalise-backward projection, which turns 1e-6 on dvh into 1e-2 of max|gv| end to end,
here only sees its own roundings.  u = 2^-24, g(n) = n u / (1 - n u) (n fp32 roundings in a row).

  norm      vsum: g(C/8 + 8) sum|x|  (a lane's 8 ceil(C/512) terms in turn, six shuffle levels, the products);
            inv: the same relative error on sum x^2, halved by the square root, + 1 ulp each for sqrt and divide;
            the attention form (no normalisation): inv == 1 exactly
  a0        inv * sum_c v an:  g(C + 2) inv sum_c |v an|   (fp32 products, C fp32 additions, the row scale)
  logits    A == A0[i, :, i] exactly.  Every other output is a function of w = sigm((x - eps) / tau):
            |dw| <= (K_SIG + 3 Y) u [w (1 - w) (1 + |z|) + w]      -- the "sigmoid unit" in brackets is how an error
            of u |z| in the argument, of u in exp and of u in 1 + e and 1 / . moves w; K_SIG = 4 of it cover the
            roundings the kernel's source shows (x - eps, 1 / tau, the product; 1 + e, the divide); the intrinsic
            __expf is not derivable here, so its share is 3 Y units, Y = the largest error IN THE SAME UNIT of
            torch's fp32 sigmoid((x - eps) / tau) on the CPU against fp64 over the case's own arguments (the rule of
            tests/gradcheck.py: 3 x the reference's own fp32 error, never the kernel's).  Y is computed per case
            and printed.  dw is then propagated through the sums over P (g(depth) on the sum of magnitudes), the
            quotients (1 ulp) and the  * -99 / 0.07f  (4 u); pn = 1 / max(||Pos||, 1e-12f) takes the clamp when
            the norm and its error are below the constant (both precisions then agree exactly)
  logits_bwd, wa_bwd, aux_bwd   the same propagation through the kernels' expressions, term by term, on the
            magnitudes (w + wd (x - s) may cancel: the bound does not); off the diagonal the two diagonal kernels
            must leave dA0 BIT-IDENTICAL
  dvh       g(B + 2) sum_j |dA0 an|
  gan       g(rows + splits + 3) sum_k |dA0 inv v|  (+ u |gan0 + .| when accumulating)
  norm_bwd  dot = inv sum x (dvh + dm / C) as norm's sum, propagated through inv (e - x inv dot), then one bf16
            rounding: HALF A bf16 ULP OF THE RESULT, 2^-9 of the power of two above it (never more than 2^-8 |gv|:
            fwdlink's apply bound is its upper envelope) + bf16's smallest subnormal.  The fp32 gv of the attention
            form (gv = dvh) is exact.

Constants enter as the kernels see them: eps1, eps2, tau as fp32, 0.07f, 1e-12f.

Each function returns records (name, link, worst error / bound, index); a record is out of bound when its ratio
exceeds 1 (exact checks give 0 or inf).  emulate_head is the reference emulation: the eleven launches in torch fp32
on the CPU, filling the same tape.  It is the stand-in for the GPU in tests/test_head_links_cpu.py and the carrier of
the faults that file injects (FAULTS).  oracle_e2e is the end-to-end fp64 autograd reference the older tests use,
for the reading of their tolerances (OLD_TOL) on the same faults.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from fwdlink import INF, exact, failures, worst  # noqa: F401  (re-exported for the tests)

U = 2.0 ** -24
ULP = 2.0 ** -23
K_SIG = 4.0
EPS1, EPS2, TAU = 0.65, 0.4, 0.03
TINY_BF16 = 2.0 ** -133
F32_TINY = 2.0 ** -149
# tests/test_head_edges_gpu.py's TOL (the GPU test asserts the two are the same)
OLD_TOL = {"A": 1e-5, "logits": 2e-3, "loss": 1e-5, "Pos": 1e-3, "Neg": 1e-3, "wA": 1e-5, "gan": 2e-3, "gv": 1e-2}
LINKS = ("norm", "a0", "logits", "ce", "logits_bwd", "wa_bwd", "aux_bwd", "dvh", "gan", "norm_bwd")


def gam(n):
    return n * U / (1.0 - n * U)


def f32c(x):
    """A C `float` argument or literal as the kernel sees it, as a Python float."""
    return float(np.float32(x))


def _consts(eps):
    e1, e2, tau = (f32c(e) for e in eps)
    return e1, e2, 1.0 / tau


def expected_splits(rows):
    """tests/test_head_edges_gpu._expected_splits restated (the GPU test asserts they agree)."""
    splits = min(max(rows // 256, 1), 64)
    kps = -(-rows // splits)
    kps = -(-kps // 32) * 32
    return -(-rows // kps), kps


def _depth_block(n, nthr):
    """Additions an element passes through in block_sum over n terms strided over nthr threads."""
    return -(-n // nthr) + 6 + nthr // 64


# ----------------------------------------------------------------------------------------------------------------
# the sigmoid and its yardstick
# ----------------------------------------------------------------------------------------------------------------

def _sig_unit(z, w):
    return U * (w * (1 - w) * (1 + z.abs()) + w)


def sig_yardstick(x: torch.Tensor, e: float, tau: float, sign: float = 1.0) -> float:
    """Y: the largest error, in sigmoid units, of torch's fp32 sigmoid(sign (x - e) / tau) against fp64 on the fp32
    arguments x."""
    x64 = x.double()
    z = sign * (x64 - f32c(e)) / f32c(tau)
    w = torch.sigmoid(z)
    x32 = x.float()
    w32 = torch.sigmoid((x32 - torch.tensor(e, dtype=torch.float32)) / torch.tensor(tau, dtype=torch.float32) * sign)
    return float(((w32.double() - w).abs() / _sig_unit(z, w)).max())


def _sig(x64, e, it, Y, sign=1.0):
    z = sign * (x64 - e) * it
    w = torch.sigmoid(z)
    return w, (K_SIG + 3.0 * Y) * _sig_unit(z, w)


def _norm_clamped(pp, dpp, n_terms):
    """nrm = sqrt(pp), den = max(nrm, 1e-12f), pn = 1 / den with their error bounds, from pp (fp64) and its relative-
    form bound dpp.  Below the fp32 normal range the squares lose bits absolutely: n_terms 2^-149 more on pp, taken
    through |sqrt(a + d) - sqrt(a)| <= sqrt(d).  When nrm + dnrm < 1e-12f both precisions clamp and den is exact."""
    c = f32c(1e-12)
    nrm = pp.sqrt()
    dn_rel = torch.where(nrm > 0, dpp / (2 * nrm.clamp_min(1e-300)) * 1.001, torch.zeros_like(nrm))
    dnrm = torch.minimum(dn_rel, dpp.sqrt()) + math.sqrt(n_terms * F32_TINY) + ULP * nrm
    clamped = nrm + dnrm < c
    free = nrm - dnrm > c
    den = nrm.clamp_min(c)
    dden = torch.where(clamped, torch.zeros_like(nrm), dnrm)
    pn = 1.0 / den
    dpn = pn * (dden / (den - dden).clamp_min(1e-300) + ULP)
    return nrm, pn, dpn, clamped, free


# ----------------------------------------------------------------------------------------------------------------
# links
# ----------------------------------------------------------------------------------------------------------------

def norm_link(v, inv, vsum, attention=False):
    """vis_norm_kernel: v [B, P, C] -> inv, vsum [B, P]."""
    x = v.double()
    C = x.shape[-1]
    g = gam(C // 8 + 8)
    s = x.sum(-1)
    rec = [("vsum", "norm", *worst((vsum.double() - s).abs(), g * x.abs().sum(-1)))]
    if attention:
        return rec + [("inv", "norm", *exact(inv == 1.0))]
    ss = (x * x).sum(-1)
    i64 = 1.0 / ss.sqrt().clamp_min(f32c(1e-12))
    rel = (0.5 * g * (1 + g) + 2 * ULP) * 1.001
    return rec + [("inv", "norm", *worst((inv.double() - i64).abs(), rel * i64))]


def a0_link(v, an, inv, A0):
    """sgemm_kernel, A0[(i, p), j] = inv[(i, p)] sum_c v[(i, p), c] an[j, c], inv from the tape."""
    B, P, C = v.shape
    x, a, iv = v.double().reshape(B * P, C), an.double(), inv.double().reshape(B * P, 1)
    ref = (x @ a.T) * iv
    mag = (x.abs() @ a.abs().T) * iv
    return [("A0", "a0", *worst((A0.double().reshape(B * P, B) - ref).abs(), gam(C + 2) * mag))]


def _masks(B, dtype=torch.float64):
    return torch.where(torch.eye(B, dtype=torch.bool), -99.0, 1.0).to(dtype)


def _diag(A0):
    """A0 [B, P, B] -> [B, P], element (i, p) = A0[i, p, i]."""
    return A0.diagonal(dim1=0, dim2=2).transpose(0, 1)


def logits_yardsticks(A0, trimap, eps=(EPS1, EPS2, TAU)):
    """(Y of sigm((x - eps1) / tau) over all of A0, Y of the Neg sigmoid over its diagonal)."""
    y1 = sig_yardstick(A0, eps[0], eps[2])
    y2 = sig_yardstick(_diag(A0), eps[1] if trimap else eps[0], eps[2], -1.0)
    return y1, y2


def logits_link(A0, vsum, inv, C, trimap, neg, save, logits, A, Pos, Neg, wA, eps=(EPS1, EPS2, TAU), yard=None):
    """hardway_logits_kernel from the tape's A0, vsum, inv."""
    B, P, _ = A0.shape
    e1, e2, it = _consts(eps)
    y1, y2 = yard if yard is not None else logits_yardsticks(A0, trimap, eps)
    x = A0.double()
    sv = save.double().reshape(B, 2 * B + 4)
    L = B + (2 if neg else 1)
    c07 = f32c(0.07)
    # the column loop: nsub threads per column, each ceil(P / nsub) terms in turn, then nsub partials in turn
    nsub = max(1024 // min(B, 1024), 1)
    n = -(-P // nsub) + nsub
    w, dw = _sig(x, e1, it, y1)
    sw, swx, aswx = w.sum(1), (w * x).sum(1), (w * x.abs()).sum(1)
    dsw = dw.sum(1) + gam(n) * sw
    dswx = (dw * x.abs()).sum(1) + gam(n + 1) * aswx
    s = swx / sw
    ds = (dswx + s.abs() * dsw) / (sw - dsw).clamp_min(1e-300) + ULP * s.abs()
    m = _masks(B)
    lg = s * m / c07
    dlg = ds * m.abs() / c07 + 4 * U * lg.abs()
    lo = logits.double()
    rec = [("save.s", "logits", *worst((sv[:, :B] - s).abs(), ds)),
           ("save.W", "logits", *worst((sv[:, B:2 * B] - sw).abs(), dsw)),
           ("logits.sim", "logits", *worst((lo[:, 1:1 + B] - lg).abs(), dlg)),
           ("A", "logits", *exact(A == _diag(A0)))]
    # the diagonal: block_sum over P
    nb = _depth_block(P, 1024)
    xd = _diag(x)
    w1, dw1 = _sig(xd, e1, it, y1)
    w2, dw2 = _sig(xd, e2 if trimap else e1, it, y2, -1.0)
    rec += [("Pos", "logits", *worst((Pos.double() - w1).abs(), dw1)),
            ("Neg", "logits", *worst((Neg.double() - w2).abs(), dw2))]
    for k, (wk, dwk, col) in enumerate(((w1, dw1, 0), (w2, dw2, B + 1))):
        W, X = wk.sum(1), (wk * xd).sum(1)
        dW = dwk.sum(1) + gam(nb) * W
        dX = (dwk * xd.abs()).sum(1) + gam(nb + 1) * (wk * xd.abs()).sum(1)
        sk = X / W
        dsk = (dX + sk.abs() * dW) / (W - dW).clamp_min(1e-300) + ULP * sk.abs()
        rec += [(f"save.s{k + 1}", "logits", *worst((sv[:, 2 * B + 2 * k] - sk).abs(), dsk)),
                (f"save.W{k + 1}", "logits", *worst((sv[:, 2 * B + 2 * k + 1] - W).abs(), dW))]
        if col < L:
            rec.append((f"logits.s{k + 1}", "logits",
                        *worst((lo[:, col] - sk / c07).abs(), dsk / c07 + 2 * U * (sk / c07).abs())))
    pp = (w1 * w1).sum(1)
    dpp = (2 * w1 * dw1).sum(1) + gam(nb + 1) * pp
    _, pn, dpn, _, _ = _norm_clamped(pp, dpp, P + nb)
    mm = vsum.double() * inv.double() / C
    ref = mm * w1 * pn[:, None]
    dref = mm.abs() * (dw1 * pn[:, None] + w1 * dpn[:, None]) + 6 * U * ref.abs()
    rec.append(("wA", "logits", *worst((wA.double() - ref).abs(), dref)))
    return rec


def ce_link(logits, loss, dl, scale=1.0):
    """hardway_ce_kernel from the tape's logits: lse = mx + logf(sum expf(x - mx)) per row (a wave: L / 64 terms per
    lane in turn, six shuffle levels), loss = mean(lse - x0), dl = (expf(x - lse) - [j = 0]) scale / B.  expf and logf
    are the library functions (1 ulp each, as documented), not intrinsics: d lse <= u (|mx| + 2 |lse|) + the relative
    error of the sum, (depth + 3) u; d softmax <= softmax (d lse + u |x - lse| + 2 ulp)."""
    x = logits.double()
    B, L = x.shape
    mx = x.max(1, keepdim=True).values
    lse = torch.logsumexp(x, 1, keepdim=True)
    dlse = U * (mx.abs() + 2 * lse.abs()) + gam(-(-L // 64) + 6 + 3) + 2 * ULP
    sm = torch.exp(x - lse)
    dsm = sm * (dlse + U * (x - lse).abs() + 2 * ULP) * 1.001
    hot = torch.zeros_like(x)
    hot[:, 0] = 1
    ref = (sm - hot) * scale / B
    rec = [("dlogits", "ce", *worst((dl.double() - ref).abs(), dsm * scale / B + 3 * U * ref.abs()))]
    per = lse[:, 0] - x[:, 0]
    dper = dlse[:, 0] + U * per.abs()
    nb = -(-B // 16) + 6 + 16
    lref = per.mean()
    rec.append(("loss", "ce", *worst((loss.double() - lref).abs().reshape(1),
                                     (dper.mean() + gam(nb + 1) * per.abs().mean()).reshape(1))))
    return rec


def _logit_terms(x, sk, Wk, dsk_dl, w, dw, it, sign):
    """dsk_dl * (w + wd (x - sk)) / Wk and its bound; wd = sign w (1 - w) / tau."""
    wd = sign * w * (1 - w) * it
    dwd = (1 - 2 * w).abs() * dw * it + 5 * U * wd.abs()
    t = x - sk
    N = w + wd * t
    dN = dw + t.abs() * dwd + 3 * U * (wd * t).abs() + U * (w + (wd * t).abs())
    term = dsk_dl * N / Wk
    return term, (dsk_dl / Wk).abs() * dN + 8 * U * (dsk_dl / Wk).abs() * (w + (wd * t).abs())


def logits_bwd_link(A0, save, dl, trimap, neg, dA0, eps=(EPS1, EPS2, TAU), yard=None):
    """hardway_logits_bwd_kernel from the tape's A0, save and dlogits: dA0 before the diagonal kernels."""
    B, P, _ = A0.shape
    e1, e2, it = _consts(eps)
    y1, y2 = yard if yard is not None else logits_yardsticks(A0, trimap, eps)
    x, sv, d = A0.double(), save.double().reshape(B, 2 * B + 4), dl.double()
    c07 = f32c(0.07)
    w, dw = _sig(x, e1, it, y1)
    dsim = (d[:, 1:1 + B] * _masks(B) / c07)[:, None, :]
    g, dg = _logit_terms(x, sv[:, None, :B], sv[:, None, B:2 * B], dsim, w, dw, it, 1.0)
    # the diagonal's two more terms
    xd = _diag(x)
    w1, dw1 = _sig(xd, e1, it, y1)
    t1, dt1 = _logit_terms(xd, sv[:, 2 * B, None], sv[:, 2 * B + 1, None], (d[:, 0] / c07)[:, None], w1, dw1, it, 1.0)
    gd, dgd = _diag(g) + t1, _diag(dg) + dt1 + U * (_diag(g).abs() + t1.abs())
    if neg:
        w2, dw2 = _sig(xd, e2 if trimap else e1, it, y2, -1.0)
        t2, dt2 = _logit_terms(xd, sv[:, 2 * B + 2, None], sv[:, 2 * B + 3, None], (d[:, B + 1] / c07)[:, None],
                               w2, dw2, it, -1.0)
        dgd = dgd + dt2 + U * (gd.abs() + t2.abs())
        gd = gd + t2
    g, dg = g.clone(), dg.clone()
    _diag(g).copy_(gd)
    _diag(dg).copy_(dgd)
    return [("dA0", "logits_bwd", *worst((dA0.double() - g).abs(), dg))]


def _offdiag_same(name, link, before, after):
    B = before.shape[0]
    same = (before == after) | (torch.isnan(before) & torch.isnan(after))
    same = same | torch.eye(B, dtype=torch.bool)[:, None, :]
    return (name, link, *exact(same))


def wa_bwd_link(A0, dwA, vsum, inv, C, dA0_before, dA0_after, dm, eps=(EPS1, EPS2, TAU), yard=None):
    """hardway_wa_bwd_kernel: the diagonal of dA0 and dm from the tape's A0, vsum, inv, dwA; the rest of dA0
    bitwise untouched.  A row whose ||Pos|| cannot be told from 1e-12f within its own bound has no reference
    (the projection is discontinuous there) and fails the `margin` record."""
    B, P, _ = A0.shape
    e1, _, it = _consts(eps)
    y1 = (yard if yard is not None else logits_yardsticks(A0, True, eps))[0]
    xd = _diag(A0.double())
    w, dw = _sig(xd, e1, it, y1)
    g = dwA.double()
    m = vsum.double() * inv.double() / C
    dmm = 4 * U * m.abs()
    nb = _depth_block(P, 256)
    pp = (w * w).sum(1)
    dpp = (2 * w * dw).sum(1) + gam(nb + 1) * pp
    nrm, pn, dpn, clamped, free = _norm_clamped(pp, dpp, P + nb)
    a = g * m
    da = g.abs() * dmm + U * a.abs()
    dot = (w * a).sum(1)
    ddot = (dw * a.abs() + w * da).sum(1) + gam(nb + 2) * (w * a.abs()).sum(1)
    proj = torch.where(clamped, torch.zeros_like(dot), dot * pn * pn)
    dproj = torch.where(clamped, torch.zeros_like(dot),
                        ddot * pn * pn + dot.abs() * 2 * pn * dpn * 1.001 + 2 * U * proj.abs())
    pn_, dpn_, proj_, dproj_ = pn[:, None], dpn[:, None], proj[:, None], dproj[:, None]
    b = w * proj_
    db = dw * proj_.abs() + w * dproj_ + U * b.abs()
    dpos = (a - b) * pn_
    ddpos = (da + db + U * (a.abs() + b.abs())) * pn_ + (a - b).abs() * dpn_ + U * dpos.abs()
    k = w * (1 - w) * it
    dk = (1 - 2 * w).abs() * dw * it + 4 * U * k
    upd = dpos * k
    dupd = ddpos * k + dpos.abs() * dk + U * upd.abs()
    want = _diag(dA0_before.double()) + upd
    dwant = dupd + U * (want.abs() + dupd)
    dmr = g * w * pn_
    ddm = g.abs() * (dw * pn_ + w * dpn_) + 2 * U * dmr.abs()
    return [("margin", "wa_bwd", *exact(clamped | free)),
            ("dA0.diag", "wa_bwd", *worst((_diag(dA0_after.double()) - want).abs(), dwant)),
            _offdiag_same("dA0.offdiag", "wa_bwd", dA0_before, dA0_after),
            ("dm", "wa_bwd", *worst((dm.double() - dmr).abs(), ddm))]


def aux_bwd_link(A0, gA, gPos, gNeg, trimap, dA0_before, dA0_after, eps=(EPS1, EPS2, TAU), yard=None):
    """hardway_aux_bwd_kernel: dA0[i, p, i] += gA + gPos Pos (1 - Pos) / tau - gNeg Neg (1 - Neg) / tau."""
    e1, e2, it = _consts(eps)
    y1, y2 = yard if yard is not None else logits_yardsticks(A0, trimap, eps)
    xd = _diag(A0.double())
    g = torch.zeros_like(xd) if gA is None else gA.double().clone()
    dg = torch.zeros_like(xd)
    for gk, e, y, sign in ((gPos, e1, y1, 1.0), (gNeg, e2 if trimap else e1, y2, -1.0)):
        if gk is None:
            continue
        w, dw = _sig(xd, e, it, y, sign)
        k = w * (1 - w) * it
        dk = (1 - 2 * w).abs() * dw * it + 4 * U * k
        t = gk.double() * k
        dg = dg + gk.double().abs() * dk + U * t.abs() + U * (g.abs() + t.abs())
        g = g + sign * t
    want = _diag(dA0_before.double()) + g
    return [("dA0.diag", "aux_bwd", *worst((_diag(dA0_after.double()) - want).abs(), dg + U * (want.abs() + dg))),
            _offdiag_same("dA0.offdiag", "aux_bwd", dA0_before, dA0_after)]


def dvh_link(dA0, an, dvh):
    """sgemm_kernel, dvh[(i, p), c] = sum_j dA0[(i, p), j] an[j, c]."""
    B, P, _ = dA0.shape
    d, a = dA0.double().reshape(B * P, B), an.double()
    return [("dvh", "dvh", *worst((dvh.double().reshape(B * P, -1) - d @ a).abs(), gam(B + 2) * (d.abs() @ a.abs())))]


def gan_link(dA0, inv, v, gan, splits=1, gan0=None):
    """sgemm_kernel (+ sgemm_sum_splits_kernel), gan[j, c] (+)= sum_(i, p) dA0[(i, p), j] inv[(i, p)] v[(i, p), c]."""
    B, P, C = v.shape
    rows = B * P
    d = dA0.double().reshape(rows, B) * inv.double().reshape(rows, 1)
    x = v.double().reshape(rows, C)
    ref, bound = d.T @ x, gam(rows + splits + 3) * (d.abs().T @ x.abs())
    if gan0 is not None:
        ref = gan0.double() + ref
        bound = bound + U * (ref.abs() + bound)
    return [("gan", "gan", *worst((gan.double() - ref).abs(), bound))]


def norm_bwd_link(v, inv, dvh, dm, gv, attention=False):
    """vis_norm_bwd_kernel: gv = inv (e - x inv dot), e = dvh + dm / C, dot = inv sum_c x e; bf16 out.  The
    attention form (fp32, no normalisation, no dm): gv == dvh bitwise."""
    if attention:
        return [("gv", "norm_bwd", *exact(gv == dvh))]
    x, iv, d = v.double(), inv.double()[..., None], dvh.double()
    C = x.shape[-1]
    if dm is None:
        e, de = d, torch.zeros_like(d)
    else:
        dmc = dm.double()[..., None] / C
        e = d + dmc
        de = ULP * dmc.abs() + U * e.abs()
    n = C // 8 + 8 + 1
    raw = (x * e).sum(-1, keepdim=True)
    draw = (x.abs() * de).sum(-1, keepdim=True) + gam(n) * (x * e).abs().sum(-1, keepdim=True)
    dot = raw * iv
    ddot = draw * iv + U * dot.abs()
    q = x * iv * dot
    dq = (x * iv).abs() * ddot + 2 * U * q.abs()
    o = iv * (e - q)
    do = iv * (de + dq + U * (e.abs() + q.abs())) + U * o.abs()
    half_ulp = torch.exp2(torch.floor(torch.log2((o.abs() + do).clamp_min(1e-300))) - 8)
    return [("gv", "norm_bwd", *worst((gv.double() - o).abs(), do + half_ulp + TINY_BF16))]


def head_links(tp, C, trimap=True, neg=True, attention=False, splits=1, gan0=None, eps=(EPS1, EPS2, TAU),
               forward=True, backward=True):
    """Every link of a head tape in launch order.  tp (CPU tensors): v, an, inv, vsum, A0, save, logits, A, Pos, Neg,
    wA; the backward adds dl, dA0_pre (after hardway_logits_bwd_kernel alone), optionally dwA + dA0_wa + dm (after
    hardway_wa_bwd_kernel) and gA / gPos / gNeg, dA0 (what the GEMMs read), dvh + gv (absent: detached), gan.
    Returns (records, (Y_pos, Y_neg))."""
    yard = logits_yardsticks(tp["A0"], trimap, eps)
    rec = []
    if forward:
        rec += norm_link(tp["v"], tp["inv"], tp["vsum"], attention)
        rec += a0_link(tp["v"], tp["an"], tp["inv"], tp["A0"])
        rec += logits_link(tp["A0"], tp["vsum"], tp["inv"], C, trimap, neg, tp["save"], tp["logits"], tp["A"],
                           tp["Pos"], tp["Neg"], tp["wA"], eps, yard)
        if tp.get("loss") is not None:
            rec += ce_link(tp["logits"], tp["loss"], tp["dl"])
    if backward:
        rec += logits_bwd_link(tp["A0"], tp["save"], tp["dl"], trimap, neg, tp["dA0_pre"], eps, yard)
        cur = tp["dA0_pre"]
        if tp.get("dwA") is not None:
            rec += wa_bwd_link(tp["A0"], tp["dwA"], tp["vsum"], tp["inv"], C, cur, tp["dA0_wa"], tp["dm"], eps, yard)
            cur = tp["dA0_wa"]
        aux = [tp.get(k) for k in ("gA", "gPos", "gNeg")]
        if any(a is not None for a in aux):
            rec += aux_bwd_link(tp["A0"], *aux, trimap, cur, tp["dA0"], eps, yard)
        else:
            same = (cur == tp["dA0"]) | (torch.isnan(cur) & torch.isnan(tp["dA0"]))
            rec.append(("dA0.chain", "aux_bwd", *exact(same)))
        if tp.get("dvh") is not None:
            rec += dvh_link(tp["dA0"], tp["an"], tp["dvh"])
        rec += gan_link(tp["dA0"], tp["inv"], tp["v"], tp["gan"], splits, gan0)
        if tp.get("dvh") is not None:
            rec += norm_bwd_link(tp["v"], tp["inv"], tp["dvh"], tp.get("dm") if tp.get("dwA") is not None else None,
                                 tp["gv"], attention)
    return rec, yard


def worst_by_link(records):
    out = {}
    for r in records:
        if r[1] not in out or not r[2] <= out[r[1]][2]:
            out[r[1]] = r
    return out


def report(tag, records, yard=None):
    w = worst_by_link(records)
    y = "" if yard is None else f"  [fp32 sigmoid yardstick Y: Pos {yard[0]:.2f}, Neg {yard[1]:.2f} units]"
    return f"{tag}: " + ", ".join(f"{k} {w[k][2]:.3f} ({w[k][0]}@{w[k][3]})" for k in LINKS if k in w) + y


def first_failing_link(records):
    bad = failures(records)
    return bad[0][1] if bad else None


# ----------------------------------------------------------------------------------------------------------------
# draws
# ----------------------------------------------------------------------------------------------------------------

def draw_positive(B, h, w, C, seed):
    """tests/test_head_edges_gpu._head_inputs at any C: positive features, similarities near the thresholds."""
    g = torch.Generator().manual_seed(seed)
    v = (torch.randn(B, h, w, C, generator=g).abs() + 0.3 * torch.rand(B, 1, 1, C, generator=g)).to(torch.bfloat16)
    an = F.normalize(torch.randn(B, C, generator=g).abs() + 0.5, dim=1)
    return v, an


def _vhat(v):
    return F.normalize(v.float(), dim=-1)


def draw_mixed(B, h, w, C, seed):
    """Half the pairs (even i) get an[i] near +vhat, half near -vhat (vhat: the pair's mean feature direction), so A
    spans about [-0.9, 0.9] and the odd rows have every Pos far below 1e-20: the clamp of weighted_A."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(B, 1, 1, C, generator=g)
    v = (base + 0.35 * torch.randn(B, h, w, C, generator=g)).to(torch.bfloat16)
    d = _vhat(v).mean(dim=(1, 2))
    sign = torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0)[:, None]
    an = F.normalize(sign * F.normalize(d, dim=1) + 0.25 * torch.randn(B, C, generator=g) / math.sqrt(C), dim=1)
    return v, an


def draw_threshold(B, h, w, C, seed, eps=(EPS1, EPS2, TAU)):
    """A[i, p] within +-2 tau of eps1 (even positions) or eps2 (odd positions): v[i, p] = t an[i] + sqrt(1 - t^2) n,
    n a unit vector orthogonal to an[i], t the target similarity."""
    g = torch.Generator().manual_seed(seed)
    an = F.normalize(torch.randn(B, C, generator=g), dim=1)
    P = h * w
    n = torch.randn(B, P, C, generator=g)
    n = F.normalize(n - (n * an[:, None]).sum(-1, keepdim=True) * an[:, None], dim=-1)
    centre = torch.where(torch.arange(P) % 2 == 0, eps[0], eps[1])[None, :]
    t = centre + (torch.rand(B, P, generator=g) * 4 - 2) * eps[2]
    v = 3.0 * (t[..., None] * an[:, None] + (1 - t * t).sqrt()[..., None] * n)
    return v.reshape(B, h, w, C).to(torch.bfloat16), an


DRAWS = {"positive": draw_positive, "mixed": draw_mixed, "threshold": draw_threshold}


def draw_cotangents(B, P, seed, names=("dwA", "gA", "gPos", "gNeg")):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(B, P, generator=g) for k in names}


# ----------------------------------------------------------------------------------------------------------------
# the reference emulation
# ----------------------------------------------------------------------------------------------------------------

FAULTS = ("ktail_a0", "ktail_dvh", "ktail_gan", "stale_col", "split_twice", "save_w_next", "mask_next",
          "dm_not_in_dot", "diag_before_store", "gan_acc_twice", "pn_wrong_side", "neg_eps1")
# the link each fault touches
FAULT_LINK = {"ktail_a0": "a0", "ktail_dvh": "dvh", "ktail_gan": "gan", "stale_col": "a0", "split_twice": "gan",
              "save_w_next": "logits", "mask_next": "logits", "dm_not_in_dot": "norm_bwd",
              "diag_before_store": "wa_bwd", "gan_acc_twice": "gan", "pn_wrong_side": "logits", "neg_eps1": "logits"}


def emulate_head(v, an, cot=None, faults=(), trimap=True, neg=True, attention=False, splits=1, gan0=None,
                 detached=False, eps=(EPS1, EPS2, TAU)):
    """The head's eleven launches in torch fp32 on the CPU, filling head_links' tape: v [B, P, C] bf16 (attention:
    fp32), an [B, C] fp32; cot: dlogits (default: the CE's own, mean over rows, target 0), dwA, gA, gPos, gNeg.
    faults (tests only; FAULTS):
      ktail_a0 / ktail_dvh / ktail_gan  the last k element of one row of the GEMM's A operand read as zero
      stale_col          the last column of A0's first 64 x 64 tile left at 0
      split_twice        the split-K sum counts split 1 twice
      save_w_next        save's W_ij taken from column j + 1
      mask_next          the forward's -99 on column i + 1
      dm_not_in_dot      dm / C added to dvh but not inside <vh, dvh>
      diag_before_store  the diagonal kernels run before hardway_logits_bwd_kernel's store (their updates are lost)
      gan_acc_twice      the accumulate epilogue adds the product twice
      pn_wrong_side      pn = 1 / min(||Pos||, 1e-12)
      neg_eps1           Neg from eps1 under trimap = 1"""
    assert all(f in FAULTS for f in faults), faults
    cot = dict(cot or {})
    f32 = torch.float32
    B, P, C = v.shape
    rows = B * P
    T = lambda c: torch.tensor(c, dtype=f32)  # noqa: E731
    e1, e2, it, c07, c12 = T(eps[0]), T(eps[1]), 1.0 / T(eps[2]), T(0.07), T(1e-12)
    x = v.float()
    xr = x.reshape(rows, C)
    an = an.float()
    tp = {"v": v, "an": an, "vsum": x.sum(-1)}
    tp["inv"] = torch.ones(B, P) if attention else 1.0 / (x * x).sum(-1).sqrt().clamp_min(c12)
    ivr = tp["inv"].reshape(rows, 1)
    xa = xr
    if "ktail_a0" in faults:
        xa = xr.clone()
        xa[rows - 1, C - 1] = 0
    A0 = ((xa @ an.T) * ivr)
    if "stale_col" in faults:
        A0[:min(64, rows), min(64, B) - 1] = 0
    A0 = tp["A0"] = A0.reshape(B, P, B)
    # hardway_logits_kernel
    eye = torch.eye(B, dtype=torch.bool)
    mask = torch.where(eye, -99.0, 1.0).to(f32)
    w = torch.sigmoid((A0 - e1) * it)
    sw, swx = w.sum(1), (w * A0).sum(1)
    s = swx / sw
    L = B + (2 if neg else 1)
    logits = torch.empty(B, L)
    fmask = torch.roll(mask, 1, dims=1) if "mask_next" in faults else mask
    logits[:, 1:1 + B] = s * fmask / c07
    A = _diag(A0).contiguous()
    Pos = torch.sigmoid((A - e1) * it)
    eneg = e2 if trimap and "neg_eps1" not in faults else e1
    Neg = torch.sigmoid(-(A - eneg) * it)
    W1, W2 = Pos.sum(1), Neg.sum(1)
    s1, s2 = (Pos * A).sum(1) / W1, (Neg * A).sum(1) / W2
    logits[:, 0] = s1 / c07
    if neg:
        logits[:, B + 1] = s2 / c07
    Wsave = torch.roll(sw, -1, dims=1) if "save_w_next" in faults else sw
    save = tp["save"] = torch.cat([s, Wsave, s1[:, None], W1[:, None], s2[:, None], W2[:, None]], 1).contiguous()
    nrm = (Pos * Pos).sum(1).sqrt()
    pn = 1.0 / (nrm.clamp_max(c12) if "pn_wrong_side" in faults else nrm.clamp_min(c12))
    tp.update(logits=logits, A=A, Pos=Pos, Neg=Neg, wA=tp["vsum"] * tp["inv"] / float(C) * Pos * pn[:, None])
    # hardway_ce_kernel (only when no dlogits is given)
    dl = cot.get("dlogits")
    if dl is None:
        lse = torch.logsumexp(logits, 1)
        tp["loss"] = (lse - logits[:, 0]).mean()
        dl = torch.exp(logits - lse[:, None])
        dl[:, 0] -= 1
        dl = dl / float(B)
    else:
        tp["loss"] = None
    tp["dl"] = dl = dl.float()
    # hardway_logits_bwd_kernel (reads the tape's save)
    wd = w * (1 - w) * it
    dsim = (dl[:, 1:1 + B] * mask / c07)[:, None, :]
    g = dsim * (w + wd * (A0 - save[:, None, :B])) / save[:, None, B:2 * B]
    wd1 = Pos * (1 - Pos) * it
    gd = _diag(g) + (dl[:, 0] / c07)[:, None] * (Pos + wd1 * (A - save[:, 2 * B, None])) / save[:, 2 * B + 1, None]
    if neg:
        wn = torch.sigmoid(-(A - (e2 if trimap else e1)) * it)
        wnd = -wn * (1 - wn) * it
        gd = gd + (dl[:, B + 1] / c07)[:, None] * (wn + wnd * (A - save[:, 2 * B + 2, None])) / \
            save[:, 2 * B + 3, None]
    _diag(g).copy_(gd)
    tp["dA0_pre"] = g.clone()
    lost = "diag_before_store" in faults
    # hardway_wa_bwd_kernel
    if cot.get("dwA") is not None:
        gw = tp["dwA"] = cot["dwA"].float()
        m = tp["vsum"] * tp["inv"] * (1.0 / T(float(C)))
        pp = (Pos * Pos).sum(1)
        dot = (Pos * gw * m).sum(1)
        nr = pp.sqrt()
        pn2 = 1.0 / nr.clamp_min(c12)
        proj = torch.where(nr > c12, dot * pn2 * pn2, torch.zeros_like(dot))
        dpos = (gw * m - Pos * proj[:, None]) * pn2[:, None]
        if not lost:
            _diag(g).add_(dpos * Pos * (1 - Pos) * it)
        tp["dm"] = gw * Pos * pn2[:, None]
        tp["dA0_wa"] = g.clone()
    # hardway_aux_bwd_kernel
    for k in ("gA", "gPos", "gNeg"):
        tp[k] = None if cot.get(k) is None else cot[k].float()
    if any(tp[k] is not None for k in ("gA", "gPos", "gNeg")):
        u = torch.zeros(B, P) if tp["gA"] is None else tp["gA"].clone()
        if tp["gPos"] is not None:
            u = u + tp["gPos"] * Pos * (1 - Pos) * it
        if tp["gNeg"] is not None:
            wn = torch.sigmoid(-(A - (e2 if trimap else e1)) * it)
            u = u - tp["gNeg"] * wn * (1 - wn) * it
        if not lost:
            _diag(g).add_(u)
    tp["dA0"] = g
    gr = g.reshape(rows, B)
    # the two GEMMs and the normalise backward
    if not detached:
        ga = gr
        if "ktail_dvh" in faults:
            ga = gr.clone()
            ga[rows - 1, B - 1] = 0
        tp["dvh"] = (ga @ an).reshape(B, P, C)
    gk = gr * ivr
    if "ktail_gan" in faults:
        gk = gk.clone()
        gk[rows - 1, B - 1] = 0
    kps = -(-rows // splits)
    kps = -(-kps // 32) * 32
    parts = [gk[k0:k0 + kps].T @ xr[k0:k0 + kps] for k0 in range(0, rows, kps)]
    assert len(parts) == splits, (len(parts), splits)
    if "split_twice" in faults:
        parts.insert(1, parts[min(1, len(parts) - 1)])
    tot = torch.zeros(B, C)
    for p in parts:
        tot = tot + p
    if gan0 is not None:
        tot = gan0.float() + tot + (tot if "gan_acc_twice" in faults else 0)
    elif "gan_acc_twice" in faults:
        tot = tot + tot
    tp["gan"] = tot
    if not detached:
        d = tp["dvh"]
        if attention:
            tp["gv"] = d.clone()
        else:
            dmc = tp["dm"][..., None] / float(C) if cot.get("dwA") is not None else 0.0
            e = d + dmc
            iv = tp["inv"][..., None]
            dot = (x * (d if "dm_not_in_dot" in faults else e)).sum(-1, keepdim=True) * iv
            tp["gv"] = (iv * (e - x * iv * dot)).to(torch.bfloat16)
    return tp


# ----------------------------------------------------------------------------------------------------------------
# the end-to-end reference and the older tests' reading
# ----------------------------------------------------------------------------------------------------------------

def oracle_e2e(v, an, cot=None, trimap=True, neg=True, attention=False, dtype=torch.float64,
               eps=(EPS1, EPS2, TAU)):
    """model.py:114-154 with the CE (or a given dlogits) and the cotangents as a scalar loss, by autograd in `dtype`:
    what tests/test_head_edges_gpu.py compares against.  Returns A, logits, Pos, Neg, wA, gan, gv."""
    cot = cot or {}
    B, P, C = v.shape
    vt = v.to(dtype).clone().requires_grad_(True)
    at = an.to(dtype).clone().requires_grad_(True)
    vh = vt if attention else F.normalize(vt, dim=2)
    A0 = torch.einsum("ipc,jc->ipj", vh, at)
    A = _diag(A0)
    Pos = torch.sigmoid((A - eps[0]) / eps[2])
    Neg = 1 - torch.sigmoid((A - (eps[1] if trimap else eps[0])) / eps[2])
    Pall = torch.sigmoid((A0 - eps[0]) / eps[2])
    sim1 = (Pos * A).sum(1) / Pos.sum(1)
    sim = (Pall * A0).sum(1) / Pall.sum(1) * (1 - 100 * torch.eye(B, dtype=dtype))
    sim2 = (Neg * A).sum(1) / Neg.sum(1)
    logits = torch.cat([sim1[:, None], sim] + ([sim2[:, None]] if neg else []), 1) / 0.07
    wA = vh.mean(2) * F.normalize(Pos, dim=1)
    if cot.get("dlogits") is not None:
        loss = (logits * cot["dlogits"].to(dtype)).sum()
    else:
        loss = F.cross_entropy(logits, torch.zeros(B, dtype=torch.long))
    for k, t in (("dwA", wA), ("gA", A), ("gPos", Pos), ("gNeg", Neg)):
        if cot.get(k) is not None:
            loss = loss + (t * cot[k].to(dtype)).sum()
    loss.backward()
    out = {"A": A, "logits": logits, "Pos": Pos, "Neg": Neg, "wA": wA}
    out = {k: t.detach() for k, t in out.items()}
    out.update(gan=at.grad, gv=vt.grad)
    return out


def old_reading(got, ref, gan0=None):
    """{output: (error as tests/test_head_edges_gpu._err measures it, OLD_TOL)} of a tape against oracle_e2e."""
    out = {}
    for n in ("A", "logits", "Pos", "Neg", "wA", "gan", "gv"):
        if got.get(n) is None:
            continue
        r = ref[n].double()
        if n == "gan" and gan0 is not None:
            r = r + gan0.double()
        d = (got[n].double().reshape(r.shape) - r).abs().max().item()
        if n in ("gan", "gv"):
            d /= max(ref[n].abs().max().item(), 1e-30)
        out[n] = (d if d == d else INF, OLD_TOL[n])
    return out
