"""The classifier head of the stand-alone R3D-18 (csrc/cls.hip) restated in torch, and the checks its outputs are held
to -- shared by test_cls_kernels_gpu.py (the device's outputs) and test_cls_cpu.py (the restatement, clean and with
injected faults, through the same checks).

Five links: pool_fwd, fc_fwd, ce, fc_bwd, pool_bwd.  The pool and the fc links are compared EXACTLY on operands whose
sums are exact in fp32 in any order; the CE link is bounded per element by DESIGN 4b's rule: the roundings counted in
the source (u = 2^-24 each, on the magnitude they act on) plus 3 Y, Y being the error of torch's fp32 log_softmax /
softmax on the CPU against fp64 on the case's own logits.

include/avt.h states that the pool DIVIDES by (float)per (IEEE fp32 division, no reciprocal): ``pool_quotient`` is that
statement, used for both directions."""
import math
import os
import re

import torch
import torch.nn.functional as F

U = 2.0 ** -24
POOL_ROWS = 64  # rows of one partial slot (avt_cls_pool_ws_bytes = b * ceil(per / 64) * C * 4)


def header_pool_rule() -> str:
    """'divide' or 'reciprocal', read from include/avt.h's statement on avt_cls_pool_fwd."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "avt.h")
    with open(path) as f:
        text = f.read()
    m = re.search(r"avt_cls_pool_fwd:(.*?)\*/", text, re.S)
    assert m, "include/avt.h has no avt_cls_pool_fwd comment"
    body = m.group(1)
    div, rec = "DIVIDE BY per" in body, "MULTIPLY BY THE RECIPROCAL" in body
    assert div != rec, "include/avt.h must state exactly one of the two pool rules"
    return "divide" if div else "reciprocal"


def pool_quotient(s32: torch.Tensor, per: int) -> torch.Tensor:
    """fp32 s / per by the header's rule."""
    assert s32.dtype == torch.float32 and per < 2 ** 24
    if header_pool_rule() == "divide":
        return s32 / torch.tensor(float(per), dtype=torch.float32)
    return s32 * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(per), dtype=torch.float32))


def pool_slots(per: int) -> int:
    return -(-per // POOL_ROWS)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement (any float dtype; faults by name)
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("pool_last_row", "pool_slot_twice", "fc_ktail_zero", "ce_denominator", "gbias_row", "pool_bwd_hw")


def restate_pool_fwd(v, fault=None):
    """v [b][per][C] -> sum over per in slots of POOL_ROWS rows, slots added in order, / per."""
    b, per, C = v.shape
    rows = per - 1 if fault == "pool_last_row" else per
    s = torch.zeros(b, C, dtype=v.dtype)
    for k in range(pool_slots(per)):
        part = v[:, k * POOL_ROWS:min((k + 1) * POOL_ROWS, rows)].sum(1)
        s = s + part
        if fault == "pool_slot_twice" and k == pool_slots(per) - 1:
            s = s + part
    return s / per


def restate_fc_fwd(feat, W, bias, fault=None):
    if fault == "fc_ktail_zero":  # the columns past the last multiple of 64 (a wave's strided tail) read as zero
        C = feat.shape[1]
        feat = feat.clone()
        feat[:, C // 64 * 64 if C % 64 else C - 1:] = 0
    return bias + feat @ W.t()


def restate_ce(z, labels, scale, fault=None):
    """-> (loss [1], dlogits, correct, valid rows)"""
    b, n = z.shape
    valid = (labels >= 0) & (labels < n)
    nv = int(valid.sum())
    den = b if fault == "ce_denominator" else nv
    y = labels.clamp(0, n - 1)
    lse = torch.logsumexp(z, 1)
    row = (lse - z.gather(1, y[:, None])[:, 0]) * valid
    onehot = F.one_hot(y, n).to(z.dtype)
    dl = torch.where(valid[:, None], torch.softmax(z, 1) - onehot, torch.zeros_like(z))  # ignored rows: +0
    if nv == 0:
        return torch.zeros(1, dtype=z.dtype), torch.zeros_like(z), 0, 0
    return (scale * row.sum() / den).reshape(1), scale * dl / den, int((first_argmax(z) == labels).sum()), nv


def restate_fc_bwd(dl, feat, W, fault=None):
    gW = dl.t() @ feat
    gbias = (dl[:-1] if fault == "gbias_row" else dl).sum(0)
    return gW, gbias, dl @ W


def restate_pool_bwd(gfeat, t, hw, fault=None):
    per = t * hw
    g = gfeat / (hw if fault == "pool_bwd_hw" else per)
    return g[:, None, :].expand(gfeat.shape[0], per, gfeat.shape[1])


def first_argmax(z):
    n = z.shape[1]
    idx = torch.arange(n)[None, :].expand_as(z)
    return torch.where(z == z.max(1, keepdim=True).values, idx, torch.full_like(idx, n)).min(1).values


# ---------------------------------------------------------------------------------------------------------------------
# the checks (device or restated outputs in fp32 / bf16 on the CPU); each returns a list of complaints
# ---------------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def check_pool_fwd(feat32, v_int):
    """v_int [b][per][C] integers with sum |v| < 2^24 (asserted): feat == fp32(S) (/ | * 1/) per bit for bit."""
    b, per, C = v_int.shape
    assert int(v_int.abs().sum(1).max()) < 2 ** 24, "test condition: partial sums exact in fp32"
    want = pool_quotient(v_int.sum(1).to(torch.float32), per)
    bad = bits(feat32.cpu()) != bits(want)
    return [f"pool_fwd: {int(bad.sum())} of {bad.numel()} elements differ from fp32(S) by the header's rule"] if \
        bool(bad.any()) else []


def check_pool_bwd(g_bf16, gfeat32, per):
    """g [b][per][C] bf16 == bf16_rne(gfeat by the header's rule) at every position."""
    want = pool_quotient(gfeat32.cpu(), per).to(torch.bfloat16)[:, None, :].expand(gfeat32.shape[0], per, -1)
    bad = bits(g_bf16.cpu()) != bits(want.contiguous())
    return [f"pool_bwd: {int(bad.sum())} of {bad.numel()} positions differ"] if bool(bad.any()) else []


def check_fc_fwd_exact(logits32, feat, W, bias):
    f, w, bi = feat.double().cpu(), W.double().cpu(), bias.double().cpu()
    assert float((f.abs() @ w.abs().t()).max()) <= 1.0, "test condition: sum |products| <= 1"
    want = bi + f @ w.t()
    assert torch.equal(want.float().double(), want), "test condition: the fp64 result is an fp32 number"
    bad = logits32.cpu().double() != want
    return [f"fc_fwd: {int(bad.sum())} of {bad.numel()} logits differ from the fp64 product"] if bool(bad.any()) else []


def check_fc_bwd_exact(gW, gbias, gfeat, dl, feat, W):
    d, f, w = dl.double().cpu(), feat.double().cpu(), W.double().cpu()
    assert float((d.abs().t() @ f.abs()).max()) <= 1.0 and float((d.abs() @ w.abs()).max()) <= 1.0, \
        "test condition: sum |products| <= 1"
    out = []
    for name, got, want in (("gW", gW, d.t() @ f), ("gbias", gbias, d.sum(0)), ("gfeat", gfeat, d @ w)):
        bad = got.cpu().double() != want
        if bool(bad.any()):
            out.append(f"fc_bwd {name}: {int(bad.sum())} of {bad.numel()} elements differ from the fp64 product")
    return out


def gemm_bound(a_abs, b_abs, K):
    """headlink.py's GEMM bound: (K + 2) u sum |a b| per element."""
    return (K + 2) * U * (a_abs @ b_abs)


def check_fc_random(logits32, gW, gbias, gfeat, dl, feat, W, bias):
    """random fp32 draws: every element within (K + 2) 2^-24 sum |a b| of fp64, K the reduction length (the forward's
    bias counts among the terms: sum |a b| + |bias|, the same factor)."""
    d, f, w, bi = dl.double().cpu(), feat.double().cpu(), W.double().cpu(), bias.double().cpu()
    b, C = f.shape
    n = w.shape[0]
    recs = [("fc_fwd", logits32, bi + f @ w.t(), (C + 2) * U * (f.abs() @ w.abs().t() + bi.abs())),
            ("gW", gW, d.t() @ f, gemm_bound(d.abs().t(), f.abs(), b)),
            ("gbias", gbias, d.sum(0), (b + 2) * U * d.abs().sum(0)),
            ("gfeat", gfeat, d @ w, gemm_bound(d.abs(), w.abs(), n))]
    out, worst = [], {}
    for name, got, want, bound in recs:
        err = (got.cpu().double() - want).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        worst[name] = ratio
        if bool((err > bound).any()):
            out.append(f"{name}: worst error / bound = {ratio:.3f}")
    return out, worst


def ce_reference(z32, labels, scale, B=None):
    """fp64 reference of avt_softmax_ce on the fp32 logits and the per-element bounds (module docstring).  Returns a
    dict: loss, dl, correct, nvalid, loss_bound, dl_bound, Y_loss, Y_dl (the yardstick parts, in the outputs' units)."""
    z32, labels = z32.cpu(), labels.cpu()
    b, n = z32.shape
    z = z32.double()
    loss, dl, correct, nv = restate_ce(z, labels, float(scale))
    valid = (labels >= 0) & (labels < n)
    if nv == 0:
        zero = torch.zeros_like(z)
        return dict(loss=0.0, dl=zero, correct=0, nvalid=0, loss_bound=0.0, dl_bound=zero, Y_loss=0.0, Y_dl=0.0)
    y = labels.clamp(0, n - 1)
    mx = z.max(1).values
    lse = torch.logsumexp(z, 1)
    zy = z.gather(1, y[:, None])[:, 0]
    row = (lse - zy) * valid
    sm = torch.softmax(z, 1)
    # the yardstick: torch's fp32 log_softmax / softmax on the CPU against fp64, in the outputs' own units
    ls32 = F.log_softmax(z32, 1).double()
    y_rows = ((-ls32.gather(1, y[:, None])[:, 0]) - (lse - zy)).abs() * valid
    Y_loss = float(abs(scale) * y_rows.sum() / nv)
    Y_dl = float(abs(scale) / nv * ((F.softmax(z32, 1).double() - sm).abs() * valid[:, None]).max())
    # roundings in the source, per row: the lane sums of exp (ceil(n/64) - 1 + 6 butterfly additions), the subtraction
    # in the exponent, mx + log(se), lse - z[y]; each on a magnitude of at most unit_row
    r_sum = math.ceil(n / 64) - 1 + 6
    unit_row = U * torch.maximum(torch.maximum(mx.abs() + (lse - mx).abs(), zy.abs()),
                                 torch.full_like(mx, max(1.0, 2 * math.log(n))))
    r_row = r_sum + 3
    # the rows: ceil(b / 16) additions per wave, 16 across the waves, then * scale and / valid rows
    r_rows = math.ceil(b / 16) + 16 + 2
    loss_bound = abs(scale) / nv * float((r_row * unit_row * valid).sum() + r_rows * U * row.abs().sum()) + 3 * Y_loss
    # dlogits: softmax = exp(z - lse); an error e in the exponent moves it by softmax * e: e = lse's roundings
    # ((r_row - 1) unit_row) + the subtraction's (u |z - lse|, and |x| exp(-|x|) <= 0.37); then - onehot, * scale, / rows
    dl_abs = (sm - F.one_hot(y, n).double()).abs()
    dl_bound = abs(scale) / nv * (sm * ((r_row - 1) * unit_row)[:, None] + 0.37 * U + 3 * U * dl_abs) + 3 * Y_dl
    dl_bound = dl_bound * valid[:, None]  # ignored rows: exactly +0
    return dict(loss=float(loss), dl=dl, correct=correct, nvalid=nv, loss_bound=loss_bound, dl_bound=dl_bound,
                Y_loss=Y_loss, Y_dl=Y_dl)


def check_ce(loss32, dl32, correct, z32, labels, scale):
    """-> (complaints, {"loss": worst ratio to the bound, "dlogits": ...})"""
    ref = ce_reference(z32, labels, scale)
    n = z32.shape[1]
    out = []
    lerr = abs(float(loss32.double()) - ref["loss"])
    dl = dl32.cpu()
    derr = (dl.double() - ref["dl"]).abs()
    ratios = {"loss": lerr / ref["loss_bound"] if ref["loss_bound"] > 0 else (0.0 if lerr == 0 else math.inf),
              "dlogits": float(torch.where(ref["dl_bound"] > 0, derr / ref["dl_bound"].clamp_min(1e-300),
                                           torch.where(derr == 0, torch.zeros_like(derr),
                                                       torch.full_like(derr, math.inf))).max())}
    if not lerr <= ref["loss_bound"]:
        out.append(f"ce loss: error {lerr:.3e} > bound {ref['loss_bound']:.3e}")
    if not bool((derr <= ref["dl_bound"]).all()):
        out.append(f"ce dlogits: worst error / bound = {ratios['dlogits']:.3f}")
    ignored = ~((labels.cpu() >= 0) & (labels.cpu() < n))
    if ref["nvalid"] == 0:
        ignored = torch.ones_like(ignored)
    if bool((bits(dl)[ignored] != 0).any()):
        out.append("ce dlogits: an ignored row is not exactly +0")
    if ref["nvalid"] == 0 and bits(loss32.cpu().reshape(1).float())[0] != 0:
        out.append("ce loss: not +0 with no valid row")
    if correct is not None and int(correct) != ref["correct"]:
        out.append(f"ce correct: {int(correct)} != {ref['correct']}")
    return out, ratios, ref


# ---------------------------------------------------------------------------------------------------------------------
# torch.optim.SGD's rule (the issue's statement of it) in a given dtype, for the exactness condition of the SGD test
# ---------------------------------------------------------------------------------------------------------------------
def sgd_rule(p, grads, lr, momentum, dampening, wd, nesterov, grad_scale, dtype):
    """p, grads (a list, one per step) -> (p, buf or None) after len(grads) steps, all arithmetic in ``dtype``."""
    p = p.to(dtype).clone()
    buf = None
    c = lambda x: torch.tensor(x, dtype=dtype)  # noqa: E731
    for k, gr in enumerate(grads):
        g = gr.to(dtype) * c(grad_scale) + c(wd) * p
        if momentum != 0:
            buf = g.clone() if k == 0 else c(momentum) * buf + (c(1.0) - c(dampening)) * g
            g = g + c(momentum) * buf if nesterov else buf
        p = p - c(lr) * g
    return p, buf
