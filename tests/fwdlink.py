"""The link oracle of the train-mode forward (CPU, fp64, torch + numpy only; nothing from the library).

A forward tape is a chain of launch groups.  Each function here takes ONE link's inputs from the tape (the GPU's own
bits, moved to the CPU: NHWC activations as fp64, the [4, C] statistics (scale, shift, mean, invstd) as fp32, idx /
carg / om as stored), recomputes that one link in fp64 and compares with the tape's next tensor.  Every link is one
bf16 (or a few fp32) roundings away from exact, so the bounds follow from the arithmetic and nothing is amplified:

  conv     |y - y64| <= 2^-8 |y64| + n 2^-24 A,  A = conv(|x|, |bf16(w)|), n = the reduction length rounded up to a
           power of two (one bf16 rounding -- half an ulp of an 8-bit significand is up to 2^-8 |y|, so links do
           come within 1 % of this term -- + the worst case of an fp32 sum in any order; split-K forms included)
  stats    against the fp64 batch statistics of the STORED bf16 c (the GPU's come from the unrounded fp32 values), with
           u = 2^-9 / (1 - 2^-9):  |mean - mean64| <= u E|c| + 2^-22 |mean64|,
           |var - var64| <= 4u E[c^2] + 2^-20 var64  (var = invstd^-2 - eps, biased) -- the worst case -- and the
           tightened forms below (STAT_Z): the deviation is a sum of R independent roundings, so it is measured in
           units of its standard scale  u sqrt(E[c^2] / R)  (mean)  and  2u sqrt(E[c^2 (c - mean)^2] / R)  (var), per
           channel and, for var, signed and averaged over the C channels times sqrt(C) ("bias": a systematic factor
           such as R / (R - 1) or a wrong eps moves every channel the same way)
  affine   scale = gamma * invstd, shift = beta - mean * scale from the GPU's own mean and invstd: 4 fp32 ulp of the
           larger operand
  running  running_mean / running_var after = (1 - m) before + m (mean | var R / (R - 1)), R = rows * rep, chained
           over the calls of a step in call order, relative 2^-18 of max(|before|, |after|) (of every update of
           the chain: the buffer between two calls counts); counters exact
  apply    v = bf16(relu(sum of the summands t_i)):  |v - v64| <= 2^-8 |v64| + 2^-20 sum |t_i|, v == 0 exactly where
           the fp64 pre-activation is below minus the second term; om bits, block chaining: exact
  pool     the stem's fused bn1 -> relu -> maxpool (value: as apply; carg, idx: exact), the audio pool (amax exact, an
           and anorm relative 1e-6, repeated rows bitwise)

Each function returns records (name, kind, worst error / bound, where); a record is out of bound when its ratio
exceeds 1 (exact checks give 0 or inf).  emulate_tape is the reference emulation (fp32 conv sums, statistics from the
unrounded values, every stored activation rounded to bf16, buffers updated): the yardstick of these bounds and the
carrier of the faults tests/test_forward_links_cpu.py injects.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
U = 2.0 ** -9 / (1.0 - 2.0 ** -9)
STAGES = [(64, 1), (128, 2), (256, 2), (512, 1)]
INF = float("inf")
TINY = 2.0 ** -133  # bf16's smallest subnormal: below it the rounding error is absolute, not relative

# The tightened statistics bounds, in the units above: 8 x the largest deviation emulate_tape itself shows against the
# same fp64 recomputation over every BN of the GPU tests' runs (tests/test_forward_links_cpu.py measures and asserts
# it; its docstring records the figures): "mean" and "var" per channel, "var_bias" the channel-averaged one.
STAT_Z = {"mean": 8 * 4.4, "var": 8 * 4.4, "var_bias": 8 * 3.2}


# ----------------------------------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------------------------------

def bf16(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 (round to nearest even) -> fp32."""
    return t.float().to(torch.bfloat16).float()


def pow2ceil(n: int) -> int:
    return 1 << max(0, (int(n) - 1).bit_length())


def worst(err: torch.Tensor, bound: torch.Tensor):
    """(max err / bound, its index); 0 / 0 counts as 0, anything over a zero bound or not finite as inf."""
    err, bound = torch.broadcast_tensors(err.double(), bound.double())
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, INF, 0.0).double())
    r = torch.where(torch.isfinite(err) & torch.isfinite(bound), r, torch.full_like(r, INF))
    if r.numel() == 0:
        return 0.0, ()
    i = int(r.argmax())
    return float(r.flatten()[i]), tuple(int(k) for k in np.unravel_index(i, tuple(r.shape)))


def exact(ok: torch.Tensor):
    """An exact check as a record's (ratio, where): 0 when every element of ok holds, else inf at the first failure."""
    ok = ok.reshape(-1) if ok.dim() == 0 else ok
    if bool(ok.all()):
        return 0.0, ()
    i = int((~ok).flatten().nonzero()[0])
    return INF, tuple(int(k) for k in np.unravel_index(i, tuple(ok.shape)))


def block_names(prefix: str):
    """[(block prefix, stride, has a downsample)] of a 2-D ResNet-18 trunk (layer4 stride 1)."""
    out, inplanes = [], 64
    for li, (planes, stride) in enumerate(STAGES, start=1):
        for bi in range(2):
            s = stride if bi == 0 else 1
            out.append((f"{prefix}layer{li}.{bi}.", s, bi == 0 and (s != 1 or inplanes != planes)))
        inplanes = planes
    return out


def bn_names(prefix: str) -> List[str]:
    out = [prefix + "bn1"]
    for p, _, down in block_names(prefix):
        out += [p + "bn1", p + "bn2"] + ([p + "downsample.1"] if down else [])
    return out


def stem_name(prefix: str, modal: str) -> str:
    return prefix + ("conv1_a.weight" if modal == "audio" else "conv1.weight")


def failures(records):
    return [r for r in records if not r[2] <= 1.0]


def worst_by_kind(records) -> Dict[str, tuple]:
    out: Dict[str, tuple] = {}
    for r in records:
        if r[1] not in out or not r[2] <= out[r[1]][2]:
            out[r[1]] = r
    return out


def report(tag: str, records) -> str:
    w = worst_by_kind(records)
    return f"{tag}: {len(records)} links; worst ratio per kind: " + ", ".join(
        f"{k} {w[k][2]:.3f} ({w[k][0]})" for k in sorted(w))


# ----------------------------------------------------------------------------------------------------------------
# links
# ----------------------------------------------------------------------------------------------------------------

def layout_link(name: str, x: torch.Tensor, x_tape: torch.Tensor):
    """The input layout conversion: x NCHW fp32 (a 5-D NCTHW input is folded '(b t)' first) against the tape's
    NHWC [N, H, W, cp]: bf16 RNE of the real channels, zero pad channels; exact."""
    if x.dim() == 5:
        b, c, t, h, w = x.shape
        x = x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)
    c = x.shape[1]
    want = bf16(x).permute(0, 2, 3, 1).double()
    ok_shape = tuple(x_tape.shape[:3]) == tuple(want.shape[:3]) and x_tape.shape[3] >= c
    if not ok_shape:
        return [(name, "layout", INF, ("shape",))]
    return [(name, "layout", *exact(x_tape[..., :c].double() == want)),
            (name + ".pad", "layout", *exact(x_tape[..., c:] == 0))]


def conv_link(name: str, x: torch.Tensor, w: torch.Tensor, y: torch.Tensor, stride: int, pad: int):
    """y = conv2d(x, bf16(w)): x [N, H, W, Cp] (channels past w's cin must be zero), w OIHW fp32 master weights,
    y [N, P, Q, K], all from the tape but w."""
    cin, k = w.shape[1], w.shape[2]
    wb = bf16(w).double()
    xn = x[..., :cin].double().permute(0, 3, 1, 2)
    y64 = F.conv2d(xn, wb, stride=stride, padding=pad).permute(0, 2, 3, 1)
    A = F.conv2d(xn.abs(), wb.abs(), stride=stride, padding=pad).permute(0, 2, 3, 1)
    if tuple(y64.shape) != tuple(y.shape):
        return [(name, "conv", INF, ("shape",))]
    n = pow2ceil(k * k * x.shape[-1])
    rec = [(name, "conv", *worst((y.double() - y64).abs(), 2.0 ** -8 * y64.abs() + n * 2.0 ** -24 * A))]
    if x.shape[-1] > cin:
        rec.append((name + ".xpad", "conv", *exact(x[..., cin:] == 0)))
    return rec


def conv3d_link(name: str, x: torch.Tensor, w: torch.Tensor, y: torch.Tensor, b: int, stride: int, pad_t: int,
                pad: int):
    """y = conv3d(x, bf16(w)), temporal stride 1: x [(b t), H, W, C], w OIDHW fp32, y [(b t), P, Q, K]."""
    kt, k = w.shape[2], w.shape[3]
    wb = bf16(w).double()
    bt, H, W, C = x.shape
    xn = x.double().reshape(b, bt // b, H, W, C).permute(0, 4, 1, 2, 3)
    kw = dict(stride=(1, stride, stride), padding=(pad_t, pad, pad))
    y64 = F.conv3d(xn, wb, **kw).permute(0, 2, 3, 4, 1)
    A = F.conv3d(xn.abs(), wb.abs(), **kw).permute(0, 2, 3, 4, 1)
    y64, A = y64.reshape(-1, *y64.shape[2:]), A.reshape(-1, *A.shape[2:])
    if tuple(y64.shape) != tuple(y.shape):
        return [(name, "conv", INF, ("shape",))]
    n = pow2ceil(kt * k * k * C)
    return [(name, "conv", *worst((y.double() - y64).abs(), 2.0 ** -8 * y64.abs() + n * 2.0 ** -24 * A))]


def stats_link(name: str, c: torch.Tensor, st: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
               eps: float = EPS):
    """Train mode: st[2] (mean) and st[3] (invstd) against the fp64 batch statistics of the stored c (worst-case and
    tightened bounds), then st[0] (scale) and st[1] (shift) from the tape's own mean and invstd."""
    C = c.shape[-1]
    x = c.double().reshape(-1, C)
    R = x.shape[0]
    mean64 = x.mean(0)
    d = x - mean64
    var64 = (d * d).mean(0)
    e_abs, e_sq = x.abs().mean(0), (x * x).mean(0)
    mean, inv = st[2].double(), st[3].double()
    var = inv ** -2 - eps
    dm, dv = mean - mean64, var - var64
    rec = [(name + ".mean", "stats", *worst(dm.abs(), U * e_abs + 2.0 ** -22 * mean64.abs())),
           (name + ".var", "stats", *worst(dv.abs(), 4 * U * e_sq + 2.0 ** -20 * var64))]
    s_mean = U * (e_sq / R).sqrt()
    s_var = 2 * U * ((x * x * d * d).mean(0) / R).sqrt() + 2.0 ** -20 * var64
    rec.append((name + ".mean_z", "stats", *worst(dm.abs(), STAT_Z["mean"] * s_mean + 2.0 ** -22 * mean64.abs())))
    rec.append((name + ".var_z", "stats", *worst(dv.abs(), STAT_Z["var"] * s_var)))
    bias = (dv / s_var).mean().abs() * math.sqrt(C)
    rec.append((name + ".var_bias", "stats", *worst(bias.reshape(1), torch.tensor([STAT_Z["var_bias"]]))))
    return rec + affine_link(name, st, gamma, beta)


def stat_deviations(c: torch.Tensor, st: torch.Tensor, eps: float = EPS):
    """The three tightened statistics of stats_link in their own units (what STAT_Z is 8 x the maximum of)."""
    C = c.shape[-1]
    x = c.double().reshape(-1, C)
    R = x.shape[0]
    mean64 = x.mean(0)
    d = x - mean64
    var64 = (d * d).mean(0)
    dm = st[2].double() - mean64
    dv = st[3].double() ** -2 - eps - var64
    s_var = 2 * U * ((x * x * d * d).mean(0) / R).sqrt() + 2.0 ** -20 * var64
    return {"mean": float((dm.abs() / (U * ((x * x).mean(0) / R).sqrt())).max()),
            "var": float((dv.abs() / s_var).max()),
            "var_bias": float((dv / s_var).mean().abs() * math.sqrt(C))}


def _ulp4(*ops):
    m = ops[0].double().abs()
    for o in ops[1:]:
        m = torch.maximum(m, o.double().abs())
    return 4 * 2.0 ** -23 * m


def affine_link(name: str, st: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor):
    sc, sh, mean, inv = (t.double() for t in st)
    g, b = gamma.double(), beta.double()
    return [(name + ".scale", "affine", *worst((sc - g * inv).abs(), _ulp4(g, inv))),
            (name + ".shift", "affine", *worst((sh - (b - mean * sc)).abs(), _ulp4(b, mean * sc)))]


def eval_stats_link(name: str, st: torch.Tensor, gamma, beta, rm, rv, eps: float = EPS):
    """Eval-mode tape: (gamma rsqrt(rv + eps), beta - rm scale, rm, rsqrt(rv + eps))."""
    inv64 = (rv.double() + eps).rsqrt()
    return [(name + ".mean", "stats", *exact(st[2] == rm.float())),
            (name + ".invstd", "stats", *worst((st[3].double() - inv64).abs(), _ulp4(inv64)))] + \
        affine_link(name, st, gamma, beta)


def running_link(name: str, before, after, calls, eps: float = EPS):
    """A BN's running statistics over the calls of a step: before / after = (running_mean, running_var) [C] fp32,
    calls = [(st, R, m)] in call order, st the call's tape statistics, R = rows * rep, m the momentum."""
    rm, rv = before[0].double(), before[1].double()
    a_m, a_v = after[0].double(), after[1].double()
    top_m, top_v = torch.maximum(rm.abs(), a_m.abs()), torch.maximum(rv.abs(), a_v.abs())
    for st, R, m in calls:
        mean, inv = st[2].double(), st[3].double()
        var = inv ** -2 - eps
        rm = (1 - m) * rm + m * mean
        rv = (1 - m) * rv + m * var * (R / (R - 1.0))
        # (a chained update's own before / after: the buffer between two calls of a step)
        top_m, top_v = torch.maximum(top_m, rm.abs()), torch.maximum(top_v, rv.abs())
    b_m, b_v = 2.0 ** -18 * top_m, 2.0 ** -18 * top_v
    return [(name + ".running_mean", "running", *worst((a_m - rm).abs(), b_m)),
            (name + ".running_var", "running", *worst((a_v - rv).abs(), b_v))]


def buffer_links(names, before: dict, after: dict, calls_of, inc: int):
    """running_link of every BN in names (calls_of(name) -> its calls; [] = eval mode: every buffer bitwise
    unchanged) and the counters: after - before == inc exactly."""
    rec = []
    for n in names:
        bf = (before[n + ".running_mean"], before[n + ".running_var"])
        af = (after[n + ".running_mean"], after[n + ".running_var"])
        calls = calls_of(n)
        if calls:
            rec += running_link(n, bf, af, calls)
        else:
            rec += [(n + ".running_mean", "running", *exact(bf[0] == af[0])),
                    (n + ".running_var", "running", *exact(bf[1] == af[1]))]
        k = n + ".num_batches_tracked"
        rec.append((k, "counter", *exact((after[k].long() - before[k].long()).reshape(1) == inc)))
    return rec


def apply_link(name: str, c, st, out, res=None, res_st=None):
    """out = bf16(relu(fma(c, scale, shift) [+ fma(res, rscale, rshift) | + res]))."""
    t1 = c.double() * st[0].double()
    pre, mag = t1 + st[1].double(), t1.abs() + st[1].double().abs()
    if res is not None:
        if tuple(res.shape) != tuple(c.shape):
            return [(name, "apply", INF, ("shape",))]
        if res_st is not None:
            r1 = res.double() * res_st[0].double()
            pre, mag = pre + r1 + res_st[1].double(), mag + r1.abs() + res_st[1].double().abs()
        else:
            pre, mag = pre + res.double(), mag + res.double().abs()
    v64 = pre.clamp_min(0)
    slack = 2.0 ** -20 * mag
    o = out.double()
    return [(name, "apply", *worst((o - v64).abs(), 2.0 ** -8 * v64 + slack + TINY)),
            (name + ".zero", "apply", *exact((o == 0) | ~(pre < -slack)))]


def mask_link(name: str, out, om):
    """om: bit e of byte j of a row <-> [out[row, 8 j + e] > 0], from the tape's own out."""
    C = out.shape[-1]
    bits = np.unpackbits(om.reshape(-1).numpy().astype(np.uint8), bitorder="little")
    if bits.size != out.numel():
        return [(name, "mask", INF, ("size",))]
    bits = torch.from_numpy(bits.astype(np.bool_)).reshape(-1, C)
    return [(name, "mask", *exact(bits == (out.reshape(-1, C) > 0)))]


def _windows(t: torch.Tensor, fill: float):
    """[9, N, H2, W2, C]: the 3 x 3 / stride 2 / pad 1 window taps of t [N, H, W, C], tap k = 3 r + s."""
    N, H, W, C = t.shape
    H2, W2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = torch.full((N, H + 2, W + 2, C), fill, dtype=t.dtype)
    p[:, 1:H + 1, 1:W + 1] = t
    return torch.stack([p[:, r:r + 2 * H2:2, s:s + 2 * W2:2] for r in range(3) for s in range(3)])


def stem_pool_link(name: str, c0, st0, p0, idx, carg):
    """The fused bn1 -> relu -> MaxPool2d(3, 2, 1): idx names a tap inside the image, carg == c0 there (exact), p0 is
    bf16(relu(fma(c0, scale, shift))) there (as apply), and no tap of the window is larger (each to its own apply
    bound): the position attains the window's maximum."""
    c = c0.double()
    t1 = c * st0[0].double()
    pre, mag = t1 + st0[1].double(), t1.abs() + st0[1].double().abs()
    w_pre, w_mag, w_c = _windows(pre, -INF), _windows(mag, 0.0), _windows(c, float("nan"))
    if tuple(w_pre.shape[1:]) != tuple(p0.shape) or int(idx.max()) > 8:
        return [(name, "pool", INF, ("shape",))]
    ix = idx.long().unsqueeze(0)
    a_pre, a_mag, a_c = (w.gather(0, ix)[0] for w in (w_pre, w_mag, w_c))
    valid = torch.isfinite(a_pre)
    a_pre = torch.where(valid, a_pre, torch.zeros_like(a_pre))
    v64 = a_pre.clamp_min(0)
    o = p0.double()
    over = (w_pre.clamp_min(0) - o).clamp_min(0)  # how far a tap's value lies above the stored maximum
    return [(name + ".idx", "pool", *exact(valid)),
            (name + ".carg", "pool", *exact(carg.double() == a_c)),
            (name, "pool", *worst((o - v64).abs(), 2.0 ** -8 * v64 + 2.0 ** -20 * a_mag + TINY)),
            (name + ".max", "pool", *worst(over, 2.0 ** -8 * w_pre.clamp_min(0) + 2.0 ** -20 * w_mag + TINY))]


def maxpool3d_link(name: str, h0, hp, b: int):
    """MaxPool3d(3, 2, 1) of h0 [(b t), H, W, C] -> hp [(b t'), H', W', C]: exact."""
    bt, H, W, C = h0.shape
    x = h0.double().reshape(b, bt // b, H, W, C).permute(0, 4, 1, 2, 3)
    y = F.max_pool3d(x, 3, 2, 1).permute(0, 2, 3, 4, 1)
    y = y.reshape(-1, *y.shape[2:])
    if tuple(y.shape) != tuple(hp.shape):
        return [(name, "pool", INF, ("shape",))]
    return [(name, "pool", *exact(hp.double() == y))]


def audio_pool_link(name: str, a, an_a, amax, anorm, an=None, rep: int = 1):
    """a [Ba, h, w, C] -> amax (each channel's maximum, exact), anorm, an_a = a[amax] / max(norm, 1e-12) (relative
    1e-6); an (the head's rows): row i rep + j a bitwise copy of an_a's row i."""
    Ba, h, w, C = a.shape
    flat = a.double().reshape(Ba, h * w, C)
    am = amax.long()
    rec = [(name + ".amax_range", "pool", *exact((am >= 0) & (am < h * w)))]
    if rec[0][2] > 1:
        return rec
    val = flat.gather(1, am.unsqueeze(1))[:, 0]
    rec.append((name + ".amax", "pool", *exact(val == flat.max(1).values)))
    norm = (val * val).sum(1).sqrt()
    an64 = val / norm.clamp_min(1e-12).unsqueeze(1)
    rec.append((name + ".anorm", "pool", *worst((anorm.double() - norm).abs(), 1e-6 * norm)))
    rec.append((name + ".an", "pool", *worst((an_a.double() - an64).abs(), 1e-6 * an64.abs())))
    if an is not None:
        want = an_a.repeat_interleave(rep, 0) if rep > 1 else an_a
        ok = tuple(want.shape) == tuple(an.shape)
        rec.append((name + ".repeat", "pool", *(exact(want == an) if ok else (INF, ("shape",)))))
    return rec


def trunk_links(sd, prefix: str, modal: str, tp: dict, x_in: Optional[torch.Tensor] = None, final=None):
    """Every link of one 2-D trunk tape in launch order.  sd: the master weights of the forward (and, for an eval
    tape, the running statistics it read); tp: the tape on the CPU (cpu_tape's form); x_in: the fp32 input of the
    layout kernel; final: the tensor the head read (tape["v"] / tape["a"]): the last block's out, same bits."""
    rec = []
    training = tp["training"]

    def stats(bn, c, st):
        g, b = sd[bn + ".weight"], sd[bn + ".bias"]
        if training:
            return stats_link(bn, c, st, g, b)
        return eval_stats_link(bn, st, g, b, sd[bn + ".running_mean"], sd[bn + ".running_var"])

    if x_in is not None:
        rec += layout_link(prefix + "input", x_in, tp["x"])
    rec += conv_link(stem_name(prefix, modal), tp["x"], sd[stem_name(prefix, modal)], tp["c0"], 2, 3)
    rec += stats(prefix + "bn1", tp["c0"], tp["st0"])
    rec += stem_pool_link(prefix + "maxpool", tp["c0"], tp["st0"], tp["blocks"][0]["x"], tp["idx"], tp["carg"])
    prev = None
    for (p, s, down), tb in zip(block_names(prefix), tp["blocks"]):
        if prev is not None:
            same = tuple(tb["x"].shape) == tuple(prev.shape) and torch.equal(tb["x"], prev)
            rec.append((p + "x", "chain", 0.0 if same else INF, ()))
        rec += conv_link(p + "conv1.weight", tb["x"], sd[p + "conv1.weight"], tb["c1"], s, 1)
        rec += stats(p + "bn1", tb["c1"], tb["s1"])
        rec += apply_link(p + "h1", tb["c1"], tb["s1"], tb["h1"])
        rec += conv_link(p + "conv2.weight", tb["h1"], sd[p + "conv2.weight"], tb["c2"], 1, 1)
        rec += stats(p + "bn2", tb["c2"], tb["s2"])
        if down:
            rec += conv_link(p + "downsample.0.weight", tb["x"], sd[p + "downsample.0.weight"], tb["cd"], s, 0)
            rec += stats(p + "downsample.1", tb["cd"], tb["sd"])
            rec += apply_link(p + "out", tb["c2"], tb["s2"], tb["out"], tb["cd"], tb["sd"])
        else:
            rec.append((p + "no_down", "chain", 0.0 if "cd" not in tb else INF, ()))
            rec += apply_link(p + "out", tb["c2"], tb["s2"], tb["out"], tb["x"])
        if tb.get("om") is not None:
            rec += mask_link(p + "om", tb["out"], tb["om"])
        prev = tb["out"]
    if final is not None:
        same = tuple(final.shape) == tuple(prev.shape) and torch.equal(final, prev)
        rec.append((prefix + "map", "chain", 0.0 if same else INF, ()))
    return rec


def trunk_calls(prefix: str, tp: dict, rep: int, m: float):
    """{BN name: (st, R, m)} of one train-mode trunk call, for running_link."""
    out = {prefix + "bn1": (tp["st0"], tp["c0"].numel() // tp["c0"].shape[-1] * rep, m)}
    for (p, _, down), tb in zip(block_names(prefix), tp["blocks"]):
        for bn, c, st in ((p + "bn1", "c1", "s1"), (p + "bn2", "c2", "s2")) + \
                ((((p + "downsample.1", "cd", "sd"),)) if down else ()):
            out[bn] = (tb[st], tb[c].numel() // tb[c].shape[-1] * rep, m)
    return out


def step_links(sd, names, before: dict, after: dict, calls, inc: int):
    """Every link of a step: calls = [(prefix, modal, tape, x_in, rep, m, final)] in call order (trunk_links of each,
    then the buffers of the BNs in names chained over their calls, the counters at +inc)."""
    rec, per_bn = [], {}
    for prefix, modal, tp, x_in, rep, m, final in calls:
        rec += trunk_links(sd, prefix, modal, tp, x_in, final)
        if tp["training"]:
            for bn, call in trunk_calls(prefix, tp, rep, m).items():
                per_bn.setdefault(bn, []).append(call)
    return rec + buffer_links(names, before, after, lambda n: per_bn.get(n, []), inc)


def cpu_tape(tp: dict) -> dict:
    """A Trunk tape (tensors on any device) in this module's form: activations fp64, statistics fp32, idx / om uint8,
    on the CPU."""
    def act(t):
        return t.detach().cpu().double()

    out = {"x": act(tp["x"]), "c0": act(tp["c0"]), "st0": tp["st0"].detach().cpu().float(),
           "idx": tp["idx"].detach().cpu(), "carg": act(tp["carg"]), "training": tp.get("training", True),
           "blocks": []}
    for tb in tp["blocks"]:
        b = {k: act(tb[k]) for k in ("x", "c1", "h1", "c2", "cd", "out") if k in tb}
        b.update({k: tb[k].detach().cpu().float() for k in ("s1", "s2", "sd") if k in tb})
        b["om"] = None if tb.get("om") is None else tb["om"].detach().cpu()
        out["blocks"].append(b)
    return out


def snapshot(sd: dict, names) -> dict:
    """Copies of the running statistics and counters of the BNs in names."""
    return {n + k: sd[n + k].detach().cpu().clone() for n in names
            for k in (".running_mean", ".running_var", ".num_batches_tracked")}


# ----------------------------------------------------------------------------------------------------------------
# the reference emulation
# ----------------------------------------------------------------------------------------------------------------

FAULTS = ("res_h1", "swap_down", "rv_biased", "invstd_unbiased", "stale_stats", "missing_tile", "om_prernd",
          "carg_first")


def _emu_bn(y32, sd, bn, momentum, rep, eps, fault, stale):
    """Statistics of the unrounded conv output y32 [N, P, Q, C] (fp64 sums) -> st [4, C] fp32; running statistics of
    sd updated in place in fp32."""
    C = y32.shape[-1]
    y = y32.double().reshape(-1, C)
    n = y.shape[0]
    if fault == "missing_tile":  # one 64-row tile's slot left out of the sums
        part = torch.cat([y[:64], y[128:]]) if n > 128 else y[: n // 2]
        mean = part.sum(0) / n
        m2 = ((part * part).sum(0) - n * mean * mean).clamp_min(0)
    else:
        mean = y.mean(0)
        m2 = ((y - mean) ** 2).sum(0)
    if fault == "stale_stats":  # the statistics of another call's batch
        mean, m2 = stale[2].double(), (stale[3].double() ** -2 - eps) * n
    var = (m2 / (n - 1 if fault == "invstd_unbiased" else n)).float()
    inv = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    sc = sd[bn + ".weight"].float() * inv
    sh = sd[bn + ".bias"].float() - mean.float() * sc
    nl = float(n * rep)
    unb = var if fault == "rv_biased" else (m2 * rep / (nl - 1)).float()
    m = torch.tensor(momentum, dtype=torch.float32)
    sd[bn + ".running_mean"].copy_((1 - m) * sd[bn + ".running_mean"].float() + m * mean.float())
    sd[bn + ".running_var"].copy_((1 - m) * sd[bn + ".running_var"].float() + m * unb)
    return torch.stack([sc, sh, mean.float(), inv])


def _emu_conv(x, w, stride, pad):
    """fp32 sums of bf16 operands: x [N, H, W, C] (bf16 values), w OIHW master weights -> [N, P, Q, K] fp32."""
    y = F.conv2d(x[..., :w.shape[1]].float().permute(0, 3, 1, 2), bf16(w), stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).contiguous()


def _fma(c, st_sc, st_sh):
    return (c.double() * st_sc.double() + st_sh.double()).float()  # one rounding, as a fused multiply-add


def emulate_tape(sd, x, modal: str, momentum: float = 0.1, rep: int = 1, prefix: Optional[str] = None,
                 calls: int = 1, eps: float = EPS, fault=None, fault_at: Optional[str] = None, stale=None):
    """One train-mode forward of a 2-D trunk as the library composes it, emulated on the CPU: x NCHW fp32 -> NHWC bf16
    (zero pad channel for vision), fp32 conv sums of bf16 operands, BN statistics from the unrounded fp32 conv output
    (fp64 sums), scale / shift / running statistics in fp32 (momentum, the unbiased factor of rows * rep), every
    stored activation rounded to bf16, idx / carg / om as the kernels define them.  Updates sd's running statistics
    in place and adds `calls` to its counters.  Returns the tape in cpu_tape's form.
    fault (tests only; FAULTS) with fault_at = the BN or block it acts on (default: everywhere it applies); stale:
    the [4, C] statistics "stale_stats" puts in place of fault_at's."""
    assert fault is None or fault in FAULTS, fault
    if prefix is None:
        prefix = "audnet." if modal == "audio" else "imgnet."
    cp = 1 if modal == "audio" else 4
    N, cin, H, W = x.shape
    xb = torch.zeros(N, H, W, cp)
    xb[..., :cin] = bf16(x).permute(0, 2, 3, 1)

    def bn(y32, name):
        f = fault if fault in ("rv_biased", "invstd_unbiased", "stale_stats", "missing_tile") and \
            (fault_at is None or fault_at == name) else None
        st = _emu_bn(y32, sd, name, momentum, rep, eps, f, stale)
        sd[name + ".num_batches_tracked"].add_(calls)
        return st

    y0 = _emu_conv(xb, sd[stem_name(prefix, modal)], 2, 3)
    c0 = bf16(y0)
    st0 = bn(y0, prefix + "bn1")
    pre0 = _fma(c0, st0[0], st0[1])
    h0 = bf16(pre0.clamp_min(0))
    taps = _windows(h0, -INF)
    idx = taps.argmax(0)  # (the first of equal maxima)
    taps_c = _windows(c0, 0.0)
    pick = idx
    if fault == "carg_first":  # carg from the window's first tap inside the image
        pick = torch.isfinite(taps).float().argmax(0)
    tape = {"x": xb.double(), "c0": c0.double(), "st0": st0, "idx": idx.to(torch.uint8),
            "carg": taps_c.gather(0, pick.unsqueeze(0))[0].double(), "training": True, "blocks": []}
    cur = taps.gather(0, idx.unsqueeze(0))[0]
    for p, s, down in block_names(prefix):
        here = fault_at is None or fault_at == p
        y1 = _emu_conv(cur, sd[p + "conv1.weight"], s, 1)
        c1, s1 = bf16(y1), bn(y1, p + "bn1")
        h1 = bf16(_fma(c1, s1[0], s1[1]).clamp_min(0))
        y2 = _emu_conv(h1, sd[p + "conv2.weight"], 1, 1)
        c2, s2 = bf16(y2), bn(y2, p + "bn2")
        tb = {"x": cur.double(), "c1": c1.double(), "s1": s1, "h1": h1.double(), "c2": c2.double(), "s2": s2}
        if down:
            yd = _emu_conv(cur, sd[p + "downsample.0.weight"], s, 0)
            cd, sdn = bf16(yd), bn(yd, p + "downsample.1")
            a2, ad = (sdn, s2) if fault == "swap_down" and here else (s2, sdn)
            pre = _fma(c2, a2[0], a2[1]) + _fma(cd, ad[0], ad[1])
            tb.update(cd=cd.double(), sd=sdn)
        else:
            res = h1 if fault == "res_h1" and here else cur
            pre = _fma(c2, s2[0], s2[1]) + res
        out = bf16(pre.clamp_min(0))
        bits = (pre > 0) if fault == "om_prernd" and here else (out > 0)
        om = np.packbits(bits.reshape(-1).numpy(), bitorder="little")
        tb.update(out=out.double(), om=torch.from_numpy(om))
        tape["blocks"].append(tb)
        cur = out
    return tape


def emulate_audio_pool(a: torch.Tensor, rep: int = 1):
    """(an_a, amax, anorm, an) of the audio pool + normalise + row repeat, in fp32, from a [Ba, h, w, C]."""
    Ba, h, w, C = a.shape
    flat = a.float().reshape(Ba, h * w, C)
    val, amax = flat.max(1)
    norm = (val * val).sum(1).sqrt()
    an_a = val / norm.clamp_min(1e-12).unsqueeze(1)
    return an_a, amax.to(torch.int32), norm, an_a.repeat_interleave(rep, 0)


# ----------------------------------------------------------------------------------------------------------------
# the R3D-18 video trunk
# ----------------------------------------------------------------------------------------------------------------

R3D_STAGES = [(64, 1), (128, 2), (256, 2), (512, 2)]  # (planes, spatial stride); temporal stride 1


def r3d_block_names(prefix: str):
    out, inplanes = [], 64
    for li, (planes, stride) in enumerate(R3D_STAGES, start=1):
        for bi in range(2):
            s = stride if bi == 0 else 1
            out.append((f"{prefix}layer{li}.{bi}.", s, bi == 0 and (s != 1 or inplanes != planes)))
        inplanes = planes
    return out


def r3d_bn_names(prefix: str) -> List[str]:
    out = [prefix + "bn1"]
    for p, _, down in r3d_block_names(prefix):
        out += [p + "bn1", p + "bn2"] + ([p + "downsample.1"] if down else [])
    return out


def im2col_link(name: str, video: torch.Tensor, x_tape: torch.Tensor, kt: int = 7, pad_t: int = 3):
    """The stem's temporal fold: X[n, t, h, w, 4 k + c] = bf16(video[n, c, t + k - pad_t, h, w]) (0 outside the clip,
    c = 3 and channels 4 kt .. 31 zero); exact."""
    b, C, T, H, W = video.shape
    v = bf16(video).permute(0, 2, 3, 4, 1)  # [b, T, H, W, C]
    want = torch.zeros(b, T, H, W, 32)
    for k in range(kt):
        lo, hi = max(0, pad_t - k), min(T, T + pad_t - k)  # output frames t with 0 <= t + k - pad_t < T
        want[:, lo:hi, :, :, 4 * k:4 * k + C] = v[:, lo + k - pad_t:hi + k - pad_t]
    if tuple(want.shape) != tuple(x_tape.shape):
        return [(name, "layout", INF, ("shape",))]
    return [(name, "layout", *exact(x_tape.double() == want.double()))]


def cpu_tape3d(tp: dict) -> dict:
    """An R3DTrunk tape in this module's form (activations '(b t) h w c' fp64, statistics fp32, on the CPU)."""
    def act(t):
        return t.detach().cpu().double()

    out = {"b": tp["b"], "x": act(tp["x"]), "c0": act(tp["c0"]), "s0": tp["s0"].detach().cpu().float(),
           "h0": act(tp["h0"]), "blocks": []}
    for tb in tp["blocks"]:
        b = {k: act(tb[k]) for k in ("x", "c1", "h1", "c2", "cd", "out") if k in tb}
        b.update({k: tb[k].detach().cpu().float() for k in ("s1", "s2", "sd") if k in tb})
        out["blocks"].append(b)
    return out


def r3d_links(sd, prefix: str, tp: dict, video: torch.Tensor, max_pool: bool, final=None):
    """Every link of a train-mode R3DTrunk tape in launch order: the temporal fold, the 7 x 7 x 7 stem as a Conv3d on
    the bf16-rounded video, bn1 + ReLU, the max-pool (exact), per block conv1 / bn1 / h1 / conv2 / bn2 / the per-frame
    1 x 1 x 1 downsample / out, the chaining."""
    b = tp["b"]
    rec = im2col_link(prefix + "im2col", video, tp["x"])

    def stats(bn, c, st):
        return stats_link(bn, c, st, sd[bn + ".weight"], sd[bn + ".bias"])

    bsz, C, T, H, W = video.shape
    xv = bf16(video).permute(0, 2, 3, 4, 1).reshape(bsz * T, H, W, C).double()
    rec += conv3d_link(prefix + "conv1.weight", xv, sd[prefix + "conv1.weight"], tp["c0"], b, 2, 3, 3)
    rec += stats(prefix + "bn1", tp["c0"], tp["s0"])
    rec += apply_link(prefix + "h0", tp["c0"], tp["s0"], tp["h0"])
    prev = tp["h0"]
    if max_pool:
        rec += maxpool3d_link(prefix + "maxpool", tp["h0"], tp["blocks"][0]["x"], b)
        prev = None
    for (p, s, down), tb in zip(r3d_block_names(prefix), tp["blocks"]):
        if prev is not None:
            same = tuple(tb["x"].shape) == tuple(prev.shape) and torch.equal(tb["x"], prev)
            rec.append((p + "x", "chain", 0.0 if same else INF, ()))
        rec += conv3d_link(p + "conv1.weight", tb["x"], sd[p + "conv1.weight"], tb["c1"], b, s, 1, 1)
        rec += stats(p + "bn1", tb["c1"], tb["s1"])
        rec += apply_link(p + "h1", tb["c1"], tb["s1"], tb["h1"])
        rec += conv3d_link(p + "conv2.weight", tb["h1"], sd[p + "conv2.weight"], tb["c2"], b, 1, 1, 1)
        rec += stats(p + "bn2", tb["c2"], tb["s2"])
        if down:
            w = sd[p + "downsample.0.weight"]
            rec += conv_link(p + "downsample.0.weight", tb["x"], w.reshape(w.shape[0], w.shape[1], 1, 1), tb["cd"],
                             s, 0)
            rec += stats(p + "downsample.1", tb["cd"], tb["sd"])
            rec += apply_link(p + "out", tb["c2"], tb["s2"], tb["out"], tb["cd"], tb["sd"])
        else:
            rec.append((p + "no_down", "chain", 0.0 if "cd" not in tb else INF, ()))
            rec += apply_link(p + "out", tb["c2"], tb["s2"], tb["out"], tb["x"])
        prev = tb["out"]
    if final is not None:
        same = tuple(final.shape) == tuple(prev.shape) and torch.equal(final, prev)
        rec.append((prefix + "map", "chain", 0.0 if same else INF, ()))
    return rec


def r3d_calls(prefix: str, tp: dict, m: float = 0.1):
    """{BN name: (st, R, m)} of one train-mode R3DTrunk call."""
    out = {prefix + "bn1": (tp["s0"], tp["c0"].numel() // 64, m)}
    for (p, _, down), tb in zip(r3d_block_names(prefix), tp["blocks"]):
        for bn, c, st in ((p + "bn1", "c1", "s1"), (p + "bn2", "c2", "s2")) + \
                ((((p + "downsample.1", "cd", "sd"),)) if down else ()):
            out[bn] = (tb[st], tb[c].numel() // tb[c].shape[-1], m)
    return out
