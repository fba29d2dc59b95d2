"""numpy restatement of the flow-compensated consistency entries (csrc/flow.hip) -- TEST INFRASTRUCTURE ONLY.

* ``bilinear_at`` / ``warp`` / ``consistency``: numpy float32, one rounding per operation, the terms added nw, ne, sw,
  se from the first neighbour inside the map -- what include/avt.h states, and what torch's
  ``grid_sample(mode='bilinear', padding_mode='zeros', align_corners=False)`` computes up to its own contraction.
* ``flow_loss_ordered``: the loss and its gradient in the kernel's stated order of operations (bitwise on exactly
  summable inputs); ``flow_loss_f64``: the same mathematics in fp64 from the fp32 sampling positions, with the rounding
  bounds a float32 evaluation has to meet.
* ``color_wheel`` / ``compute_color`` / ``flow2img``: utils.py:64-192 expression by expression in fp64, and
  ``flow2img_report``: which pixels a differently rounded ``atan2`` / ``sqrt`` may change, and to what.
* ``read_flo`` / ``write_flo``: the Middlebury format.

The keyword arguments named ``fault_*`` switch in one wrong reading each (swapped components, ``>`` for ``>=`` ...);
tests/test_flow_cpu.py shows that the inputs the GPU tests use tell every one of them from the right reading.
"""
import numpy as np

F = np.float32
EPS32 = 2.0 ** -24      # unit roundoff of float32
EPS64 = 2.0 ** -52      # np.finfo(float).eps, as flow2img adds it


# ---------------------------------------------------------------- sampling
def positions(field, H, W, coords, fault_swap_uv=False, fault_align_corners=False):
    """Sampling positions (ix, iy), float32 [..., Ho, Wo], of a field [..., Ho, Wo, 2] over a map [H][W]."""
    f = np.asarray(field, dtype=F)
    f0, f1 = (f[..., 1], f[..., 0]) if fault_swap_uv else (f[..., 0], f[..., 1])
    with np.errstate(over="ignore", invalid="ignore"):
        if coords == "grid":
            if fault_align_corners:
                return (f0 + F(1)) / F(2) * F(W - 1), (f1 + F(1)) / F(2) * F(H - 1)
            return ((f0 + F(1)) * F(W) - F(1)) / F(2), ((f1 + F(1)) * F(H) - F(1)) / F(2)
        assert coords == "pixels", coords
        Ho, Wo = f.shape[-3], f.shape[-2]
        return np.arange(Wo, dtype=F) + f0, np.arange(Ho, dtype=F)[:, None] + f1


def taps(ix, iy, H, W, fault_no_padding=False, dtype=F):
    """cells [4, ...] (flat index y * W + x, -1 outside the map or for a non-finite position) and weights [4, ...] in
    the order nw, ne, sw, se.  ``dtype`` float64 evaluates the weights in fp64 from the same float32 positions."""
    finite = np.isfinite(ix) & np.isfinite(iy)
    ix = np.where(finite, ix, F(0)).astype(dtype)
    iy = np.where(finite, iy, F(0)).astype(dtype)
    fx0, fy0 = np.floor(ix), np.floor(iy)
    wx1, wy1 = ix - fx0, iy - fy0
    wx0, wy0 = (fx0 + dtype(1)) - ix, (fy0 + dtype(1)) - iy
    x0 = np.clip(fx0, -2, W + 1).astype(np.int64)
    y0 = np.clip(fy0, -2, H + 1).astype(np.int64)
    cells, weights = [], []
    for dy, dx, wgt in ((0, 0, wx0 * wy0), (0, 1, wx1 * wy0), (1, 0, wx0 * wy1), (1, 1, wx1 * wy1)):
        x, y = x0 + dx, y0 + dy
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H) & finite
        if fault_no_padding:  # the nearest map pixel instead of nothing
            inside = finite
            x, y = np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)
        cells.append(np.where(inside, y * W + x, -1))
        weights.append(wgt)
    return np.stack(cells), np.stack(weights)


def taps_sum(m, cells, weights):
    """sum over the neighbours inside the map of weight * m[cell], in tap order, starting from the first one inside"""
    flat = np.asarray(m).reshape(-1)
    acc = np.zeros(cells.shape[1:], dtype=weights.dtype)
    started = np.zeros(cells.shape[1:], dtype=bool)
    for c in range(4):
        inside = cells[c] >= 0
        term = weights[c] * flat[np.maximum(cells[c], 0)].astype(weights.dtype)
        acc = np.where(inside, np.where(started, acc + term, term), acc)
        started |= inside
    return acc


def as_map(m):
    """a uint8 / bool map counts as 0 / 1"""
    m = np.asarray(m)
    return (m != 0).astype(F) if m.dtype in (np.uint8, np.bool_) else m.astype(F)


def bilinear_at(m, ix, iy, **faults):
    m = as_map(m)
    cells, weights = taps(ix, iy, m.shape[0], m.shape[1], **faults)
    return taps_sum(m, cells, weights)


def warp(src, field, coords, **faults):
    """src [N,H,W] (float32, or uint8 as 0 / 1), field [N,Ho,Wo,2] -> float32 [N,Ho,Wo]"""
    src, field = np.asarray(src), np.asarray(field, dtype=F)
    pos_faults = {k: v for k, v in faults.items() if k in ("fault_swap_uv", "fault_align_corners")}
    tap_faults = {k: v for k, v in faults.items() if k not in pos_faults}
    out = []
    for m, f in zip(src, field):
        ix, iy = positions(f, m.shape[0], m.shape[1], coords, **pos_faults)
        out.append(bilinear_at(m, ix, iy, **tap_faults))
    return np.stack(out)


def cal_ciou(infer, gt):
    """utils.Evaluator.cal_CIOU's expression (utils.py:209-214) on a boolean infer map and a 0 / 1 gt map, fp64"""
    infer = infer.astype(np.float64)
    gt = gt.astype(np.float64)
    inter = np.sum(infer * gt)
    denom = np.sum(gt) + np.sum(infer * (gt == 0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float64(inter) / np.float64(denom), inter, denom


def consistency(pred, field, coords, fault_gt=False, **faults):
    """pred [T,S,S] uint8, field [T-1,S,S,2] -> float64 [T-1,3] = (cIoU, intersection, denominator)"""
    pred = np.asarray(pred)
    warped = warp(pred[:-1], field, coords, **faults)
    rows = []
    for k in range(len(pred) - 1):
        infer = warped[k] > F(0.5) if fault_gt else warped[k] >= F(0.5)
        rows.append(cal_ciou(infer, pred[k + 1] != 0))
    return np.array(rows, dtype=np.float64)


# ---------------------------------------------------------------- loss
FL_T = 256  # the kernels' block size


def block_sum(vals):
    """float32 [256] per-thread values summed as the kernel's block_sum does: the 64 lanes of each wave by xor butterfly
    (32, 16, ..., 1), then the four waves in order starting from 0"""
    v = np.asarray(vals, dtype=F).reshape(FL_T // 64, 64).copy()
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    total = F(0)
    for wave in range(FL_T // 64):
        total = total + v[wave, 0]
    return total


def strided_sum(vals):
    """thread tid adds vals[tid], vals[tid + 256], ... in order from 0; then block_sum"""
    vals = np.asarray(vals, dtype=F).reshape(-1)
    padded = np.zeros(-(-len(vals) // FL_T) * FL_T, dtype=F)
    padded[:len(vals)] = vals
    acc = np.zeros(FL_T, dtype=F)
    for row in padded.reshape(-1, FL_T):
        acc = acc + row
    return block_sum(acc)


def sign(d):
    return np.sign(d).astype(d.dtype)


def flow_loss_ordered(x, field, coords):
    """x [b,t,h,w] float32, field [b,t-1,h,w,2] -> (loss float32, dx float32 [b,t,h,w]) in avt_flow_loss's order"""
    x, field = np.asarray(x, dtype=F), np.asarray(field, dtype=F)
    b, t, h, w = x.shape
    P = h * w
    k = F(1) / (F(b) * F(t - 1) * F(P))
    partials = []
    dx = np.zeros((b, t, P), dtype=F)
    for c in range(b):
        sgn_prev = None
        for s in range(t):
            g = np.zeros(P, dtype=F)
            if s + 1 < t:
                ix, iy = positions(field[c, s], h, w, coords)
                cells, weights = taps(ix.reshape(-1), iy.reshape(-1), h, w)
                d = taps_sum(x[c, s], cells, weights) - x[c, s + 1].reshape(-1)
                partials.append(strided_sum(np.abs(d)))
                sg = sign(d)
                acc = np.zeros(P, dtype=F)
                for p in range(P):
                    for corner in range(4):
                        q = cells[corner, p]
                        if q >= 0:
                            acc[q] = acc[q] + sg[p] * weights[corner, p]
                g = g + acc * k
            if s > 0:
                g = g - sgn_prev * k
            if s + 1 < t:
                sgn_prev = sg
            dx[c, s] = g
    return strided_sum(partials) * k, dx.reshape(b, t, h, w)


def flow_loss_f64(x, field, coords):
    """The same loss in fp64 from the float32 sampling positions (the positions are part of the definition: one fp32
    add, or four fp32 operations, each).  Returns dict(loss, dx, loss_bound, dx_bound, min_margin):

    With u = 2^-24: a weight is a product of two differences of float32 numbers, each rounded once (relative error
    <= u), then rounded (u), times the map value (u): every term of the sample is within 4u of its fp64 value, and
    the three additions add at most 3u of sum|w m|; the difference with x[s+1] one more u of (sum|w m| + |x|).  So
    |d32 - d64| <= 8u (sum|w m| + |x|) =: e_p.  sum|d| passes through at most 4 (thread) + 6 (lanes) + 4 (waves)
    additions per launch, two launches, and one product: <= 32u sum|d| more (plus ceil(partials / 256)).  The sign of
    d is settled when |d64| > e_p: ``min_margin`` = min(|d64| - e_p), positive when every sign is.  With the signs
    equal, a gradient entry is k (G - sign): G a sum of n_q weights, each within 3u, added with at most n_q roundings,
    then one product, one or two additions and a product by k."""
    x32, field = np.asarray(x, dtype=F), np.asarray(field, dtype=F)
    x = x32.astype(np.float64)
    b, t, h, w = x.shape
    P = h * w
    u = EPS32
    k = 1.0 / (b * (t - 1) * P)
    total, sum_abs, sum_err, margin = 0.0, 0.0, 0.0, np.inf
    dx = np.zeros((b, t, P))
    dx_bound = np.zeros((b, t, P))
    for c in range(b):
        for s in range(t - 1):
            ix, iy = positions(field[c, s], h, w, coords)
            cells, weights = taps(ix.reshape(-1), iy.reshape(-1), h, w, dtype=np.float64)
            flat = x[c, s].reshape(-1)
            mag = np.zeros(P)
            for corner in range(4):
                mag += np.where(cells[corner] >= 0, np.abs(weights[corner] * flat[np.maximum(cells[corner], 0)]), 0.0)
            d = taps_sum(x[c, s], cells, weights) - x[c, s + 1].reshape(-1)
            e = 8 * u * (mag + np.abs(x[c, s + 1].reshape(-1)))
            margin = min(margin, float(np.min(np.abs(d) - e)))
            total += np.sum(np.abs(d))
            sum_abs += np.sum(np.abs(d))
            sum_err += np.sum(e)
            sg = np.sign(d)
            wsum, count = np.zeros(P), np.zeros(P)
            for corner in range(4):
                inside = cells[corner] >= 0
                np.add.at(dx[c, s], cells[corner][inside], sg[inside] * weights[corner][inside] * k)
                np.add.at(wsum, cells[corner][inside], np.abs(weights[corner][inside]))
                np.add.at(count, cells[corner][inside], 1.0)
            dx[c, s + 1] -= sg * k
            dx_bound[c, s] += u * k * ((count + 5) * wsum)
            dx_bound[c, s + 1] += u * k * 3
    npart = b * (t - 1)
    loss_bound = k * (sum_err + (33 + -(-npart // FL_T)) * u * sum_abs)
    return dict(loss=total * k, dx=dx.reshape(b, t, h, w), loss_bound=loss_bound,
                dx_bound=dx_bound.reshape(b, t, h, w) + 1e-45, min_margin=margin)


# ---------------------------------------------------------------- colour
SEGMENTS = (15, 6, 4, 11, 13, 6)  # RY, YG, GC, CB, BM, MR
NCOLS = sum(SEGMENTS)


def color_wheel():
    """utils.make_color_wheel (utils.py:64-111): float64 [55,3]"""
    RY, YG, GC, CB, BM, MR = SEGMENTS
    wheel = np.zeros([NCOLS, 3])
    col = 0
    wheel[0:RY, 0] = 255
    wheel[0:RY, 1] = np.floor(255 * np.arange(0, RY) / RY)
    col += RY
    wheel[col:col + YG, 0] = 255 - np.floor(255 * np.arange(0, YG) / YG)
    wheel[col:col + YG, 1] = 255
    col += YG
    wheel[col:col + GC, 1] = 255
    wheel[col:col + GC, 2] = np.floor(255 * np.arange(0, GC) / GC)
    col += GC
    wheel[col:col + CB, 1] = 255 - np.floor(255 * np.arange(0, CB) / CB)
    wheel[col:col + CB, 2] = 255
    col += CB
    wheel[col:col + BM, 2] = 255
    wheel[col:col + BM, 0] = np.floor(255 * np.arange(0, BM) / BM)
    col += BM
    wheel[col:col + MR, 2] = 255 - np.floor(255 * np.arange(0, MR) / MR)
    wheel[col:col + MR, 0] = 255
    return wheel


def compute_color(u, v, fault_no_wrap=False, fault_no_dim=False, force_branch=None):
    """utils.compute_color (utils.py:112-154) on fp64 copies.  Returns (values float64 [H,W,3] = 255 * col * (1 -
    nan) before the floor, rad, fk).  ``force_branch`` True / False takes the rad <= 1 / rad > 1 branch everywhere."""
    u, v = np.array(u, dtype=np.float64), np.array(v, dtype=np.float64)
    nan_idx = np.isnan(u) | np.isnan(v)
    u[nan_idx] = v[nan_idx] = 0
    wheel = color_wheel()
    ncols = np.size(wheel, 0)
    rad = np.sqrt(u ** 2 + v ** 2)
    a = np.arctan2(-v, -u) / np.pi
    fk = (a + 1) / 2 * (ncols - 1) + 1
    k0 = np.floor(fk).astype(int)
    k1 = k0 + 1
    if not fault_no_wrap:           # without it colour 56 is looked up: an IndexError wherever k0 reaches 55
        k1[k1 == ncols + 1] = 1
    f = fk - k0
    vals = np.zeros(u.shape + (3,))
    for i in range(3):
        tmp = wheel[:, i]
        col0 = tmp[k0 - 1] / 255
        col1 = tmp[k1 - 1] / 255
        col = (1 - f) * col0 + f * col1
        idx = rad <= 1 if force_branch is None else np.full(rad.shape, force_branch)
        col[idx] = 1 - rad[idx] * (1 - col[idx])
        notidx = np.logical_not(idx)
        if not fault_no_dim:
            col[notidx] *= 0.75
        vals[:, :, i] = 255 * col * (1 - nan_idx)
    return vals, rad, fk


def normalise(field):
    """flow2img up to compute_color's arguments: (u, v, unknown).  A NaN radius does not take part in the maximum
    (include/avt.h: the one departure from numpy's max, which would give NaN and then max(-1, nan) = -1)."""
    f = np.asarray(field, dtype=F).astype(np.float64)
    u, v = f[:, :, 0].copy(), f[:, :, 1].copy()
    unknown = (np.abs(u) > 1e7) | (np.abs(v) > 1e7)
    u[unknown] = v[unknown] = 0
    rad = np.sqrt(u ** 2 + v ** 2)
    finite = rad[~np.isnan(rad)]
    maxrad = max(-1, np.max(finite)) if finite.size else -1
    with np.errstate(invalid="ignore", divide="ignore"):
        u = u / maxrad + np.finfo(float).eps
        v = v / maxrad + np.finfo(float).eps
    return u, v, unknown


def to_bytes(vals, unknown):
    img = np.uint8(np.floor(vals))
    img[np.repeat(unknown[:, :, np.newaxis], 3, axis=2)] = 0
    return img


def flow2img(field, **faults):
    """utils.flow2img (utils.py:155-192) of one field [H,W,2] -> uint8 [H,W,3]; the argument is left alone"""
    u, v, unknown = normalise(field)
    return to_bytes(compute_color(u, v, **faults)[0], unknown)


# What a differently rounded sqrt / atan2 can move, in the chain's own units (ulp64(x) = spacing of doubles at x):
#  * atan2: the OpenCL full-profile bound the device library meets is 6 ulp, numpy's vector loops stay within 4 ulp
#    (glibc's scalar atan2 within 1): the two results differ by at most 10 ulp64(pi) = 10 * 2^-51.  The arguments
#    u / maxrad + eps differ by the maximum radius's sqrt (1 ulp either way, the same factor on u and v: no change
#    of angle) and by one rounding each of the divide and the add: at most 2 * 2 * 2^-53 of angle.
#  * a = theta / pi: the error over pi, plus one rounding (2^-53 at |a| <= 1).
#  * fk = (a + 1) / 2 * 54 + 1: 27 times the error of a (plus 27 roundings of a + 1 at 2^-52), plus the product's and
#    the sum's rounding at up to 2^-47 each.
#  * col = (1 - f) c0 + f c1 is continuous in fk (also across an integer fk, where k0 steps) with slope <= 1 / 4
#    (the steepest ramp has 4 steps); taken as 1.  Its own roundings: 4 * 2^-53.  rad: 2 ulp from u and v, 1 from its
#    sqrt: 4 * 2^-52 at rad ~ 1.  col' = 1 - rad (1 - col): the errors of col and rad add, 3 more roundings.
#  * 255 col': times 255, one rounding at 2^-45.
D_THETA = 10 * 2.0 ** -51 + 4 * 2.0 ** -53
D_A = D_THETA / np.pi + 2.0 ** -53
D_FK = 27 * (D_A + 2.0 ** -52) + 2 * 2.0 ** -47
D_RAD = 4 * 2.0 ** -52
D_COL = D_FK + 4 * 2.0 ** -53 + D_RAD + 3 * 2.0 ** -53
DELTA = 255 * D_COL + 2.0 ** -45          # ~2.2e-11, in units of 255 * col
DELTA_RAD = D_RAD


def flow2img_report(field):
    """(img, excused, alt): ``img`` the oracle's bytes; ``excused`` [H,W] marks the pixels another correctly-within-
    bounds sqrt / atan2 may change: one of the three 255 * col values lies within DELTA of an integer, or rad lies
    within DELTA_RAD of 1.  A value within DELTA of an integer does not excuse its channel when the wheel holds 255
    there at k0 and k1 (and, where fk is within D_FK of an integer so that k0 may step, at the next colour on that
    side): col is then (1 - f) + f = 1 exactly in fp64 for every f (1 - f is
    exact for f >= 1/2, and for f < 1/2 the sum is within 2^-54 of 1 and rounds to it), so the byte is 255 -- or
    floor(191.25) -- whatever the roundings before it.  ``alt`` holds the bytes of the other rad branch (equal to img
    away from rad ~ 1)."""
    u, v, unknown = normalise(field)
    vals, rad, fk = compute_color(u, v)
    img = to_bytes(vals, unknown)
    wheel = color_wheel()
    k0 = np.clip(np.floor(fk).astype(int), 1, NCOLS)
    f = (fk - k0)[:, :, None]
    at = lambda k: wheel[(k - 1) % NCOLS] == 255            # the wheel's entry of colour k (1-based, wrapping)
    held = at(k0) & at(k0 + 1) & ((f > D_FK) | at(k0 - 1)) & ((f < 1 - D_FK) | at(k0 + 2))
    near = (np.abs(vals - np.round(vals)) <= DELTA) & ~held
    near_rad = np.abs(rad - 1) <= DELTA_RAD
    dead = unknown | np.isnan(u) | np.isnan(v)            # black whatever the roundings
    excused = (near.any(axis=2) | near_rad) & ~dead
    other = to_bytes(compute_color(u, v, force_branch=False)[0], unknown)
    lower = to_bytes(compute_color(u, v, force_branch=True)[0], unknown)
    alt = np.where((rad <= 1)[:, :, None], other, lower)
    alt = np.where(near_rad[:, :, None], alt, img)
    return img, excused, alt


# ---------------------------------------------------------------- .flo
FLO_MAGIC = 202021.25


def write_flo(path, uv):
    """magic float32, width int32, height int32, rows of interleaved (u, v) float32, little endian"""
    uv = np.asarray(uv)
    h, w, _ = uv.shape
    with open(path, "wb") as f:
        f.write(np.array([FLO_MAGIC], dtype="<f4").tobytes())
        f.write(np.array([w, h], dtype="<i4").tobytes())
        f.write(uv.astype("<f4").tobytes())


def read_flo(path):
    raw = open(path, "rb").read()
    if np.frombuffer(raw, "<f4", 1)[0] != F(FLO_MAGIC):
        raise ValueError("bad magic")
    w, h = np.frombuffer(raw, "<i4", 2, 4)
    return np.frombuffer(raw, "<f4", 2 * int(w) * int(h), 12).reshape(int(h), int(w), 2)
