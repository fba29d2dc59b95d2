"""Seeded inputs shared by tests/test_flow_cpu.py and tests/test_flow_gpu.py -- TEST INFRASTRUCTURE ONLY.

The CPU file shows what the inputs are good for (they tell the injected faults apart, the colour fields keep the
oracle's excused share under the cap); the GPU file runs the kernels on the same arrays."""
import numpy as np

F = np.float32
SHAPES = [(1, 1), (2, 3), (14, 14), (17, 33), (64, 64), (224, 224)]
FIELD_KINDS = ["zero", "shift_out", "half", "random", "nonfinite"]


def checkerboard(N, H, W, dtype=np.uint8):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([((yy + xx + n) % 2) for n in range(N)]).astype(dtype)


def binary_maps(N, H, W, seed):
    """uint8 maps: checkerboard first, then random blobs"""
    rng = np.random.default_rng(seed)
    m = (rng.random((N, H, W)) < 0.45).astype(np.uint8)
    m[0] = checkerboard(1, H, W)[0]
    return m


def float_maps(N, H, W, seed):
    return np.random.default_rng(seed).standard_normal((N, H, W)).astype(F)


def pixel_field(kind, N, H, W, seed):
    """[N,H,W,2] float32 displacements in pixels"""
    rng = np.random.default_rng(seed)
    f = np.zeros((N, H, W, 2), dtype=F)
    if kind == "shift_out":       # whole pixels, far enough to push the map out on one side or the other
        f[..., 0] = W + 1
        f[N // 2:, :, :, 0] = 0
        f[N // 2:, :, :, 1] = -(H + 1)
    elif kind == "half":          # every interior sample of a checkerboard is exactly 0.5
        f[..., 0] = 0.5
    elif kind in ("random", "nonfinite"):
        # positions from two pixels outside every edge to two pixels outside the other
        yy, xx = np.mgrid[0:H, 0:W]
        f[..., 0] = rng.uniform(-3.0, W + 2.0, (N, H, W)) - xx
        f[..., 1] = rng.uniform(-3.0, H + 2.0, (N, H, W)) - yy
        f = f.astype(F)
        if kind == "nonfinite":
            bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38], dtype=F)
            flat = f.reshape(-1)
            idx = rng.choice(flat.size, size=min(flat.size, 2 * len(bad)), replace=False)
            flat[idx] = np.resize(bad, idx.size)
    else:
        assert kind == "zero", kind
    return f


def grid_field(kind, N, Ho, Wo, seed):
    """[N,Ho,Wo,2] float32 grid_sample coordinates reaching beyond [-1, 1]"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(-1.3, 1.3, (N, Ho, Wo, 2)).astype(F)
    if kind == "zero":
        f[:] = 0
    elif kind == "shift_out":
        f[:] = 3
    elif kind == "nonfinite":
        bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38], dtype=F)
        flat = f.reshape(-1)
        idx = rng.choice(flat.size, size=min(flat.size, 2 * len(bad)), replace=False)
        flat[idx] = np.resize(bad, idx.size)
    return f


def quarter_field(shape, seed, reach=2.0):
    """displacements in quarters of a pixel, |.| <= reach"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-int(4 * reach), int(4 * reach) + 1, shape) / 4.0).astype(F)


def loss_inputs(b, t, h, w, seed, exact):
    """x [b,t,h,w], field [b,t-1,h,w,2] (pixels).  exact: integer maps in [-8, 8] and quarter-pixel fields, so every
    product and sum of the loss is exact in float32 in any order; frame 1 of clip 0 repeats frame 0 under a zero
    field at pixel 0 (d = 0 there)."""
    rng = np.random.default_rng(seed)
    if exact:
        x = rng.integers(-8, 9, (b, t, h, w)).astype(F)
        f = quarter_field((b, t - 1, h, w, 2), seed + 1)
        f[0, 0, 0, 0] = 0
        x[0, 1, 0, 0] = x[0, 0, 0, 0]
    else:
        x = rng.standard_normal((b, t, h, w)).astype(F)
        f = rng.uniform(-2.0, 2.0, (b, t - 1, h, w, 2)).astype(F)
    return x, f


def wheel_field():
    """[12,55,2]: per row one radius (a multiple of 1/64 below 1, times a unit vector rounded to float32), per column
    one of the wheel's 55 segments: columns 0 .. 53 point at the middle of the segment between colours k + 1 and
    k + 2 (fk = k + 1.5), column 54 where fk reaches 55 and k1 wraps to 1; pixel (0, 0) is replaced by the vector
    (1, 0): the maximum radius, exactly 1 (row 1 still shows segment 0)."""
    ncols = 55
    k = np.arange(ncols - 1)
    ang = ((k + 0.5) / (ncols - 1) * 2 - 1) * np.pi       # a = atan2(-v, -u) / pi at fk = k + 1.5
    radii = np.array([3, 7, 13, 19, 23, 29, 37, 41, 47, 53, 59, 61]) / 64.0
    f = np.zeros((len(radii), ncols, 2), dtype=F)
    f[:, :ncols - 1, 0] = (-np.cos(ang)[None] * radii[:, None]).astype(F)
    f[:, :ncols - 1, 1] = (-np.sin(ang)[None] * radii[:, None]).astype(F)
    f[:, ncols - 1, 0] = radii                               # -u < 0, -v = +tiny: atan2 rounds to pi, fk = 55
    f[:, ncols - 1, 1] = F(-2.3e-16)                        # + eps = -8e-18: under half an ulp of pi from pi
    f[0, 0] = (1.0, 0.0)
    return f


def color_fields():
    """name -> [H,W,2] float32, every colour field the GPU test draws"""
    rng = np.random.default_rng(77)
    out = {}
    for H, W in ((3, 5), (17, 33), (224, 224)):
        out[f"random{H}x{W}"] = (rng.standard_normal((H, W, 2)) * rng.choice([0.3, 2.0, 40.0])).astype(F)
    out["wheel"] = wheel_field()
    out["zero"] = np.zeros((5, 7, 2), dtype=F)
    f = (rng.standard_normal((17, 33, 2)) * 3).astype(F)
    f[2, 3, 0] = 2e7
    f[4, 5, 1] = -np.inf
    f[6, 7, 0] = np.nan
    f[8, 9] = (np.nan, 1.0)
    out["unknown_nan"] = f
    return out
