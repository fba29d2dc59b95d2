"""avt_heatmap_upsample and avt_render_overlay through the C ABI, bitwise against tests/render_oracle.py.

Every output lies between two 256-byte guard bands inside a larger buffer, as in test_layout_edges_gpu.py.  A uint8
result can hold any byte, so the calls run on a buffer filled with 0xA5 and on one filled with 0x5A (the aligned ones on both): the guards
must keep the fill and the interior must equal the oracle both times, so a byte the kernel skipped shows in one of
the two runs and a stray one in the guards.

  * heat maps: source sizes from 1 x 1 to 16 x 16, S = 2 (a downscale of most), 224 and the odd 255, one and three maps
    per launch, the three modes; a constant map (left unnormalised) and one spanning 1e-30 .. 1e30; a source above the
    LDS staging size; mode "pred", binarised as the protocol does, is localize's own map;
  * overlays: one pixel, 5 x 7 and 17 x 33 (H W % 4 != 0: scalar loads, and frames 1, 2 start at odd bytes of the
    output), 224 x 224 (16-byte loads, packed stores), each again with the frames, maps and output moved off their
    alignment; 0, 1 and 2 layers; random colour tables; per-frame ranges and a constant frame; weights above 1 and
    below 0 for both ends of the saturation; map values at 0, at 1 and one ulp below a truncation step."""
import ctypes

import numpy as np
import pytest
import torch

import render_oracle as ro
from avt_amd import evaluate as ev
from avt_amd import render
from avt_amd._lib import call

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256
FILLS = (0xA5, 0x5A)
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


class Guarded:
    """nbytes inside a uint8 buffer of `fill`: GUARD bytes in front, `skew` more to move the interior off its
    alignment, GUARD behind."""

    def __init__(self, nbytes, fill, skew=0):
        self.fill, self.lo, self.n = fill, GUARD + skew, nbytes
        self.buf = torch.full((self.lo + nbytes + GUARD,), fill, device=DEV, dtype=torch.uint8)
        assert self.buf.data_ptr() % 256 == 0
        self.t = self.buf[self.lo:self.lo + nbytes]
        _KEEP.append(self.buf)

    def guards_intact(self):
        return bool((self.buf[:self.lo] == self.fill).all()) and bool((self.buf[self.lo + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())

    def bytes(self):
        return self.t.cpu().numpy()


def _skewed(x, elems):
    """a device copy of x that starts `elems` elements past a 256-byte boundary"""
    x = torch.as_tensor(x)
    buf = torch.empty(x.numel() + elems, device=DEV, dtype=x.dtype)
    assert buf.data_ptr() % 256 == 0
    v = buf[elems:].view(x.shape)
    v.copy_(x)
    _KEEP.append(buf)
    return v


# ---------------------------------------------------------------------------------------------- heat maps
MODES = {"resize": 0, "norm": 1, "pred": -1}


def _heat_sources(N, h, w, seed):
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((N, h, w)) * 0.3 + 0.5).astype(np.float32)
    if N >= 3:
        mag = 10.0 ** rng.uniform(-30, 30, (h, w)) * rng.choice([-1.0, 1.0], (h, w))
        mag.flat[0] = 1e30
        A[1] = mag.astype(np.float32)
        A[2] = -0.75  # constant
    return A


def _upsample(dA, N, h, w, size, mode, fill):
    out = Guarded(N * size * size * 4, fill)
    call("avt_heatmap_upsample", P(dA), N, h, w, size, MODES[mode], P(out.t), S())
    torch.cuda.synchronize()
    assert out.guards_intact(), (mode, fill)
    return out.bytes().view(np.float32).reshape(N, size, size)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("size", [2, 224, 255])
@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (7, 9), (14, 14), (16, 16)])
def test_heatmap_upsample_bitwise(h, w, size, N):
    A = _heat_sources(N, h, w, 100 * h + 10 * w + size + N)
    dA = torch.from_numpy(A).to(DEV)
    for mode in MODES:
        ref = ro.heatmap(A, size, mode)
        assert np.isfinite(ref).all()
        for fill in FILLS:
            got = _upsample(dA, N, h, w, size, mode, fill)
            assert ro.first_difference(got, ref) is None, (mode, fill, ro.first_difference(got, ref))
        if N >= 3 and mode != "resize":
            # the constant map is left unnormalised -- where its resize is still constant: a0 + a1 is not always 1
            # in fp32, and then normalize_img stretches the rounding wobble to [0, 1], in the reference as here
            flat = ro.heatmap(A[2:], size, "resize")
            if (flat == np.float32(-0.75)).all():
                assert (ref[2] == (np.float32(-0.75) if mode == "norm" else np.float32(0.25))).all()  # 1 - (-(-.75))
            else:
                assert ref[2].min() == 0 and ref[2].max() == 1
            assert (flat == np.float32(-0.75)).all() or (h, w) != (1, 1)   # one source pixel: weights 1 and 0
        # the Python entry point gives the same bits, from [N,1,h,w] and from [N,h,w]
        for a in (dA[:, None], dA):
            assert torch.equal(ev.heatmaps(a, size=size, mode=mode).cpu(), torch.from_numpy(ref))


def test_heatmap_source_above_the_lds_staging_size():
    """300 x 17 = 5100 floats > 4096: read in place."""
    A = _heat_sources(3, 300, 17, 5)
    dA = torch.from_numpy(A).to(DEV)
    for mode in MODES:
        got = _upsample(dA, 3, 300, 17, 64, mode, FILLS[0])
        assert ro.first_difference(got, ro.heatmap(A, 64, mode)) is None, mode


def test_pred_mode_binarised_is_localizes_map():
    A = _heat_sources(3, 14, 14, 9)
    dA = torch.from_numpy(A).to(DEV)
    pred = ev.heatmaps(dA, mode="pred").cpu().numpy()
    _, maps = ev.localize(dA, return_maps=True)
    maps = maps.cpu().numpy()
    for i in range(3):
        np.testing.assert_array_equal((ro.median_binarize(pred[i]) >= 0.5).astype(np.uint8), maps[i], err_msg=str(i))
    assert maps[0].any() and not maps[0].all()


def test_heatmap_refusals():
    dA = torch.zeros(2, 3, 3, device=DEV)
    out = Guarded(2 * 8 * 8 * 4, FILLS[0])
    for args in [(None, 2, 3, 3, 8, 0, P(out.t)), (P(dA), 2, 3, 3, 8, 0, None), (P(dA), 0, 3, 3, 8, 0, P(out.t)),
                 (P(dA), 2, 0, 3, 8, 0, P(out.t)), (P(dA), 2, 3, -1, 8, 0, P(out.t)), (P(dA), 2, 3, 3, 1, 0, P(out.t)),
                 (P(dA), 2, 3, 3, 513, 0, P(out.t)), (P(dA), 2, 3, 3, 8, 2, P(out.t)), (P(dA), 2, 3, 3, 8, -2, P(out.t))]:
        with pytest.raises(RuntimeError, match="heatmap_upsample"):
            call("avt_heatmap_upsample", *args, S())
    torch.cuda.synchronize()
    assert out.untouched()
    with pytest.raises(ValueError, match="mode"):
        ev.heatmaps(dA, mode="median")
    with pytest.raises(ValueError, match=r"\[N,1,h,w\]"):
        ev.heatmaps(torch.zeros(2, 2, 3, 3, device=DEV))
    with pytest.raises(RuntimeError, match="GPU"):
        ev.heatmaps(torch.zeros(2, 3, 3))


# ---------------------------------------------------------------------------------------------- overlays
def _frames(N, H, W, rng):
    f = rng.standard_normal((N, 3, H, W)).astype(np.float32)
    if N >= 2:
        f[1] = f[1] * 4 - 100    # another range per frame
    if N >= 3:
        f[2] = 0.75              # a constant frame: left unnormalised, 0.75 * 255 * wimg everywhere
    return f


def _map(N, H, W, scale, rng):
    """values in [0, 1]: random, with 0, 1 and k / scale one ulp down (whose fp32 product with scale may round to k)
    planted at the front of every map"""
    m = rng.random((N, H, W)).astype(np.float32)
    steps = np.float32(np.arange(1, int(scale) + 1)) / np.float32(scale)
    special = np.concatenate([np.float32([0.0, 1.0]), np.nextafter(steps, np.float32(0)), steps])
    flat = m.reshape(N, -1)
    k = min(flat.shape[1], len(special))
    flat[:, :k] = special[:k]
    return flat.reshape(N, H, W)


def _render(f, layers, wimg, w0, lut, fill, skew):
    """layers: [(device map, scale)]; skew: (frames floats, map floats, out bytes) off alignment"""
    N, _, H, W = f.shape
    out = Guarded(N * H * W * 3, fill, skew=skew[2])
    (m0, s0), (m1, s1) = (layers + [(None, 0.0), (None, 0.0)])[:2]
    call("avt_render_overlay", P(f), N, H, W, P(m0), ctypes.c_float(s0), ctypes.c_double(w0), P(m1),
         ctypes.c_float(s1), ctypes.c_double(0.0), ctypes.c_float(wimg), P(lut), P(out.t), S())
    torch.cuda.synchronize()
    assert out.guards_intact(), (fill, skew)
    return out.bytes().reshape(N, H, W, 3)


WEIGHTS = [(0.4, 0.6), (0.5, 0.5), (0.8, 0.9), (-0.5, 0.3)]  # save_image, save_labels, above 1, below 0


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (17, 33), (224, 224)])
def test_render_overlay_bitwise(H, W, N):
    rng = np.random.default_rng(1000 * H + 10 * W + N)
    f = _frames(N, H, W, rng)
    maps = [(_map(N, H, W, 128, rng), 128.0), (_map(N, H, W, 255, rng), 255.0)]
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    dlut = torch.from_numpy(lut).to(DEV)
    for skew in [(0, 0, 0), (1, 3, 1), (0, 0, 2)]:
        df = _skewed(f, skew[0])
        dmaps = [(_skewed(m, skew[1]), s) for m, s in maps]
        for nl in (0, 1, 2):
            for k, (wimg, w0) in enumerate(WEIGHTS):
                ref = ro.overlay(f, lut, maps[:nl], wimg=wimg, w0=w0)
                for fill in (FILLS if skew == (0, 0, 0) else FILLS[(k + nl) % 2:][:1]):
                    got = _render(df, dmaps[:nl], wimg, w0, dlut if nl else None, fill, skew)
                    d = ro.first_difference(got, ref)
                    assert d is None, (skew, nl, wimg, w0, fill, d)


def test_cases_hit_what_they_are_for():
    """CPU arithmetic: the planted map values land on both sides of a truncation step, the weights above 1 overflow
    255 before saturation, and the constant frame takes the unnormalised branch."""
    rng = np.random.default_rng(3)
    m = _map(1, 17, 33, 255, rng)[0].reshape(-1)
    below = m[2:2 + 255]
    idx = ro.lut_index(below, 255)
    k = np.arange(1, 256)
    assert ((idx == k) | (idx == k - 1)).all() and (idx == k - 1).any()   # one ulp below k / 255: mostly k - 1
    assert (below * np.float32(255) < k).sum() == (idx == k - 1).sum()
    assert (ro.lut_index(m[:2], 255) == [0, 255]).all()
    f = _frames(3, 17, 33, rng)
    lut = np.full((256, 3), 255, np.uint8)
    a = ro.frame_term(f[0], 0.8)
    assert (np.add(a, lut[idx[:1]] * 0.9) > 255).any()
    assert (ro.frame_term(f[0], -0.5) < 0).any()
    assert (ro.frame_term(f[2], 0.4) == np.float32(0.75) * 255 * np.float32(0.4)).all()
    assert f[1].max() < f[0].min()   # batch-wide min / max would differ from per-frame ones


def test_render_refusals():
    N, H, W = 2, 4, 4
    f = torch.zeros(N, 3, H, W, device=DEV)
    m = torch.zeros(N, H, W, device=DEV)
    lut = torch.zeros(256, 3, device=DEV, dtype=torch.uint8)
    out = Guarded(N * H * W * 3, FILLS[0])

    def go(img=f, n=N, h=H, w=W, m0=None, m1=None, w1=0.0, table=lut, o=out.t):
        call("avt_render_overlay", P(img), n, h, w, P(m0), ctypes.c_float(255), ctypes.c_double(0.5), P(m1),
             ctypes.c_float(255), ctypes.c_double(w1), ctypes.c_float(0.5), P(table), P(o), S())

    for kw in [dict(m0=m, table=None), dict(m0=m, m1=m, table=None), dict(m1=m), dict(n=0), dict(h=0), dict(w=-3),
               dict(img=None), dict(o=None), dict(m0=m, m1=m, w1=0.5)]:
        with pytest.raises(RuntimeError, match="render_overlay"):
            go(**kw)
    torch.cuda.synchronize()
    assert out.untouched()
    go(table=None)  # no layer needs no table
    torch.cuda.synchronize()
    assert out.guards_intact() and not out.untouched()


def test_render_python_entry_points():
    """render.overlay / render.labels: the defaults are save_image / save_labels with render.JET, [b,3,t,H,W] folds to
    (b t), uint8 maps from localize and [N,1,H,W] maps are taken, and bad shapes are refused."""
    rng = np.random.default_rng(21)
    b, t, H, W = 2, 3, 12, 10
    video = rng.standard_normal((b, 3, t, H, W)).astype(np.float32)
    frames = video.transpose(0, 2, 1, 3, 4).reshape(b * t, 3, H, W)
    pred = (rng.random((b * t, H, W)) < 0.5).astype(np.uint8)
    gt = rng.choice([0.0, 0.5, 1.0], (b * t, H, W)).astype(np.float32)
    jet = render.JET.numpy()
    dv, dp, dg = torch.from_numpy(video).to(DEV), torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    got = render.overlay(dv, pred=dp, gt=dg)
    assert got.shape == (b * t, H, W, 3) and got.dtype == torch.uint8 and got.is_cuda
    for i in range(b * t):
        np.testing.assert_array_equal(got[i].cpu().numpy(),
                                      ro.save_image_expr(frames[i:i + 1], pred[i].astype(np.float32), gt[i], jet))
    lab = render.labels(torch.from_numpy(frames).to(DEV), dg[:, None]).cpu().numpy()
    for i in range(b * t):
        np.testing.assert_array_equal(lab[i], ro.save_labels_expr(frames[i:i + 1], gt[i], jet))
    only_pred = render.overlay(dv, pred=dp.float(), lut=render.JET.flip(1)).cpu().numpy()
    np.testing.assert_array_equal(only_pred, ro.overlay(frames, jet[:, ::-1], [(pred, 255)], wimg=0.4, w0=0.6))
    bare = render.overlay(dv).cpu().numpy()
    np.testing.assert_array_equal(bare, ro.overlay(frames, jet, [], wimg=0.4))
    with pytest.raises(ValueError, match="pred must be"):
        render.overlay(dv, pred=dp[:, :-1])
    with pytest.raises(ValueError, match="frames must be"):
        render.overlay(dv[:, :2])
    with pytest.raises(ValueError, match="colour table"):
        render.overlay(dv, pred=dp, lut=torch.zeros(256, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU"):
        render.overlay(torch.from_numpy(video))
