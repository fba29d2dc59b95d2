"""avt_frames_transform (avt_amd.frames.FrameTransform) at its edges, bit-exact float32 against
Pillow's resize + the restated crop / flip / ToTensor / Normalize (oracle/frames_oracle.py): the
top of the 32-entry tap table (downscale 7.5), upscales, the largest crop (S = 256 = the block
size), axes that are not resized, batches whose frames are far shorter than Hmax, saturating
content, and the host-side refusals (nothing may be launched)."""
import numpy as np
import pytest
import torch

import frames_oracle as fo
from avt_amd import frames as fr
from avt_amd.frames import FrameTransform

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
KMAX = 32  # FR_KMAX of csrc/frames.hip


def _frame(h, w, kind, seed=0):
    """uint8 [h, w, 3]: 'random'; 'gradient' (smooth ramps + saturated corners: the bicubic overshoot
    at the steps is clipped at 0 and 255, as in test_frames_gpu._frames); 'white' (all 255);
    'checker' (1-pixel checkerboard of 0 / 255)."""
    rng = np.random.default_rng(1000 * h + w + seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "white":
        return np.full((h, w, 3), 255, dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "checker":
        return np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
    assert kind == "gradient"
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[..., 0] = (yy * 255 // max(h - 1, 1)).astype(np.uint8)
    img[..., 1] = (xx * 255 // max(w - 1, 1)).astype(np.uint8)
    img[: max(h // 4, 1), : max(w // 4, 1)] = 255
    img[-max(h // 4, 1):, -max(w // 4, 1):] = 0
    return img


KINDS = ("random", "gradient", "white", "checker")


def _taps(in_size, out_size):
    """Pillow precompute_coeffs' tap count `xmax - xmin` per output index (Resample.c), restated."""
    scale = in_size / out_size
    support = 2.0 * max(scale, 1.0)
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        out.append(xmax - xmin)
    return out


def _corners(rw, rh, s):
    """Crop offsets touching every border of the resized frame (duplicates dropped)."""
    return sorted({(0, 0), (rh - s, rw - s), (0, rw - s), (rh - s, 0)})


def _check(t, frames, params):
    got = t(frames, params=params).cpu().numpy()
    s = t.size
    assert got.shape == (len(frames), 3, s, s) and got.dtype == np.float32
    for i, (f, (rw, rh, ci, cj, flip)) in enumerate(zip(frames, params)):
        ref = fo.frame_transform(f, rw, rh, ci, cj, flip, s, resize=fo.pil_resize)
        np.testing.assert_array_equal(
            got[i], ref, err_msg=f"frame {i} {f.shape} -> {rw}x{rh} @ ({ci},{cj}) flip={flip} S={s}")


@pytest.mark.parametrize("h,w", [(240, 300), (239, 480), (700, 240)])
def test_downscale_at_the_tap_table_limit(h, w):
    """Short side 240 -> 32 is the documented 7.5x; 239x480 is just under it on the short side and at
    it on the long one; 700x240 resizes to 93x32, where Resize's truncation of the long side makes
    that axis 7.53x and its tap count 31.  Centre crop plus crops on every border, all content kinds."""
    t = FrameTransform(32, "test")
    rw, rh = fo.resized_size(w, h, 32)
    # the case reaches the top of the kk[32] table and stays inside it (CPU, Pillow's own counts)
    for n_in, n_out in ((h, rh), (w, rw)):
        taps = _taps(n_in, n_out)
        assert taps == [c for _, c, _ in fo.precompute_coeffs(n_in, n_out)]
        assert 30 <= max(taps) <= KMAX, (n_in, n_out, max(taps))
    centre = t.params(w, h)
    assert centre[:2] == (rw, rh)
    params = [centre] + [(rw, rh, ci, cj, bool(k % 2)) for k, (ci, cj) in enumerate(_corners(rw, rh, 32))]
    frames = [_frame(h, w, KINDS[k % 4], seed=k) for k in range(len(params))]
    _check(t, frames, params)


def test_tap_count_bound_of_the_host_check():
    """The wrapper admits an axis factor f <= 8; Pillow's tap count is then <= ceil(4 f) <= 32."""
    worst = 0
    for n_out in (1, 2, 3, 31, 32, 33, 93, 256):
        for n_in in {n_out * 8, n_out * 8 - 1, int(n_out * 7.99), int(n_out * 7.53), int(n_out * 7.5)}:
            if n_in >= n_out:
                assert n_in / n_out <= fr.MAX_AXIS_DOWNSCALE
                worst = max(worst, max(_taps(n_in, n_out)))
    assert worst == KMAX


@pytest.mark.parametrize("h,w,s", [(40, 56, 32), (17, 300, 32), (100, 100, 224)])
def test_upscale(h, w, s):
    """Resize(int(1.1 S)) of frames smaller than the crop: 17 -> 35 (2.06x), 100 -> 246 (2.46x);
    40x56 -> 35x49 is the mild downscale next to it.  Border crops, drawn crops, both flips."""
    t = FrameTransform(s, "train")
    rw, rh = fo.resized_size(w, h, int(s * 1.1))
    torch.manual_seed(90 + h)
    params = [(rw, rh, ci, cj, bool(k % 2)) for k, (ci, cj) in enumerate(_corners(rw, rh, s))]
    params += [t.params(w, h) for _ in range(4)]
    frames = [_frame(h, w, KINDS[k % 4], seed=k) for k in range(len(params))]
    _check(t, frames, params)


def test_step_content_saturates_both_ways():
    """The 'gradient' content above really drives the resampler past [0, 255] before clip8 (CPU, restated
    horizontal pass of the 2.46x upscale), so the clip is exercised on both sides."""
    img = _frame(100, 100, "gradient").astype(np.int64)
    lo = hi = False
    for xmin, cnt, k in fo.precompute_coeffs(100, 246):
        v = ((1 << (fo.PRECISION_BITS - 1)) + np.einsum("hxc,x->hc", img[:, xmin:xmin + cnt], k)) >> fo.PRECISION_BITS
        lo, hi = lo or bool((v < 0).any()), hi or bool((v > 255).any())
    assert lo and hi


@pytest.mark.parametrize("mode", ["test", "train"])
@pytest.mark.parametrize("s", [256, 255])
def test_largest_crop(s, mode):
    """S = 256 fills the 256-thread block (no idle lane, kk[.][255] written); S = 255 is the odd
    size next to it.  Each frame once per flip state."""
    t = FrameTransform(s, mode)
    sizes = [(300, 420), (512, 512)]
    torch.manual_seed(91 + s)
    frames, params = [], []
    for k, (h, w) in enumerate(sizes):
        p = t.params(w, h)
        for flip in (False, True):
            frames.append(_frame(h, w, KINDS[(2 * k + flip) % 4], seed=k))
            params.append(p[:4] + (flip,))
    if mode == "train":  # the far corner of the resized frame as well
        rw, rh = fo.resized_size(420, 300, t.resize_to)
        frames.append(_frame(300, 420, "random", seed=9))
        params.append((rw, rh, rh - s, rw - s, True))
    _check(t, frames, params)


def test_identity_passes():
    """No resize in both axes with a zero crop offset (Pillow returns the image itself), and no
    resize in one axis only (Pillow skips that pass; the kernel runs it with the unit weight)."""
    t = FrameTransform(32, "test")
    frames = [_frame(32, 32, k) for k in KINDS]
    params = [t.params(32, 32) for _ in frames]
    assert all(p == (32, 32, 0, 0, False) for p in params)
    params[1] = (32, 32, 0, 0, True)
    # 48 x 40 frames: width kept (rw == W) and height resized up / down, then the converse
    frames += [_frame(48, 40, "gradient", 1), _frame(48, 40, "random", 2), _frame(48, 40, "checker", 3),
               _frame(48, 40, "random", 4), _frame(64, 32, "random", 5)]
    params += [(40, 60, 28, 8, False), (40, 33, 1, 0, True), (50, 48, 16, 18, False), (33, 48, 0, 1, True),
               (32, 64, 32, 0, False)]
    _check(t, frames, params)
    got = t(frames[:1], params=params[:1]).cpu().numpy()[0]
    np.testing.assert_array_equal(got, fo.to_tensor_normalize(frames[0]))


@pytest.mark.parametrize("pos", [0, 3, 5])
def test_mixed_batch_with_one_tall_frame(pos):
    """One 1080 x 1920 frame among five of 36-60 rows: Hmax is ~30x the small frames' H, so nearly
    every horizontal-pass block of a small frame is clipped to no rows by yr[0..1], and the
    intermediate planes are addressed with Hmax.  The tall frame is resized 7.5x (to 256 x 144) by
    explicit params."""
    t = FrameTransform(32, "train")
    small = [(36, 50), (41, 77), (48, 48), (55, 36), (60, 80)]
    torch.manual_seed(92)
    frames = [_frame(h, w, KINDS[k % 4], seed=k) for k, (h, w) in enumerate(small)]
    params = [t.params(w, h) for h, w in small]
    params[0] = params[0][:4] + (True,)
    params[1] = params[1][:4] + (False,)
    frames.insert(pos, _frame(1080, 1920, "gradient"))
    params.insert(pos, (256, 144, 144 - 32, 97, pos == 3))
    assert max(_taps(1080, 144)) >= 30
    _check(t, frames, params)


def test_refusals_launch_nothing(monkeypatch):
    """Every bad request raises ValueError on the host; avt_frames_transform is never called.  One
    good request afterwards shows that the spy sees a launch."""
    launched = []
    real = fr.call

    def spy(name, *args):
        launched.append(name)
        return real(name, *args)

    monkeypatch.setattr(fr, "call", spy)
    for size in (0, 257):
        with pytest.raises(ValueError, match="image_size"):
            FrameTransform(size, "test")
    t = FrameTransform(40, "test")
    for h, w in [(304, 304), (304, 500), (500, 304)]:  # 304 / 40 = 7.6 on the short side
        with pytest.raises(ValueError, match="downscale"):
            t([_frame(h, w, "random")])
    t = FrameTransform(32, "train")
    f = _frame(70, 90, "random")
    rw, rh = fo.resized_size(90, 70, 35)
    bad = [(rw, rh, rh - 32 + 1, 0, False), (rw, rh, 0, rw - 32 + 1, False), (rw, rh, -1, 0, False),
           (rw, rh, 0, -1, True), (31, rh, 0, 0, False), (rw, 20, 0, 0, False)]
    for p in bad:
        with pytest.raises(ValueError, match="crop"):
            t([f], params=[p])
        with pytest.raises(ValueError, match="crop"):  # a good frame first does not let it through
            t([f, f], params=[(rw, rh, 0, 0, False), p])
    with pytest.raises(ValueError, match="per frame"):
        t([f, f], params=[(rw, rh, 0, 0, False)])
    with pytest.raises(ValueError, match="no frames"):
        t([])
    with pytest.raises(ValueError, match="uint8"):
        t([f.astype(np.float32)])
    with pytest.raises(ValueError, match="uint8"):
        t([f[..., 0]])
    with pytest.raises(ValueError, match="uint8"):
        t([torch.from_numpy(f).to(DEV), torch.from_numpy(f[..., :2].copy()).to(DEV)])
    assert launched == []
    _check(t, [f], [(rw, rh, rh - 32, rw - 32, True)])
    assert launched == ["avt_frames_transform"]
