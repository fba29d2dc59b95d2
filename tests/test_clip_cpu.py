"""The colour arithmetic csrc/frames.hip ports for the two-view clip transform, restated in numpy
(tests/clip_oracle.py) and pinned bit-exactly against Pillow; ClipTransform.params' draws; and every
host-side refusal of ClipTransform (raised before any device work: none of this needs a GPU)."""
import random

import numpy as np
import pytest

import clip_oracle as co
from avt_amd import frames as fr
from avt_amd.frames import ClipParams, ClipTransform

FACTORS = (0.0, 0.5, 0.73, 1.0, 1.37, 1.5)


@pytest.fixture(scope="module")
def triples():
    a = co.all_triples()
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def sample():
    """uint8 [96, 128, 3]: random colours, a gray block, saturated primaries and black / white"""
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)
    a[:8] = a[:8, :, :1]
    a[8, :8] = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (0, 0, 0),
                (255, 255, 255)]
    a.setflags(write=False)
    return a


def test_gray_over_all_colours(triples):
    np.testing.assert_array_equal(co.np_gray(triples), co.pil_gray(triples))


def test_rgb_to_hsv_over_all_colours(triples):
    np.testing.assert_array_equal(co.np_rgb_to_hsv(triples), co.pil_rgb_to_hsv(triples))


def test_hsv_to_rgb_over_all_triples(triples):
    np.testing.assert_array_equal(co.np_hsv_to_rgb(triples), co.pil_hsv_to_rgb(triples))


def test_hue_zero_is_not_the_identity(triples):
    back = co.np_hsv_to_rgb(co.np_rgb_to_hsv(triples))
    same = (back == triples).all(axis=-1).mean()
    assert 0.1 < same < 0.3 and np.abs(back.astype(int) - triples.astype(int)).max() == 7


@pytest.mark.parametrize("kind", [co.BRIGHTNESS, co.CONTRAST, co.SATURATION])
@pytest.mark.parametrize("f", FACTORS)
def test_blend_ops_match_pillow(sample, kind, f):
    np.testing.assert_array_equal(co.np_op(sample, kind, f), co.pil_op(sample, kind, f))


@pytest.mark.parametrize("f", FACTORS)
def test_blend_saturating_pixels(f):
    """0 / 1 / 254 / 255 against every degenerate value: the clipping branch at both ends"""
    from PIL import Image

    img = np.tile(np.array([0, 1, 128, 254, 255], dtype=np.uint8), 5)[None, :, None].repeat(3, axis=2)
    deg = np.repeat(np.array([0, 1, 128, 254, 255], dtype=np.uint8), 5)[None, :, None].repeat(3, axis=2)
    ref = np.asarray(Image.blend(Image.fromarray(deg, "RGB"), Image.fromarray(img, "RGB"), f))
    np.testing.assert_array_equal(co.np_blend(deg, img, f), ref)


def test_contrast_mean_rounds_half_up():
    """a frame whose mean gray is exactly x.5, and a constant one"""
    a = np.zeros((2, 2, 3), dtype=np.uint8)
    a[0] = 101
    a[1] = 100
    assert co.np_contrast_mean(a) == 101
    for f in FACTORS:
        np.testing.assert_array_equal(co.np_op(a, co.CONTRAST, f), co.pil_op(a, co.CONTRAST, f))
        c = np.full((3, 5, 3), 77, dtype=np.uint8)
        np.testing.assert_array_equal(co.np_op(c, co.CONTRAST, f), co.pil_op(c, co.CONTRAST, f))


@pytest.mark.parametrize("shift", [-127, -1, 0, 1, 127])
def test_hue_shifts(sample, shift):
    h = shift / 255 + (1e-9 if shift >= 0 else -1e-9)
    assert co.hue_shift(h) == shift
    np.testing.assert_array_equal(co.np_op(sample, co.HUE, h), co.pil_op(sample, co.HUE, h))
    assert co.hue_shift(0.5) == 127 and co.hue_shift(-0.5) == -127


def test_chains_match_pillow(sample):
    ops = [(co.BRIGHTNESS, 1.37), (co.CONTRAST, 0.73), (co.SATURATION, 1.5), (co.HUE, -0.2)]
    for order in ([1, 0, 2, 3], [0, 1, 2, 3], [3, 2, 1, 0], [2, 3, 0, 1], []):
        chain = [ops[i] for i in order]
        np.testing.assert_array_equal(co.np_chain(sample, chain), co.pil_chain(sample, chain))


# ------------------------------------------------------------------------------------- params()
def test_params_reproduce_under_a_seed():
    t = ClipTransform(224, "train")
    a = [t.params(640, 360, random.Random(5)) for _ in range(2)]
    assert a[0] == a[1]
    p = a[0]
    assert (p.rw, p.rh) == (437, 246) and 0 <= p.crop_top <= 22 and 0 <= p.crop_left <= 213
    assert t.size2 == 156 and 0 <= p.crop2_top <= 68 and 0 <= p.crop2_left <= 68
    assert sorted(k for k, _ in p.ops) == [0, 1, 2, 3]
    for k, f in p.ops:
        assert (-0.5 <= f <= 0.5) if k == fr.HUE else (0.5 <= f <= 1.5)
    assert t.params(640, 360, random.Random(6)) != p


def test_params_draw_order():
    """the documented order, replayed by hand on a second generator"""
    t = ClipTransform(32, "train")
    p = t.params(56, 40, random.Random(11))  # -> 49 x 35
    r = random.Random(11)
    cj, ci, flip = r.randint(0, 49 - 32), r.randint(0, 35 - 32), r.random() < 0.5
    cj2, ci2 = r.randint(0, 10), r.randint(0, 10)
    ops = [(k, r.uniform(0.5, 1.5)) for k in (fr.BRIGHTNESS, fr.CONTRAST, fr.SATURATION)] + [(fr.HUE, r.uniform(-0.5, 0.5))]
    r.shuffle(ops)
    flip2 = r.random() < 0.5
    assert p == ClipParams(49, 35, ci, cj, flip, ci2, cj2, tuple(ops), flip2)


def test_params_make_no_crop_draw_without_a_range():
    t = ClipTransform(32, "train")
    assert t.resize_to == 35
    p = t.params(35, 35, random.Random(3))  # resized 35 x 35: both axes have a range
    q = ClipTransform(35, "train")
    q.resize_to = 35  # the resized frame equals the crop: no view-1 crop draw
    a = q.params(35, 35, random.Random(3))
    r = random.Random(3)
    flip = r.random() < 0.5
    cj2 = r.randint(0, 35 - 24)
    assert (a.crop_top, a.crop_left, a.flip, a.crop2_left) == (0, 0, flip, cj2)
    # one axis without a range: one draw
    b = ClipTransform(32, "train").params(45, 71, random.Random(3))  # -> 35 x 55
    r = random.Random(3)
    assert (b.rw, b.rh) == (35, 55) and b.crop_left == r.randint(0, 3) and b.crop_top == r.randint(0, 23)
    c = ClipTransform(32, "test").params(56, 40, random.Random(3))
    assert c == ClipParams(44, 32, 0, 6, False) and p.ops and not c.ops


def test_second_crop_size_matches_the_library():
    from avt_amd._lib import LIB_PATH
    import os

    for s in (2, 32, 100, 224, 256):
        assert ClipTransform(s).size2 == int(s * 0.7)
    if os.path.exists(LIB_PATH):
        from avt_amd._lib import query

        assert all(query("avt_clip_crop2", s) == int(s * 0.7) for s in range(1, 257))


# ------------------------------------------------------------------------------------- refusals
def _clip(h, w, t=2, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(t)]


def test_every_refusal_is_raised_on_the_host(monkeypatch):
    """ValueError before any device work: the library call and the allocator are never reached"""
    def never(*a, **k):
        raise AssertionError("reached the device")

    monkeypatch.setattr(fr, "call", never)
    monkeypatch.setattr(fr, "query", never)
    monkeypatch.setattr(fr, "_empty", never)
    for size in (1, 257):
        with pytest.raises(ValueError, match="image_size"):
            ClipTransform(size)
    with pytest.raises(ValueError, match="mode"):
        ClipTransform(32, "val")
    t = ClipTransform(32, "train")
    good = ClipParams(49, 35, 1, 2, True, 3, 4, ((fr.HUE, 0.1), (fr.CONTRAST, 1.2)), False)
    clip = _clip(40, 56)

    def bad(match, clips, **kw):
        with pytest.raises(ValueError, match=match):
            t(clips, device="cuda", **kw)

    bad("no clips", [])
    bad("no clips", [clip, []], params=[good, good])
    bad("same size", [[clip[0], clip[1][:39]]], params=[good])
    bad("same number", [clip, clip[:1]], params=[good, good])
    bad("per clip", [clip, clip], params=[good])
    bad("uint8", [[clip[0].astype(np.float32)]], params=[good])
    rep = dict(good.__dict__)
    for field, value, match in [
        ("ops", ((fr.HUE, 0.1), (fr.HUE, 0.2)), "repeated"),
        ("ops", ((fr.BRIGHTNESS, 1.0),) * 2, "repeated"),
        ("ops", ((4, 1.0),), "unknown"),
        ("ops", ((-1, 1.0),), "unknown"),
        ("ops", ((fr.BRIGHTNESS, -0.1),), "negative"),
        ("ops", ((fr.CONTRAST, -1e-9),), "negative"),
        ("ops", ((fr.SATURATION, float("nan")),), "negative"),
        ("ops", ((fr.HUE, 0.51),), "hue"),
        ("ops", ((fr.HUE, -0.5000001),), "hue"),
        ("crop_top", 4, "crop"), ("crop_top", -1, "crop"), ("crop_left", 18, "crop"), ("crop_left", -1, "crop"),
        ("crop2_top", 11, "crop"), ("crop2_top", -1, "crop"), ("crop2_left", 11, "crop"), ("crop2_left", -1, "crop"),
        ("rw", 31, "crop"), ("rh", 31, "crop"),
    ]:
        p = ClipParams(**{**rep, field: value})
        bad(match, [clip], params=[p])
        bad(match, [clip, clip], params=[good, p])  # a good clip first does not let it through
    tt =ClipTransform(40, "test")
    for h, w in [(304, 304), (304, 500), (500, 304)]:  # 304 / 40 = 7.6 on the short side
        with pytest.raises(ValueError, match="downscale"):
            tt([_clip(h, w, 1)], device="cuda")
