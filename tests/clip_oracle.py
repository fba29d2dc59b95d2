"""CPU oracle of the two-view clip transform (avt_amd.frames.ClipTransform) -- TEST INFRASTRUCTURE ONLY.

Two things live here:

- ``pil_*``: the transform done with Pillow itself, frame by frame (Image.resize(BICUBIC), crop,
  transpose, convert("L") / convert("HSV") / Image.blend-style enhancers), the way torchvision's and
  torchvideotransforms' PIL paths do it.  This is what the GPU tests compare against, bitwise.
- ``np_*``: the numpy restatement of every colour op (the arithmetic csrc/frames.hip ports), pinned
  against the ``pil_*`` functions in tests/test_clip_cpu.py; both hue conversions exhaustively.

Colour jitter ops are ``(kind, factor)`` with kind in BRIGHTNESS / CONTRAST / SATURATION / HUE, applied in
the order given, each to the previous op's 8-bit result (torchvision's ColorJitter).
"""
from __future__ import annotations

import numpy as np
from PIL import Image, ImageEnhance

import frames_oracle as fo

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------ Pillow
def _img(a: np.ndarray) -> Image.Image:
    return Image.fromarray(np.ascontiguousarray(a, dtype=np.uint8), "RGB")


def pil_gray(a: np.ndarray) -> np.ndarray:
    return np.asarray(_img(a).convert("L"))


def pil_rgb_to_hsv(a: np.ndarray) -> np.ndarray:
    return np.asarray(_img(a).convert("HSV"))


def pil_hsv_to_rgb(a: np.ndarray) -> np.ndarray:
    return np.asarray(Image.fromarray(np.ascontiguousarray(a, dtype=np.uint8), "HSV").convert("RGB"))


def hue_shift(h: float) -> int:
    """the 8-bit hue offset of a hue factor h in [-0.5, 0.5]: int(h * 255), truncated toward zero"""
    return int(h * 255)


def pil_op(a: np.ndarray, kind: int, f: float) -> np.ndarray:
    """one jitter op on a uint8 [h, w, 3] frame with Pillow (ImageEnhance = torchvision's adjust_*)"""
    im = _img(a)
    if kind == BRIGHTNESS:
        return np.asarray(ImageEnhance.Brightness(im).enhance(f))
    if kind == CONTRAST:
        return np.asarray(ImageEnhance.Contrast(im).enhance(f))
    if kind == SATURATION:
        return np.asarray(ImageEnhance.Color(im).enhance(f))
    assert kind == HUE
    h, s, v = im.convert("HSV").split()
    nh = ((np.asarray(h).astype(np.int64) + hue_shift(f)) % 256).astype(np.uint8)
    return np.asarray(Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB"))


def pil_chain(a: np.ndarray, ops) -> np.ndarray:
    for kind, f in ops:
        a = pil_op(a, kind, f)
    return np.asarray(a)


def pil_view1(frame: np.ndarray, p, s: int) -> np.ndarray:
    """uint8 [s, s, 3]: Resize -> crop -> flip of one frame under the clip's parameters p"""
    r = fo.pil_resize(frame, p.rw, p.rh)
    c = r[p.crop_top:p.crop_top + s, p.crop_left:p.crop_left + s]
    return np.ascontiguousarray(c[:, ::-1] if p.flip else c)


def pil_view2(v1: np.ndarray, p, s: int) -> np.ndarray:
    """uint8 [s, s, 3]: crop(int(0.7 s)) -> jitter chain -> Resize(s) -> flip of the 8-bit view 1"""
    s2 = int(s * 0.7)
    c = np.ascontiguousarray(v1[p.crop2_top:p.crop2_top + s2, p.crop2_left:p.crop2_left + s2])
    r = fo.pil_resize(pil_chain(c, p.ops), s, s)
    return np.ascontiguousarray(r[:, ::-1] if p.flip2 else r)


def pil_clips(clips, params, s: int, train: bool = True):
    """(frames, augmented) float32 [b, 3, t, s, s] (augmented None in test mode), normalised in fp32
    with the formula of csrc/frames.hip (oracle/frames_oracle.to_tensor_normalize)"""
    b, t = len(clips), len(clips[0])
    fr = np.empty((b, 3, t, s, s), dtype=np.float32)
    au = np.empty_like(fr) if train else None
    for i, (clip, p) in enumerate(zip(clips, params)):
        for k, frame in enumerate(clip):
            v1 = pil_view1(np.asarray(frame), p, s)
            fr[i, :, k] = fo.to_tensor_normalize(v1)
            if train:
                au[i, :, k] = fo.to_tensor_normalize(pil_view2(v1, p, s))
    return fr, au


# ------------------------------------------------------------------------------ numpy restatement
def np_gray(a: np.ndarray) -> np.ndarray:
    """convert("L"): (19595 R + 38470 G + 7471 B + 0x8000) >> 16"""
    a = a.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)


def np_blend(deg: np.ndarray, img: np.ndarray, f: float) -> np.ndarray:
    """Image.blend(deg, img, f) on uint8: fp32, separately rounded multiply and add; truncation for
    0 <= f <= 1, else clipped at 0 / 255 and truncated"""
    f32 = np.float32
    d, x = deg.astype(f32), img.astype(f32)
    tmp = d + f32(f) * (x - d)
    if 0.0 <= f <= 1.0:
        return tmp.astype(np.int32).astype(np.uint8)
    return np.where(tmp <= 0, 0, np.where(tmp >= 255, 255, tmp.astype(np.int32))).astype(np.uint8)


def np_contrast_mean(a: np.ndarray) -> int:
    """int(sum(L) / count + 0.5), the division in double (ImageStat mean of the frame's "L")"""
    g = np_gray(a)
    return int(int(g.astype(np.int64).sum()) / g.size + 0.5)


def np_rgb_to_hsv(a: np.ndarray) -> np.ndarray:
    """convert("HSV") (Convert.c rgb2hsv_row, after colorsys): float32 h, s; the hue's constants are
    doubles, so `2.0 + rc - bc`, `h / 6.0 + 1.0` and `h * 255.0` are evaluated in double"""
    f32, f64 = np.float32, np.float64
    r, g, b = (a[..., i].astype(np.int32) for i in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    gray = maxc == minc
    cr = np.where(gray, 1, maxc - minc).astype(f32)
    mx = np.where(maxc == 0, 1, maxc).astype(f32)
    s = cr / mx
    rc, gc, bc = ((maxc - c).astype(f32) / cr for c in (r, g, b))
    h = np.where(r == maxc, (bc - gc).astype(f64),
                 np.where(g == maxc, f64(2.0) + rc.astype(f64) - bc.astype(f64),
                          f64(4.0) + gc.astype(f64) - rc.astype(f64))).astype(f32)
    h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
    uh = np.clip((h.astype(f64) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(f64) * 255.0).astype(np.int64), 0, 255)
    out = np.stack([np.where(gray, 0, uh), np.where(gray, 0, us), maxc], axis=-1)
    return out.astype(np.uint8)


def _round_half_away(x: np.ndarray) -> np.ndarray:
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5)).astype(np.int64)


def np_hsv_to_rgb(a: np.ndarray) -> np.ndarray:
    """convert("RGB") of an HSV image (Convert.c hsv2rgb, after colorsys): sector i = floor(h 6 / 255)
    in double, f and fs rounded to float32, p / q / t = round(v (1 - ...)) in double, half away from 0"""
    f32, f64 = np.float32, np.float64
    h, s, v = (a[..., i].astype(f64) for i in range(3))
    h6 = h * 6.0 / 255.0
    i = np.floor(h6).astype(np.int64)
    f = (h6 - i.astype(f32).astype(f64)).astype(f32).astype(f64)
    fs = (s / 255.0).astype(f32).astype(f64)
    p = np.clip(_round_half_away(v * (1.0 - fs)), 0, 255)
    q = np.clip(_round_half_away(v * (1.0 - fs * f)), 0, 255)
    t = np.clip(_round_half_away(v * (1.0 - fs * (1.0 - f))), 0, 255)
    vi = a[..., 2].astype(np.int64)
    sect = i % 6
    r = np.choose(sect, [vi, q, p, p, t, vi])
    g = np.choose(sect, [t, vi, vi, q, p, p])
    b = np.choose(sect, [p, p, t, vi, vi, q])
    gray = a[..., 1] == 0
    out = np.stack([np.where(gray, vi, r), np.where(gray, vi, g), np.where(gray, vi, b)], axis=-1)
    return out.astype(np.uint8)


def np_op(a: np.ndarray, kind: int, f: float) -> np.ndarray:
    if kind == BRIGHTNESS:
        return np_blend(np.zeros_like(a), a, f)
    if kind == CONTRAST:
        return np_blend(np.full_like(a, np_contrast_mean(a)), a, f)
    if kind == SATURATION:
        return np_blend(np.repeat(np_gray(a)[..., None], 3, axis=2), a, f)
    assert kind == HUE
    hsv = np_rgb_to_hsv(a)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int64) + hue_shift(f)) % 256).astype(np.uint8)
    return np_hsv_to_rgb(hsv)


def np_chain(a: np.ndarray, ops) -> np.ndarray:
    for kind, f in ops:
        a = np_op(a, kind, f)
    return a


def all_triples() -> np.ndarray:
    """every one of the 2^24 byte triples, uint8 [4096, 4096, 3]"""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
