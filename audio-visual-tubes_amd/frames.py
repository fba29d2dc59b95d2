"""Frame front end of the reference's datasets on libavt.

``GetAudioVideoDataset`` (datasets/dataloader.py:47-62, applied at :81) turns each decoded RGB frame
into the network input on the host with PIL + torchvision:
    train: Resize(int(224 * 1.1), BICUBIC) -> RandomCrop(224) -> RandomHorizontalFlip()
           -> CenterCrop(224) -> ToTensor() -> Normalize(mean, std)
    test:  Resize(224, BICUBIC) -> CenterCrop(224) -> ToTensor() -> Normalize(mean, std)
``FrameTransform`` does the same for a whole batch of decoded frames (any sizes) in two launches
(``avt_frames_transform``); its resize is bit-identical to Pillow's, and with the same torch RNG state
it draws the same crops and flips as torchvision (RandomCrop's two ``torch.randint`` then the flip's
``torch.rand``, per frame, in that order; no crop draw when the image already has the crop's size).
JPEG decoding stays with the loader.

``SubSampledFlickr`` (datasets/dataloader.py:155-181, 260-263) feeds the 16-frame two-view step with two
tensors per clip; ``ClipTransform`` below builds both on the GPU (``avt_clip_transform``).
"""
from __future__ import annotations

import ctypes
import random
from dataclasses import dataclass

import numpy as np
import torch

from ._lib import call, query
from .trunk import P, stream_ptr

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
MAX_DOWNSCALE = 7.5  # supported factor of the resize (its short side)
# One axis alone may go up to 8: a factor f needs at most ceil(4 f) bicubic taps per output pixel and
# csrc/frames.hip holds FR_KMAX = 32.  Resize(int) truncates the long side, int(size * long / short),
# so that axis shrinks a little more than the short one (700x240 -> 93x32: 7.53 for a 7.5 resize).
MAX_AXIS_DOWNSCALE = 8.0


def resized_size(w: int, h: int, size: int) -> tuple[int, int]:
    """torchvision Resize(int) on a PIL image of size (w, h): the short side becomes `size`."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    return (new_short, new_long) if w <= h else (new_long, new_short)


class FrameTransform:
    """``img_transform`` of datasets/dataloader.py:47-62 on the GPU: frames (uint8 [H, W, 3] arrays,
    tensors or RGB PIL images) -> float32 [n, 3, S, S] on the device."""

    def __init__(self, image_size: int = 224, mode: str = "train", mean=MEAN, std=STD):
        if mode not in ("train", "test"):
            raise ValueError(f"avt: mode must be 'train' or 'test', got {mode!r}")
        if not 1 <= image_size <= 256:
            raise ValueError("avt: image_size must be in [1, 256]")
        self.size = image_size
        self.mode = mode
        self.resize_to = int(image_size * 1.1) if mode == "train" else image_size
        self._mean = (ctypes.c_float * 3)(*mean)
        self._std = (ctypes.c_float * 3)(*std)

    def params(self, w: int, h: int, generator: torch.Generator | None = None):
        """(resized_w, resized_h, crop_top, crop_left, flip) for a w x h frame; in train mode drawn
        from the torch RNG exactly as RandomCrop + RandomHorizontalFlip draw them."""
        s = self.size
        rw, rh = resized_size(w, h, self.resize_to)
        if rw < s or rh < s:
            raise ValueError(f"avt: resized frame {rw}x{rh} is smaller than the crop {s}")
        if self.mode == "train":
            if rw == s and rh == s:
                ci = cj = 0
            else:
                ci = int(torch.randint(0, rh - s + 1, size=(1,), generator=generator).item())
                cj = int(torch.randint(0, rw - s + 1, size=(1,), generator=generator).item())
            flip = bool(torch.rand(1, generator=generator).item() < 0.5)
        else:  # CenterCrop
            ci, cj, flip = int(round((rh - s) / 2.0)), int(round((rw - s) / 2.0)), False
        return rw, rh, ci, cj, flip

    def __call__(self, frames, params=None, device=None, generator: torch.Generator | None = None) -> torch.Tensor:
        frames = [_as_uint8(f) for f in frames]
        if not frames:
            raise ValueError("avt: no frames")
        device = torch.device(device) if device is not None else (
            frames[0].device if frames[0].is_cuda else torch.device("cuda"))
        if device.type != "cuda":
            raise RuntimeError("avt: the frame transform runs on the GPU (no CPU path)")
        if params is None:
            params = [self.params(f.shape[1], f.shape[0], generator) for f in frames]
        if len(params) != len(frames):
            raise ValueError("avt: one parameter tuple per frame")
        s, n = self.size, len(frames)
        desc = np.zeros((n, 8), dtype=np.int64)
        off = 0
        for i, (f, (rw, rh, ci, cj, flip)) in enumerate(zip(frames, params)):
            H, W = f.shape[0], f.shape[1]
            if not (0 <= ci <= rh - s and 0 <= cj <= rw - s):
                raise ValueError(f"avt: crop ({ci}, {cj}) of {s} outside the {rw}x{rh} resized frame")
            if min(H / rh, W / rw) > MAX_DOWNSCALE or max(H / rh, W / rw) > MAX_AXIS_DOWNSCALE:
                raise ValueError(f"avt: downscale {W}x{H} -> {rw}x{rh} exceeds {MAX_DOWNSCALE}x")
            desc[i] = (off, H, W, rh, rw, ci, cj, int(bool(flip)))
            off += H * W * 3
        hmax = int(desc[:, 1].max())
        src = torch.cat([f.reshape(-1).to(device, non_blocking=True) for f in frames])
        d_desc = torch.from_numpy(desc).to(device)
        tmp = torch.empty(n * 3 * hmax * s, device=device, dtype=torch.uint8)
        out = torch.empty(n, 3, s, s, device=device, dtype=torch.float32)
        with torch.cuda.device(device):
            call("avt_frames_transform", P(src), P(d_desc), n, s, hmax, P(tmp),
                 ctypes.cast(self._mean, ctypes.c_void_p), ctypes.cast(self._std, ctypes.c_void_p), P(out),
                 stream_ptr())
        return out


BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3  # AVT_JITTER_* of include/avt.h
JITTER = 0.5  # ColorJitter(0.5, 0.5, 0.5, 0.5)
# avt_clip_view2 of include/avt.h (80 bytes)
_VIEW2 = np.dtype([("crop_top", "<i4"), ("crop_left", "<i4"), ("flip", "<i4"), ("nops", "<i4"),
                   ("ops", [("kind", "<i4"), ("reserved", "<i4"), ("factor", "<f8")], (4,))])


@dataclass(frozen=True)
class ClipParams:
    """One clip's draw: view 1 is Resize to rw x rh, crop S at (crop_top, crop_left), flip; view 2 is
    the crop int(0.7 S) at (crop2_top, crop2_left) of view 1's 8-bit image, the ordered chain `ops` of
    (kind, factor), Resize(S), flip2."""
    rw: int
    rh: int
    crop_top: int
    crop_left: int
    flip: bool
    crop2_top: int = 0
    crop2_left: int = 0
    ops: tuple = ()
    flip2: bool = False


def _empty(shape, dtype, device) -> torch.Tensor:
    """every device buffer of ClipTransform comes from here"""
    return torch.empty(shape, dtype=dtype, device=device)


class ClipTransform:
    """``video_transform`` / ``video_transform2`` / ``normalize_transform`` of datasets/dataloader.py:155-181
    on the GPU: b clips of t decoded frames -> ``(frames, augmented)``, float32 [b, 3, t, S, S] on the device
    (``frames`` alone in test mode: Resize(S) + CenterCrop).

    View 1 (``frames``): Resize(int(1.1 S), bicubic) -> RandomCrop(S) -> RandomHorizontalFlip, one draw per
    clip, applied to all its frames.  View 2 (``augmented``), from view 1's 8-bit result: RandomCrop(int(0.7 S))
    -> ColorJitter(0.5, 0.5, 0.5, 0.5) -> Resize(S, bicubic) -> RandomHorizontalFlip.  Both end in ClipToTensor +
    Normalize.  Five launches for the whole batch (two in test mode).

    Parity is pinned to Pillow (12.2.0), bitwise: the resampler is Image.resize(BICUBIC); brightness,
    contrast and saturation are ImageEnhance.Brightness / Contrast / Color (the contrast mean is per frame, every
    factor per clip); hue h in [-0.5, 0.5] is convert("HSV"), H' = (H + shift) mod 256 with
    shift = int(h * 255) truncated toward zero, convert("RGB").  That wrap rule is this project's definition.
    Pillow's RGB -> HSV -> RGB is lossy, so hue 0 is not the identity: it goes through the conversion as
    torchvision's does.  The jitter is an ordered chain, each op on the previous op's 8-bit result
    (torchvision's ColorJitter); a one-element chain gives a "last op only" jitter.

    The draw order of ``params`` is this project's own (the library the reference uses is not pinned), from
    Python's ``random``: (1) view-1 crop x, (2) view-1 crop y, each ``randint(0, range)`` and not drawn when
    the axis has no range, (3) view-1 flip ``random() < 0.5``, (4) view-2 crop x, (5) view-2 crop y,
    (6) brightness, contrast, saturation factors, each ``uniform(max(0, 1 - 0.5), 1.5)``, (7) hue
    ``uniform(-0.5, 0.5)``, (8) ``shuffle`` of the four ops, (9) view-2 flip."""

    def __init__(self, image_size: int = 224, mode: str = "train", mean=MEAN, std=STD):
        if mode not in ("train", "test"):
            raise ValueError(f"avt: mode must be 'train' or 'test', got {mode!r}")
        if not 2 <= image_size <= 256:
            raise ValueError("avt: image_size must be in [2, 256]")
        self.size = image_size
        self.size2 = int(image_size * 0.7)
        self.mode = mode
        self.resize_to = int(image_size * 1.1) if mode == "train" else image_size
        self._mean = (ctypes.c_float * 3)(*mean)
        self._std = (ctypes.c_float * 3)(*std)

    def params(self, w: int, h: int, rng: random.Random | None = None) -> ClipParams:
        """The draw for one clip of w x h frames (the order is in the class docstring); test mode draws nothing."""
        rng = rng if rng is not None else random
        s, s2 = self.size, self.size2
        rw, rh = resized_size(w, h, self.resize_to)
        if rw < s or rh < s:
            raise ValueError(f"avt: resized frame {rw}x{rh} is smaller than the crop {s}")
        if self.mode != "train":  # CenterCrop
            return ClipParams(rw, rh, int(round((rh - s) / 2.0)), int(round((rw - s) / 2.0)), False)
        cj = rng.randint(0, rw - s) if rw > s else 0
        ci = rng.randint(0, rh - s) if rh > s else 0
        flip = rng.random() < 0.5
        cj2 = rng.randint(0, s - s2)
        ci2 = rng.randint(0, s - s2)
        ops = [(kind, rng.uniform(max(0.0, 1.0 - JITTER), 1.0 + JITTER)) for kind in (BRIGHTNESS, CONTRAST, SATURATION)]
        ops.append((HUE, rng.uniform(-JITTER, JITTER)))
        rng.shuffle(ops)
        flip2 = rng.random() < 0.5
        return ClipParams(rw, rh, ci, cj, flip, ci2, cj2, tuple(ops), flip2)

    def _check(self, p: ClipParams, H: int, W: int) -> None:
        s, s2 = self.size, self.size2
        if not (0 <= p.crop_top <= p.rh - s and 0 <= p.crop_left <= p.rw - s):
            raise ValueError(f"avt: crop ({p.crop_top}, {p.crop_left}) of {s} outside the {p.rw}x{p.rh} resized frame")
        if min(H / p.rh, W / p.rw) > MAX_DOWNSCALE or max(H / p.rh, W / p.rw) > MAX_AXIS_DOWNSCALE:
            raise ValueError(f"avt: downscale {W}x{H} -> {p.rw}x{p.rh} exceeds {MAX_DOWNSCALE}x")
        if self.mode != "train":
            return
        if not (0 <= p.crop2_top <= s - s2 and 0 <= p.crop2_left <= s - s2):
            raise ValueError(f"avt: crop ({p.crop2_top}, {p.crop2_left}) of {s2} outside the {s}x{s} first view")
        kinds = [k for k, _ in p.ops]
        if any(k not in (BRIGHTNESS, CONTRAST, SATURATION, HUE) for k in kinds):
            raise ValueError(f"avt: unknown jitter op in {kinds}")
        if len(set(kinds)) != len(kinds):
            raise ValueError(f"avt: repeated jitter op in {kinds}")
        for k, f in p.ops:
            if k == HUE:
                if not -0.5 <= f <= 0.5:
                    raise ValueError(f"avt: hue factor {f} outside [-0.5, 0.5]")
            elif not (0.0 <= f < float("inf")):
                raise ValueError(f"avt: negative jitter factor {f}")

    def __call__(self, clips, params=None, device=None, rng: random.Random | None = None):
        clips = [[_as_uint8(f) for f in clip] for clip in clips]
        if not clips or any(not clip for clip in clips):
            raise ValueError("avt: no clips, or a clip without frames")
        b, t = len(clips), len(clips[0])
        if any(len(clip) != t for clip in clips):
            raise ValueError("avt: every clip needs the same number of frames")
        for clip in clips:
            if any(f.shape != clip[0].shape for f in clip):
                raise ValueError("avt: the frames of one clip must have the same size")
        first = clips[0][0]
        device = torch.device(device) if device is not None else (
            first.device if first.is_cuda else torch.device("cuda"))
        if device.type != "cuda":
            raise RuntimeError("avt: the clip transform runs on the GPU (no CPU path)")
        if params is None:
            params = [self.params(clip[0].shape[1], clip[0].shape[0], rng) for clip in clips]
        if len(params) != b:
            raise ValueError("avt: one ClipParams per clip")
        train = self.mode == "train"
        s, n = self.size, b * t
        desc = np.zeros((n, 8), dtype=np.int64)
        view2 = np.zeros(b, dtype=_VIEW2)
        off = 0
        for i, (clip, p) in enumerate(zip(clips, params)):
            H, W = clip[0].shape[0], clip[0].shape[1]
            self._check(p, H, W)
            for k in range(t):
                desc[i * t + k] = (off, H, W, p.rh, p.rw, p.crop_top, p.crop_left, int(bool(p.flip)))
                off += H * W * 3
            v = view2[i]
            v["crop_top"], v["crop_left"], v["flip"], v["nops"] = p.crop2_top, p.crop2_left, int(bool(p.flip2)), len(p.ops)
            for o, (kind, f) in enumerate(p.ops):
                v["ops"][o]["kind"], v["ops"][o]["factor"] = kind, f
        hmax = int(desc[:, 1].max())
        src = torch.cat([f.reshape(-1).to(device, non_blocking=True) for clip in clips for f in clip])
        d_desc = torch.from_numpy(desc).to(device)
        d_view2 = torch.from_numpy(view2.view(np.uint8)).to(device) if train else None
        ws_bytes = int(query("avt_clip_workspace_bytes", b, t, s, hmax, int(train)))
        ws = _empty(ws_bytes, torch.uint8, device)
        frames = _empty((b, 3, t, s, s), torch.float32, device)
        augmented = _empty((b, 3, t, s, s), torch.float32, device) if train else None
        with torch.cuda.device(device):
            call("avt_clip_transform", P(src), P(d_desc), P(d_view2) if train else None, b, t, s, hmax, P(ws), ws_bytes,
                 ctypes.cast(self._mean, ctypes.c_void_p), ctypes.cast(self._std, ctypes.c_void_p), P(frames),
                 P(augmented) if train else None, stream_ptr())
        return (frames, augmented) if train else frames


def _as_uint8(f) -> torch.Tensor:
    if not isinstance(f, (torch.Tensor, np.ndarray)):
        if getattr(f, "mode", "RGB") != "RGB":
            f = f.convert("RGB")
        f = np.asarray(f)
    t = torch.as_tensor(f)
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"avt: frames must be uint8 [H, W, 3], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()
