"""The reference's qualitative output on libavt (HIP): frames blended with colour-mapped maps, uint8 HWC on the device.

Every reference entry script carries ``save_image`` (visualize.py:46-50, train_3D.py:73-81, flow.py:71-79) or
``save_labels`` (flow.py:80-84): min-max normalise the frame, colour-map the ground-truth map and the binarised
prediction with ``cv2.applyColorMap(..., COLORMAP_JET)``, blend, cast to uint8 -- one frame at a time on the host.
``overlay`` does it for a batch of frames in one launch (``avt_render_overlay``, one block per frame) and returns the
bytes numpy 2.x gives for the reference's own expression, with ``applyColorMap(x) := lut[x]``.  Two things are ours:
sums outside [0, 255] saturate (numpy's cast of them is undefined), and a scaled map value outside [0, 255] is clamped.

As in the reference, channel ``ch`` of the table is added to channel ``ch`` of the frame: ``cv2.applyColorMap``
returns BGR and the frame is RGB, so in the reference's pictures the jet colours are mirrored (a hot pixel adds blue).
``JET`` keeps cv2's BGR order so that the defaults reproduce that; pass ``lut=JET.flip(1)`` for the usual colours.

Encoding (JPEG, MP4) and logging are the caller's: the result is a device uint8 [N,H,W,3] tensor.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from ._lib import call
from .trunk import P, stream_ptr


def _jet_table() -> torch.Tensor:
    """COLORMAP_JET as OpenCV publishes it: 256 samples at x = i / 255 of the piecewise-linear jet
    r, g, b = clamp(1.5 - |4x - k|, 0, 1), k = 3, 2, 1, scaled by 255 and rounded half to even (cv2's saturate_cast),
    stored in cv2's BGR order.  Evaluated in integers (every unrounded value is a multiple of 0.5)."""
    rows = []
    for i in range(256):
        bgr = []
        for k in (1, 2, 3):  # b, g, r
            twice = min(max(765 - 2 * abs(4 * i - 255 * k), 0), 510)  # 2 * 255 * clamp(1.5 - |4 i / 255 - k|)
            v = twice // 2
            if twice % 2 and v % 2:  # x.5: to the even neighbour
                v += 1
            bgr.append(v)
        rows.append(bgr)
    return torch.tensor(rows, dtype=torch.uint8)


#: [256,3] uint8, BGR.  cv2 is not available where this package is developed, so the table is NOT pinned against
#: ``cv2.applyColorMap`` itself: it is built from OpenCV's published definition of the map, and cv2's own float table
#: may round an entry the other way.  What is checked: shape, dtype, dark blue (128, 0, 0) at 0 and dark red
#: (0, 0, 128) at 255 in BGR order.  The kernel takes any table; its tests use random ones.
JET = _jet_table()

_JET_ON = {}  # device -> JET's copy there


def _device_lut(lut: torch.Tensor, device) -> torch.Tensor:
    if tuple(lut.shape) != (256, 3) or lut.dtype != torch.uint8:
        raise ValueError(f"avt: a colour table is [256,3] uint8, got {tuple(lut.shape)} {lut.dtype}")
    if lut is JET:
        if device not in _JET_ON:
            _JET_ON[device] = JET.to(device)
        return _JET_ON[device]
    return lut.to(device).contiguous()


def _fold_frames(frames: torch.Tensor) -> torch.Tensor:
    if not frames.is_cuda:
        raise RuntimeError("avt: overlay runs on the GPU (no CPU path)")
    if frames.dim() == 5:  # [b,3,t,H,W] -> [(b t),3,H,W], as the model folds it
        if frames.shape[1] != 3:
            raise ValueError(f"avt: frames must be [b,3,t,H,W], got {tuple(frames.shape)}")
        b, _, t, H, W = frames.shape
        frames = frames.permute(0, 2, 1, 3, 4).reshape(b * t, 3, H, W)
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError(f"avt: frames must be [N,3,H,W] or [b,3,t,H,W], got {tuple(frames.shape)}")
    return frames.detach().contiguous().float()


def _layer(m: Optional[torch.Tensor], name: str, N: int, H: int, W: int, device) -> Optional[torch.Tensor]:
    if m is None:
        return None
    m = torch.as_tensor(m)
    if m.dim() == 4 and m.shape[1] == 1:
        m = m[:, 0]
    if tuple(m.shape) != (N, H, W):
        raise ValueError(f"avt: {name} must be [{N},{H},{W}], got {tuple(m.shape)}")
    return m.detach().to(device).contiguous().float()


def overlay(frames: torch.Tensor, pred: Optional[torch.Tensor] = None, gt: Optional[torch.Tensor] = None, *,
            pred_scale: float = 255, gt_scale: float = 128, image_weight: float = 0.4, overlay_weight: float = 0.6,
            lut: torch.Tensor = JET) -> torch.Tensor:
    """frames [N,3,H,W] (or [b,3,t,H,W], folded to (b t)): the network's normalised frames on the GPU; pred, gt:
    [N,H,W] maps in [0, 1] (any dtype: ``localize``'s uint8 maps, ``heatmaps``' fp32 ones) or None.  Returns
    [N,H,W,3] uint8 on the device.  With both maps and the defaults this is ``save_image(frame, _, pred, gt)`` for
    every frame: ``uint8(normalize_img(frame) * 255 * 0.4 + (lut[uint8(gt * 128)] * 0.5 + lut[uint8(pred * 255)] * 0.5)
    * 0.6)``; with one map, ``uint8(frame term + lut[uint8(map * scale)] * overlay_weight)``; with none, the frame
    term alone."""
    x = _fold_frames(frames)
    N, _, H, W = x.shape
    layers = [(m, float(s)) for m, s in ((_layer(gt, "gt", N, H, W, x.device), gt_scale),
                                         (_layer(pred, "pred", N, H, W, x.device), pred_scale)) if m is not None]
    (m0, s0), (m1, s1) = (layers + [(None, 0.0), (None, 0.0)])[:2]
    table = _device_lut(lut, x.device) if layers else None
    out = torch.empty(N, H, W, 3, device=x.device, dtype=torch.uint8)
    call("avt_render_overlay", P(x), N, H, W, P(m0), ctypes.c_float(s0), ctypes.c_double(overlay_weight), P(m1),
         ctypes.c_float(s1), ctypes.c_double(0.0), ctypes.c_float(image_weight), P(table), P(out), stream_ptr())
    return out


def labels(frames: torch.Tensor, gt: torch.Tensor, *, lut: torch.Tensor = JET) -> torch.Tensor:
    """``save_labels(frame, _, gt)`` (flow.py:80-84) for every frame:
    ``uint8(normalize_img(frame) * 255 * 0.5 + lut[uint8(gt * 255)] * 0.5)``."""
    return overlay(frames, gt=gt, gt_scale=255, image_weight=0.5, overlay_weight=0.5, lut=lut)
