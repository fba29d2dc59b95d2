"""Flow-compensated temporal consistency on libavt (HIP): everything of the reference's ``flow.py`` that lies
downstream of "an optical-flow field exists".

After the hard-way forward, ``flow.py`` takes a flow field per consecutive frame pair, warps frame t's prediction onto
frame t+1 with ``grid_sample(..., mode='bilinear')`` (flow.py:152-153) and draws the field with ``utils.flow2img``
(flow.py:157); it cites the metric it is after, the flow-compensated consistency of consecutive predictions.  The
estimator itself (FlowNet2) is not vendored by the reference and is not part of this package: every function here
takes the field as a tensor.

* ``warp(maps, field, coords)``: the bilinear warp, ``avt_flow_warp``.
* ``consistency(pred_maps, field, coords)`` / ``mtc_flow(...)``: ``evaluate.mtc`` with frame t's map warped onto
  frame t+1 first, in one pass that never stores the warped map (``avt_flow_consistency``).
* ``flow_to_image(field)``: ``utils.flow2img`` per field, uint8 HWC on the device (``avt_flow_color``).
* ``read_flo`` / ``write_flo``: the Middlebury ``.flo`` file format (utils.py:14-63), on the host.
* the trainable form is ``losses.FlowLoss``.

``coords="grid"`` reads the field as ``grid_sample`` coordinates (align_corners=False) -- flow.py:152 to the letter,
which hands FlowNet2's pixel displacements to ``grid_sample`` unconverted; ``coords="pixels"`` reads it as
displacements (u, v) = (dx, dy) in pixels of the map, channel 0 horizontal, which is what the cited metric means.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import call, query
from .trunk import P, stream_ptr

COORDS = {"grid": 0, "pixels": 1}
FLO_MAGIC = 202021.25


def coords_id(coords: str) -> int:
    if coords not in COORDS:
        raise ValueError(f"avt: coords must be one of {sorted(COORDS)}, got {coords!r}")
    return COORDS[coords]


def _gpu(t: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"avt: {what} runs on the GPU (no CPU path)")


def _field(field: torch.Tensor, lead: tuple, what: str) -> torch.Tensor:
    """an fp32 contiguous field whose leading dimensions are ``lead`` and whose last is 2"""
    if field.dim() != len(lead) + 3 or field.shape[-1] != 2 or tuple(field.shape[:len(lead)]) != lead \
            or field.shape[-2] < 1 or field.shape[-3] < 1:
        raise ValueError(f"avt: {what} takes a field [{', '.join(map(str, lead))}, H, W, 2], got {tuple(field.shape)}")
    return field.detach().contiguous().float()


def _workspace(maps: int, pixels: int, device) -> torch.Tensor:
    return torch.empty(int(query("avt_flow_workspace_bytes", maps, pixels)) // 8, device=device, dtype=torch.float64)


def warp(maps: torch.Tensor, field: torch.Tensor, coords: str = "grid") -> torch.Tensor:
    """maps [N,H,W] or [N,1,H,W] (fp32, or uint8 read as 0 / 1) warped by field [N,Ho,Wo,2]: with "grid",
    ``grid_sample(maps, field, mode='bilinear', padding_mode='zeros', align_corners=False)`` (flow.py:152), output
    [N,Ho,Wo]; with "pixels", out[n,y,x] = maps[n] sampled bilinearly at (x + field[n,y,x,0], y + field[n,y,x,1]),
    the field of the maps' size.  Returns fp32 of the maps' rank."""
    cid = coords_id(coords)
    _gpu(maps, "warp")
    _gpu(field, "warp")
    four = maps.dim() == 4
    if four:
        if maps.shape[1] != 1:
            raise ValueError(f"avt: maps must be [N,H,W] or [N,1,H,W], got {tuple(maps.shape)}")
        maps = maps[:, 0]
    if maps.dim() != 3 or min(maps.shape) < 1:
        raise ValueError(f"avt: maps must be [N,H,W] or [N,1,H,W], got {tuple(maps.shape)}")
    N, H, W = maps.shape
    f = _field(field, (N,), "warp")
    Ho, Wo = f.shape[1:3]
    if cid == 1 and (Ho, Wo) != (H, W):
        raise ValueError(f"avt: pixel displacements need a field of the maps' size [{N},{H},{W},2], got "
                         f"{tuple(field.shape)}")
    u8 = maps.dtype in (torch.uint8, torch.bool)
    m = maps.detach().contiguous()
    m = m.view(torch.uint8) if maps.dtype == torch.bool else (m if u8 else m.float())
    out = torch.empty(N, Ho, Wo, device=m.device, dtype=torch.float32)
    call("avt_flow_warp", P(m), int(u8), N, H, W, P(f), Ho, Wo, cid, P(out), stream_ptr())
    return out[:, None] if four else out


def consistency(pred_maps: torch.Tensor, field: torch.Tensor, coords: str = "pixels") -> torch.Tensor:
    """pred_maps [T,S,S] uint8 (``localize(..., return_maps=True)``), field [T-1,S,S,2]: per consecutive pair k,
    ``cal_CIOU(warp(pred[k]), pred[k+1], 0.5)`` as (cIoU, intersection, denominator), [T-1,3] fp64 on the device."""
    cid = coords_id(coords)
    _gpu(pred_maps, "consistency")
    _gpu(field, "consistency")
    if pred_maps.dim() != 3 or pred_maps.shape[1] != pred_maps.shape[2] or pred_maps.shape[1] < 1 \
            or pred_maps.dtype != torch.uint8:
        raise ValueError(f"avt: consistency takes uint8 maps [T,S,S], got {tuple(pred_maps.shape)} {pred_maps.dtype}")
    T, S, _ = pred_maps.shape
    if T < 2:
        raise ValueError("avt: consistency needs at least two frames")
    f = _field(field, (T - 1,), "consistency")
    if tuple(f.shape[1:3]) != (S, S):
        raise ValueError(f"avt: consistency takes a field [{T - 1},{S},{S},2], got {tuple(field.shape)}")
    p = pred_maps.contiguous()
    out = torch.empty(T - 1, 3, device=p.device, dtype=torch.float64)
    call("avt_flow_consistency", P(p), T, S, P(f), cid, P(out), P(_workspace(T - 1, S * S, p.device)), stream_ptr())
    return out


def mtc_flow(pred_maps: torch.Tensor, field: torch.Tensor, coords: str = "pixels") -> float:
    """``evaluate.mtc`` under flow compensation: the mean over consecutive frames of cIoU(warp(pred_i), pred_{i+1},
    0.5).  With a zero field in pixel coordinates it is ``evaluate.mtc(pred_maps)``."""
    out = consistency(pred_maps, field, coords)
    return float(out[:, 0].sum().item() / out.shape[0])


def _color_wheel() -> torch.Tensor:
    """The Middlebury colour wheel (utils.make_color_wheel, utils.py:64-111): 55 colours in six segments of 15, 6, 4,
    11, 13 and 6 steps -- red to yellow, yellow to green, green to cyan, cyan to blue, blue to magenta, magenta to red
    -- one channel ramping by floor(255 i / length) up or down while another stays at 255.  Integers: uint8 [55,3]."""
    rows = []
    # (length, channel held at 255, channel ramping, ramp rises?)
    for length, held, ramp, rises in ((15, 0, 1, True), (6, 1, 0, False), (4, 1, 2, True), (11, 2, 1, False),
                                      (13, 2, 0, True), (6, 0, 2, False)):
        for i in range(length):
            rgb = [0, 0, 0]
            rgb[held] = 255
            step = (255 * i) // length
            rgb[ramp] = step if rises else 255 - step
            rows.append(rgb)
    return torch.tensor(rows, dtype=torch.uint8)


#: [55,3] uint8, RGB
WHEEL = _color_wheel()
_WHEEL_ON = {}  # device -> WHEEL's copy there


def flow_to_image(field: torch.Tensor) -> torch.Tensor:
    """``utils.flow2img`` (utils.py:155-192) of field [N,H,W,2] or [H,W,2] on the GPU: uint8 [N,H,W,3] or [H,W,3] on
    the device, RGB, the layout ``render.overlay`` returns.  The field is left as it is (the reference overwrites
    its argument)."""
    _gpu(field, "flow_to_image")
    one = field.dim() == 3
    f = field[None] if one else field
    if f.dim() != 4 or f.shape[-1] != 2 or min(f.shape) < 1:
        raise ValueError(f"avt: flow_to_image takes a field [N,H,W,2] or [H,W,2], got {tuple(field.shape)}")
    f = f.detach().contiguous().float()
    N, H, W, _ = f.shape
    if f.device not in _WHEEL_ON:
        _WHEEL_ON[f.device] = WHEEL.to(f.device)
    out = torch.empty(N, H, W, 3, device=f.device, dtype=torch.uint8)
    call("avt_flow_color", P(f), N, H, W, P(_WHEEL_ON[f.device]), P(out), P(_workspace(N, H * W, f.device)),
         stream_ptr())
    return out[0] if one else out


def read_flo(path) -> np.ndarray:
    """utils.readFlow (utils.py:14-33): a Middlebury ``.flo`` file as float32 [h,w,2].  A wrong magic number or a
    short file raises ValueError (the reference prints a line and returns None)."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 12 or np.frombuffer(raw, "<f4", 1)[0] != np.float32(FLO_MAGIC):
        raise ValueError(f"avt: {path}: not a .flo file (the magic number {FLO_MAGIC} is missing)")
    w, h = (int(v) for v in np.frombuffer(raw, "<i4", 2, 4))
    if w < 1 or h < 1 or len(raw) < 12 + 8 * w * h:
        raise ValueError(f"avt: {path}: a {w} x {h} .flo file needs {12 + 8 * w * h} bytes, has {len(raw)}")
    return np.frombuffer(raw, "<f4", 2 * w * h, 12).reshape(h, w, 2).copy()


def write_flo(path, uv, v=None) -> None:
    """utils.writeFlow (utils.py:34-63): uv [h,w,2], or u and v [h,w] each, as a Middlebury ``.flo`` file: the magic
    number 202021.25 as float32, int32 width, int32 height, then the rows of interleaved (u, v) float32, little
    endian.  The same bytes the reference's writer gives for the same arrays."""
    uv = uv.detach().cpu().numpy() if isinstance(uv, torch.Tensor) else np.asarray(uv)
    if v is None:
        if uv.ndim != 3 or uv.shape[2] != 2:
            raise ValueError(f"avt: write_flo takes uv [h,w,2] or u, v [h,w], got {uv.shape}")
        u, v = uv[:, :, 0], uv[:, :, 1]
    else:
        u = uv
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    if u.ndim != 2 or u.shape != v.shape:
        raise ValueError(f"avt: write_flo takes u and v of one shape [h,w], got {u.shape} and {v.shape}")
    h, w = u.shape
    with open(path, "wb") as f:
        f.write(np.array([FLO_MAGIC], "<f4").tobytes())
        f.write(np.array([w, h], "<i4").tobytes())
        f.write(np.stack([u, v], axis=2).astype("<f4").tobytes())
