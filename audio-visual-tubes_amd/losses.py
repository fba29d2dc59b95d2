"""Drop-ins for the reference's losses.py, computed by libavt (HIP); each gradient is produced in the
forward launch and scaled by the upstream gradient in backward.

* ``PropagationLoss()(heatmap)`` (losses.py:16-23; train_hardway.py:110 ``criterion2``), heatmap
  [b, t, h, w]: mean over (clip, frame pair, pixel) of |heatmap[:, s+1] - heatmap[:, s]|.
* ``NPRatio()(heatmap)`` (losses.py:7-14; train_3D.py:113, 135 ``criterion2``), heatmap [b, t, h, w]:
  mean over (clip, frame pair) of |sum_hw heatmap[:, s+1] - sum_hw heatmap[:, s]|.
* ``FlipLoss()(heatmap, flipped_heatmap)`` (losses.py:25-36): nn.L1Loss()(flipped_heatmap,
  RandomHorizontalFlip(p=1)(heatmap)), the flip along the last dimension.
* ``FlowLoss()(heatmap, field)`` (flow.py:117 ``criterion2 = FlowLoss(14 * 14)``; losses.py of the reference never
  defines it), heatmap [b, t, h, w], field [b, t-1, h, w, 2]: PropagationLoss under flow compensation, the mean over
  (clip, frame pair, pixel) of |warp(heatmap[:, s], field[:, s]) - heatmap[:, s+1]| (``flow.warp``'s bilinear warp).

Each runs on a multi-block grid (no size limit): gradients elementwise, the loss as per-block partial
sums that one block adds in a fixed order (deterministic, run to run).
"""
from __future__ import annotations

import torch
from torch import nn

from ._lib import call, query
from .trunk import P, stream_ptr


def _workspace(x: torch.Tensor, rows: int = 0) -> torch.Tensor:
    """Scratch of the multi-block loss kernels (per-block partial sums, NPRatio's row sums)."""
    return torch.empty(int(query("avt_loss_workspace_floats", x.numel(), rows)), device=x.device, dtype=torch.float32)


class _PropagationLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, heatmap: torch.Tensor):
        if not heatmap.is_cuda:
            raise RuntimeError("avt: PropagationLoss runs on the GPU (no CPU path)")
        if heatmap.dim() != 4:
            raise ValueError(f"avt: PropagationLoss expects [b, t, h, w], got {tuple(heatmap.shape)}")
        b, t, h, w = heatmap.shape
        if t < 2:
            raise ValueError("avt: PropagationLoss needs t >= 2 (the reference's mean over an empty diff is NaN)")
        x = heatmap.detach().contiguous().float()
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        dx = torch.empty_like(x) if heatmap.requires_grad else None
        call("avt_propagation_loss", P(x), b, t, h * w, P(loss), P(dx), P(_workspace(x)), stream_ptr())
        ctx.save_for_backward(dx)
        ctx.in_dtype = heatmap.dtype
        return loss.to(heatmap.dtype)

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return (dx * g).to(ctx.in_dtype)


class PropagationLoss(nn.Module):
    """losses.py:16-23."""

    def forward(self, heatmap: torch.Tensor) -> torch.Tensor:
        return _PropagationLossFn.apply(heatmap)


class _NPRatioFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, heatmap: torch.Tensor):
        if not heatmap.is_cuda:
            raise RuntimeError("avt: NPRatio runs on the GPU (no CPU path)")
        if heatmap.dim() != 4:
            raise ValueError(f"avt: NPRatio expects [b, t, h, w], got {tuple(heatmap.shape)}")
        b, t, h, w = heatmap.shape
        if t < 2:
            raise ValueError("avt: NPRatio needs t >= 2 (the reference's mean over an empty diff is NaN)")
        x = heatmap.detach().contiguous().float()
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        dx = torch.empty_like(x) if heatmap.requires_grad else None
        call("avt_npratio_loss", P(x), b, t, h * w, P(loss), P(dx), P(_workspace(x, b * t)), stream_ptr())
        ctx.save_for_backward(dx)
        ctx.in_dtype = heatmap.dtype
        return loss.to(heatmap.dtype)

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return (dx * g).to(ctx.in_dtype)


class NPRatio(nn.Module):
    """losses.py:7-14 (Negative / Positive Ratio Loss)."""

    def forward(self, heatmap: torch.Tensor) -> torch.Tensor:
        return _NPRatioFn.apply(heatmap)


class _FlipLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, heatmap: torch.Tensor, flipped: torch.Tensor):
        if not heatmap.is_cuda or not flipped.is_cuda:
            raise RuntimeError("avt: FlipLoss runs on the GPU (no CPU path)")
        if heatmap.shape != flipped.shape or heatmap.dim() < 1:
            raise ValueError(f"avt: FlipLoss needs two tensors of one shape, got {tuple(heatmap.shape)} and "
                             f"{tuple(flipped.shape)}")
        if heatmap.numel() == 0:
            raise ValueError(f"avt: FlipLoss of an empty tensor {tuple(heatmap.shape)} (the reference's mean over "
                             "no elements is NaN)")
        x = heatmap.detach().contiguous().float()
        y = flipped.detach().contiguous().float()
        W = x.shape[-1]
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        dx = torch.empty_like(x) if heatmap.requires_grad else None
        dy = torch.empty_like(y) if flipped.requires_grad else None
        call("avt_flip_l1_loss", P(x), P(y), x.numel() // W, W, P(loss), P(dx), P(dy), P(_workspace(x)), stream_ptr())
        ctx.save_for_backward(dx, dy)
        ctx.dtypes = (heatmap.dtype, flipped.dtype)
        return loss.to(flipped.dtype)

    @staticmethod
    def backward(ctx, g):
        dx, dy = ctx.saved_tensors
        return (None if dx is None else (dx * g).to(ctx.dtypes[0]),
                None if dy is None else (dy * g).to(ctx.dtypes[1]))


class FlipLoss(nn.Module):
    """losses.py:25-36: L1 between flipped_heatmap and the horizontally flipped heatmap."""

    def forward(self, heatmap: torch.Tensor, flipped_heatmap: torch.Tensor) -> torch.Tensor:
        return _FlipLossFn.apply(heatmap, flipped_heatmap)


class _FlowLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, heatmap: torch.Tensor, field: torch.Tensor, coords: int):
        if not heatmap.is_cuda or not field.is_cuda:
            raise RuntimeError("avt: FlowLoss runs on the GPU (no CPU path)")
        if heatmap.dim() != 4:
            raise ValueError(f"avt: FlowLoss expects a heatmap [b, t, h, w], got {tuple(heatmap.shape)}")
        b, t, h, w = heatmap.shape
        if t < 2:
            raise ValueError("avt: FlowLoss needs t >= 2 (there is no frame pair to compare)")
        if b < 1 or h * w < 1 or h * w > 1024:
            raise ValueError(f"avt: FlowLoss takes b >= 1 maps of 1 <= h*w <= 1024 pixels, got {tuple(heatmap.shape)}")
        if tuple(field.shape) != (b, t - 1, h, w, 2):
            raise ValueError(f"avt: FlowLoss expects a field [{b}, {t - 1}, {h}, {w}, 2], got {tuple(field.shape)}")
        if field.requires_grad:
            raise ValueError("avt: FlowLoss gives the field no gradient (the flow estimator is frozen, flow.py:107); "
                             "pass field.detach()")
        x = heatmap.detach().contiguous().float()
        f = field.contiguous().float()
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        dx = torch.empty_like(x) if heatmap.requires_grad else None
        call("avt_flow_loss", P(x), b, t, h, w, P(f), coords, P(loss), P(dx), P(_workspace(x, b * t)), stream_ptr())
        ctx.save_for_backward(dx)
        ctx.in_dtype = heatmap.dtype
        return loss.to(heatmap.dtype)

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return (dx * g).to(ctx.in_dtype), None, None


class FlowLoss(nn.Module):
    """The ``FlowLoss`` flow.py:117 constructs.  ``coords`` as in ``flow.warp`` ("pixels": displacements in pixels of
    the heat map; "grid": grid_sample coordinates).  The reference's one positional argument (``FlowLoss(14 * 14)``,
    the number of pixels) is accepted and not used: the maps carry their own size."""

    def __init__(self, n_pixels=None, *, coords: str = "pixels"):
        super().__init__()
        from .flow import coords_id

        self.coords = coords
        self._coords_id = coords_id(coords)

    def forward(self, heatmap: torch.Tensor, field: torch.Tensor) -> torch.Tensor:
        return _FlowLossFn.apply(heatmap, field, self._coords_id)
