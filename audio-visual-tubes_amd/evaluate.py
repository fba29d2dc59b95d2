"""Localisation evaluation of the reference's test loops on libavt (HIP), batched over heatmaps.

The reference evaluates one heatmap at a time on the host (train_hardway_1frame.py:187-216,
train_hardway.py test loop, test.py:85-172): cv2 resize 14x14 -> 224x224, normalise, median-binarise,
``utils.Evaluator.cal_CIOU(pred, gt, 0.5)``, then cIoU@0.5 and AUC over the test set, and mTC over
consecutive frames.  Here the per-map work runs in one launch for the whole batch of heatmaps
(``avt_localize_ciou``: one block per map, exact median by radix select) straight from the model's
``A`` on the device; the 21-point AUC of the resulting cIoU vector is host arithmetic on N numbers,
as in the reference.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import call
from .trunk import P, stream_ptr

GT_SIZE = 224


def localize(A: torch.Tensor, gt: Optional[torch.Tensor] = None, size: int = GT_SIZE,
             return_maps: bool = False) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """A: heatmaps [N,1,h,w] (AVENet's first output) or [N,h,w] on the GPU; gt: [N,size,size] maps.
    Returns (stats [N,3] fp64 = (cIoU, intersection, denominator) or None without gt,
             binary prediction maps [N,size,size] uint8 if return_maps)."""
    if not A.is_cuda:
        raise RuntimeError("avt: localize runs on the GPU (no CPU path)")
    if A.dim() == 4:
        if A.shape[1] != 1:
            raise ValueError(f"avt: heatmaps must be [N,1,h,w], got {tuple(A.shape)}")
        A = A[:, 0]
    if A.dim() != 3:
        raise ValueError(f"avt: heatmaps must be [N,h,w], got {tuple(A.shape)}")
    N, h, w = A.shape
    if gt is None and not return_maps:
        raise ValueError("avt: localize needs gt maps or return_maps=True")
    A = A.detach().contiguous().float()
    stats = maps = None
    if gt is not None:
        if tuple(gt.shape) != (N, size, size):
            raise ValueError(f"avt: gt must be [{N},{size},{size}], got {tuple(gt.shape)}")
        gt = gt.to(A.device).contiguous().float()
        stats = torch.empty(N, 3, device=A.device, dtype=torch.float64)
    if return_maps:
        maps = torch.empty(N, size, size, device=A.device, dtype=torch.uint8)
    call("avt_localize_ciou", P(A), N, h, w, size, P(gt), P(stats), P(maps), stream_ptr())
    return stats, maps


_HEATMAP_MODES = {"resize": 0, "norm": 1, "pred": -1}


def heatmaps(A: torch.Tensor, size: int = GT_SIZE, mode: str = "norm") -> torch.Tensor:
    """The continuous map ``localize`` binarises, [N,size,size] fp32 on the device, from A [N,1,h,w] or [N,h,w]:
    ``cv2.resize(A[i,0], (size, size), INTER_LINEAR)`` as it is (mode "resize"), ``normalize_img`` of it over its
    own min and max (mode "norm": what test.py:102-111 draws), or ``1 - normalize_img(-resize)`` (mode "pred": the
    value the test loops threshold at its median).  Same arithmetic, bit for bit, as inside ``localize``."""
    if mode not in _HEATMAP_MODES:
        raise ValueError(f"avt: heatmaps mode must be one of {sorted(_HEATMAP_MODES)}, got {mode!r}")
    if not A.is_cuda:
        raise RuntimeError("avt: heatmaps runs on the GPU (no CPU path)")
    if A.dim() == 4:
        if A.shape[1] != 1:
            raise ValueError(f"avt: heatmaps must be [N,1,h,w], got {tuple(A.shape)}")
        A = A[:, 0]
    if A.dim() != 3:
        raise ValueError(f"avt: heatmaps must be [N,h,w], got {tuple(A.shape)}")
    N, h, w = A.shape
    A = A.detach().contiguous().float()
    out = torch.empty(N, size, size, device=A.device, dtype=torch.float32)
    call("avt_heatmap_upsample", P(A), N, h, w, size, _HEATMAP_MODES[mode], P(out), stream_ptr())
    return out


def mtc(pred_maps: torch.Tensor) -> float:
    """utils.mTC (utils.py:311-318): mean cIoU(pred_i, pred_{i+1}, 0.5) over consecutive frames,
    from ``localize(..., return_maps=True)`` maps [T,S,S] of one clip."""
    if pred_maps.shape[0] < 2:
        raise ValueError("avt: mTC needs at least two frames")
    p = pred_maps.contiguous()
    T = p.shape[0]
    out = torch.empty(T - 1, device=p.device, dtype=torch.float64)
    call("avt_pair_ciou", P(p), T, p[0].numel(), P(out), stream_ptr())
    return float(out.sum().item() / (T - 1))


def auc_from_cious(cious: Sequence[float]) -> float:
    """utils.Evaluator.cal_AUC (utils.py:216-225): trapezoid area under the fraction of maps with
    cIoU >= 0.05 i, i = 0..20 (sklearn.metrics.auc of a monotonic x is the trapezoid rule)."""
    c = np.asarray(cious, dtype=np.float64)
    x = np.array([0.05 * i for i in range(21)])
    y = np.array([np.sum(c >= 0.05 * i) / len(c) for i in range(21)])
    return float(np.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2))


class Evaluator:
    """utils.Evaluator (utils.py:203-231): accumulates cIoUs; ``cal_CIOU(infer, gtmap, thres)`` on
    [S,S] maps (numpy or tensors), ``add`` for a localize() batch, ``cal_AUC``, ``final`` (cIoU@0.5)."""

    def __init__(self):
        self.ciou = []

    def cal_CIOU(self, infer, gtmap, thres=0.01):
        infer = torch.as_tensor(infer)
        gtmap = torch.as_tensor(gtmap, device=infer.device).double()
        infer_map = (infer >= thres).double()
        inter = float((infer_map * gtmap).sum())
        denom = float(gtmap.sum() + (infer_map * (gtmap == 0)).sum())
        ciou = inter / denom
        self.ciou.append(ciou)
        return ciou, inter, denom

    def add(self, stats: torch.Tensor):
        self.ciou.extend(stats[:, 0].tolist())

    def cal_AUC(self):
        return auc_from_cious(self.ciou)

    def final(self):
        return float(np.mean(np.array(self.ciou) >= 0.5))

    def clear(self):
        self.ciou = []


def gt_map_flickr(bboxs, size: int = GT_SIZE) -> np.ndarray:
    """utils.testset_gt flickr branch (utils.py:243-263) from the parsed XML boxes [xmin, ymin, xmax,
    ymax] (annotation frame 256 px): boxes scaled to 224, summed, halved, clipped at 1."""
    gt = np.zeros([size, size])
    for b in bboxs:
        x0, y0, x1, y1 = [int(size * int(v) / 256) for v in b]
        gt[y0:y1, x0:x1] += 1
    gt /= 2
    gt[gt > 1] = 1
    return gt


def gt_map_vggss(bboxs, size: int = GT_SIZE) -> np.ndarray:
    """utils.testset_gt vggss branch (utils.py:264-273) from normalised boxes [xmin, ymin, xmax, ymax]."""
    gt = np.zeros([size, size])
    for b in bboxs:
        x0, y0, x1, y1 = [int(size * max(x, 0)) for x in b]
        gt[y0:y1, x0:x1] += 1
    gt[gt > 0] = 1
    return gt


@torch.no_grad()
def evaluate_hardway(model, batches, gt_maps) -> Tuple[float, float]:
    """The test_hardway loop (train_hardway_1frame.py:187-216): eval-mode forward of each (image,
    spec) batch, localisation of every heatmap against its gt map.  ``batches`` yields (image, spec)
    GPU tensors; ``gt_maps`` yields the matching [B,224,224] maps.  Returns (cIoU@0.5, AUC).  The forwards run
    on whatever path the model has enabled: the folded one after ``model.enable_folded_inference()``."""
    was_training = model.training
    model.eval()
    ev = Evaluator()
    try:
        for (image, spec), gt in zip(batches, gt_maps):
            A = model(image.float(), spec.float())[0]
            stats, _ = localize(A, torch.as_tensor(gt))
            ev.add(stats)
    finally:
        model.train(was_training)
    return ev.final(), ev.cal_AUC()


def tube_indices(T: int, sampling_rate: int) -> list:
    """The frames the per-video protocol samples (train_3D.py:152): every sampling_rate-th, the first and last left out."""
    return list(range(sampling_rate, T - 1, sampling_rate))


@torch.no_grad()
def evaluate_tube(model, videos, sampling_rate: int = 16, render_to=None, flow_fn=None) -> dict:
    """The per-video test loop of tube training (train_3D.py:146-186; flow.py:170-210 for AVENet).  ``videos`` yields
    (frames [1,3,T,H,W], spec [1,1,F,Tt], gt [n,224,224]) with one gt map per sampled frame, or (name, frames, spec,
    gt).  Per video: one eval-mode forward of ``frames[:, :, tube_indices(T, sampling_rate)]`` with the one
    spectrogram (``FullModel``, folded if enabled; an ``AVENet`` runs frame by frame, each with that spectrogram),
    ``localize`` of the n heat maps against gt, cIoU@0.5 and the 21-point AUC over those n frames, and mTC over the
    consecutive predictions.  Returns ``dict(ciou=, auc=, mtc=, per_video=[dict(name=, ciou=, auc=, mtc=, cious=)])``,
    the three headline numbers the means over the videos.  A video with fewer than two sampled frames has no mTC:
    ValueError.  ``render_to(name, images)``, when given, receives ``render.overlay(sampled frames, pred=maps, gt=gt)``
    ([n,H,W,3] uint8 on the device) per video; it needs frames of the gt maps' size.  ``flow_fn(name, sampled frames
    [1,3,n,H,W])``, when given, returns the optical flow between the consecutive sampled frames as a field [n-1,S,S,2]
    in pixels of the prediction maps (S = 224); each per-video dict then gains ``mtc_flow``, the flow-compensated mTC
    (``flow.mtc_flow``: frame i's prediction warped onto frame i+1 before the cIoU), and the result its mean over the
    videos.  Without it the result is what it was.

    The reference's tube loop resizes ``heatmap[step][0, 0]`` -- one row of the step-th map (train_3D.py:157-158).
    This is the per-frame protocol every other loop of the reference runs: the whole map of each sampled frame."""
    from .model import AVENet

    per_frame = isinstance(model, AVENet)
    was_training = model.training
    model.eval()
    per_video = []
    try:
        for k, item in enumerate(videos):
            name, frames, spec, gt = item if len(item) == 4 else (k, *item)
            if frames.dim() != 5 or frames.shape[0] != 1:
                raise ValueError(f"avt: evaluate_tube takes one video at a time, frames [1,3,T,H,W], got "
                                 f"{tuple(frames.shape)}")
            idx = tube_indices(frames.shape[2], sampling_rate)
            if len(idx) < 2:
                raise ValueError(f"avt: video {name!r}: {frames.shape[2]} frames at sampling_rate {sampling_rate} give "
                                 f"{len(idx)} sampled frame(s); mTC needs at least two frames")
            sampled = frames[:, :, idx].float()
            spec = spec.float()
            if per_frame:
                A = torch.cat([model(sampled[:, :, j].contiguous(), spec)[0] for j in range(len(idx))])
            else:
                A = model(spec, sampled)[0]
            stats, maps = localize(A, torch.as_tensor(gt), return_maps=True)
            cious = stats[:, 0].tolist()
            per_video.append(dict(name=name, ciou=float(np.mean(np.array(cious) >= 0.5)), auc=auc_from_cious(cious),
                                  mtc=mtc(maps), cious=cious))
            if flow_fn is not None:
                from . import flow

                per_video[-1]["mtc_flow"] = flow.mtc_flow(maps, flow_fn(name, sampled), "pixels")
            if render_to is not None:
                from . import render

                render_to(name, render.overlay(sampled, pred=maps, gt=gt))
    finally:
        model.train(was_training)
    if not per_video:
        raise ValueError("avt: evaluate_tube got no video")
    keys = ("ciou", "auc", "mtc") + (("mtc_flow",) if flow_fn is not None else ())
    out = {k: float(np.sum([v[k] for v in per_video]) / len(per_video)) for k in keys}
    out["per_video"] = per_video
    return out
