"""numpy restatement of the reference's qualitative output and continuous heat map -- TEST INFRASTRUCTURE ONLY.

``save_image_expr`` / ``save_labels_expr`` hold the reference's expressions literally (train_3D.py:73-81,
visualize.py:46-50, flow.py:71-84), one frame at a time, with ``cv2.applyColorMap(x, COLORMAP_JET) := lut[x]`` (cv2 is
not importable here) and the frame's torch ``normalize_img`` taken in numpy fp32 (torch's CPU min, max, subtract and
divide of fp32 are the correctly rounded ones numpy performs).  ``overlay`` is the batched oracle the GPU tests
compare with: the same arithmetic with the weights, scales and layer count of ``avt_render_overlay`` as parameters,
and the two things the kernel defines beyond numpy -- saturation of the final cast and of the table index.

``heatmap`` restates ``avt_heatmap_upsample``'s three modes on ``oracle/eval_oracle.py``'s resize and normalise
(imported, not copied).
"""
import numpy as np

from eval_oracle import cv2_resize_linear, normalize_img


def save_image_expr(image, pred, gt_map, lut):
    """train_3D.py:73-81.  image: [1,3,H,W] float32 (the reference passes a torch tensor; .cpu().numpy() is implied),
    pred / gt_map: [H,W], lut: [256,3] uint8.  Returns what Image.fromarray receives: [H,W,3] uint8."""
    image = normalize_img(image)
    temp = lut[np.uint8(gt_map * 128)]
    temp2 = lut[np.uint8(pred * 255)]
    return np.uint8(np.add((image[0] * 255).transpose((1, 2, 0)) * 0.4, np.add(temp * 0.5, temp2 * 0.5) * 0.6))


def save_labels_expr(image, gt_map, lut):
    """flow.py:80-84."""
    image = normalize_img(image)
    temp = lut[np.uint8(gt_map * 255)]
    return np.uint8(np.add((image[0] * 255).transpose((1, 2, 0)) * 0.5, temp * 0.5))


def frame_term(frame, wimg):
    """[3,H,W] float32 -> [H,W,3] float32: normalize_img over the frame's own min / max, * 255, * wimg."""
    frame = np.asarray(frame, dtype=np.float32)
    image = normalize_img(frame[None])
    return (image[0] * 255).transpose((1, 2, 0)) * np.float32(wimg)


def lut_index(m, scale):
    """uint8(map * scale): fp32 product, truncated; outside [0, 255] clamped (the kernel's definition)."""
    p = np.asarray(m, dtype=np.float32) * np.float32(scale)
    return np.clip(p, 0, 255).astype(np.uint8)


def overlay(frames, lut, layers=(), wimg=0.4, w0=0.6):
    """frames [N,3,H,W] float32, layers: up to two (maps [N,H,W], scale) -> [N,H,W,3] uint8, per frame."""
    out = []
    for i, f in enumerate(np.asarray(frames, dtype=np.float32)):
        a = frame_term(f, wimg)
        assert a.dtype == np.float32
        cs = [lut[lut_index(m[i], s)] for m, s in layers]
        if len(cs) == 2:
            v = np.add(a, np.add(cs[0] * 0.5, cs[1] * 0.5) * float(w0))
        elif len(cs) == 1:
            v = np.add(a, cs[0] * float(w0))
        else:
            v = a
        assert v.dtype == (np.float64 if cs else np.float32)
        out.append(np.clip(v, 0, 255).astype(np.uint8))
    return np.stack(out)


def heatmap(A, size, mode):
    """A [N,h,w] float32 -> [N,size,size] float32: 'resize', 'norm' = normalize_img(resize), 'pred' = 1 -
    normalize_img(-resize) (train_hardway_1frame.py:198-200)."""
    out = []
    for a in np.asarray(A, dtype=np.float32):
        r = cv2_resize_linear(a, size)
        if mode == "norm":
            r = normalize_img(r)
        elif mode == "pred":
            r = 1 - normalize_img(-r)
        else:
            assert mode == "resize"
        assert r.dtype == np.float32
        out.append(r)
    return np.stack(out)


def median_binarize(pred):
    """train_hardway_1frame.py:201-203 on a `pred` map: threshold at the median, pred > thr -> 1, pred < 1 -> 0.
    (Not simply pred > thr: a constant map above 1 has nothing above its median and nothing below 1, and stays.)"""
    pred = np.array(pred, dtype=np.float32)
    threshold = np.sort(pred.flatten())[int(pred.shape[0] * pred.shape[1] / 2)]
    pred[pred > threshold] = 1
    pred[pred < 1] = 0
    return pred


def first_difference(got, ref):
    """The comparator of the GPU tests: None when got and ref are the same bytes, else (count, index, got, ref) of
    the first differing element."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    bad = np.argwhere(got.view(np.uint8 if got.dtype == np.uint8 else np.uint32) !=
                      ref.view(np.uint8 if ref.dtype == np.uint8 else np.uint32))
    if len(bad) == 0:
        return None
    i = tuple(bad[0])
    return len(bad), i, got[i], ref[i]
