"""CPU: the oracle of the render and heat-map kernels (tests/render_oracle.py) against the reference's literal
expressions, numpy's dtypes along the way, the checkable properties of render.JET, evaluate_tube's sampling and
averaging on a hand-worked example, and the comparator's power against four injected faults."""
import numpy as np
import pytest
import torch

import eval_oracle as evo
import render_oracle as ro
from avt_amd import evaluate as ev
from avt_amd import render


def _inputs(seed, N=3, H=9, W=11):
    rng = np.random.default_rng(seed)
    frames = (rng.standard_normal((N, 3, H, W)) * rng.uniform(0.5, 3.0, (N, 1, 1, 1)) +
              rng.uniform(-2, 2, (N, 1, 1, 1))).astype(np.float32)
    pred = (rng.random((N, H, W)) < 0.5).astype(np.float32)
    gt = rng.choice([0.0, 0.5, 1.0], (N, H, W)).astype(np.float32)
    cont = rng.random((N, H, W)).astype(np.float32)
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    return frames, pred, gt, cont, lut


def test_oracle_equals_the_literal_expressions():
    frames, pred, gt, cont, lut = _inputs(1)
    both = ro.overlay(frames, lut, [(gt, 128), (pred, 255)], wimg=0.4, w0=0.6)
    both_cont = ro.overlay(frames, lut, [(gt, 128), (cont, 255)], wimg=0.4, w0=0.6)
    lab = ro.overlay(frames, lut, [(cont, 255)], wimg=0.5, w0=0.5)
    for i in range(len(frames)):
        np.testing.assert_array_equal(both[i], ro.save_image_expr(frames[i:i + 1], pred[i], gt[i], lut))
        np.testing.assert_array_equal(both_cont[i], ro.save_image_expr(frames[i:i + 1], cont[i], gt[i], lut))
        np.testing.assert_array_equal(lab[i], ro.save_labels_expr(frames[i:i + 1], cont[i], lut))
    # the two layers' halves add exactly, so their order is free
    np.testing.assert_array_equal(both, ro.overlay(frames, lut, [(pred, 255), (gt, 128)], wimg=0.4, w0=0.6))
    # torch's normalize_img of the reference (a tensor goes in) is numpy's, bit for bit
    t = torch.from_numpy(frames[:1])
    tn = ((t - t.min()) / (t.max() - t.min())).numpy()
    np.testing.assert_array_equal(tn, evo.normalize_img(frames[:1]))


def test_numpy_keeps_the_frame_term_fp32_and_the_sum_fp64():
    frames, pred, gt, _, lut = _inputs(2)
    image = evo.normalize_img(frames[:1])
    assert image.dtype == np.float32
    a = (image[0] * 255).transpose((1, 2, 0)) * 0.4
    assert a.dtype == np.float32
    np.testing.assert_array_equal(a, (image[0] * np.float32(255)).transpose((1, 2, 0)) * np.float32(0.4))
    np.testing.assert_array_equal(a, ro.frame_term(frames[0], 0.4))
    temp = lut[np.uint8(gt[0] * 128)]
    assert (gt[0] * 128).dtype == np.float32 and temp.dtype == np.uint8 and temp.shape == a.shape
    c = np.add(temp * 0.5, lut[np.uint8(pred[0] * 255)] * 0.5) * 0.6
    assert c.dtype == np.float64
    s = np.add(a, c)
    assert s.dtype == np.float64
    np.testing.assert_array_equal(s, a.astype(np.float64) + c)
    # np.uint8 truncates
    np.testing.assert_array_equal(np.uint8(np.array([0.999, 1.0, 254.999, 255.0])), [0, 1, 254, 255])
    np.testing.assert_array_equal(ro.lut_index(np.float32([0, 1, 0.999, -1, 2, 127.999 / 128]), 128), [0, 128, 127, 0, 255, 127])


def test_heatmap_oracle_is_the_protocol():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((2, 7, 9)).astype(np.float32)
    A[1] = 0.25
    for S in (16, 33):
        pred = ro.heatmap(A, S, "pred")
        norm = ro.heatmap(A, S, "norm")
        for i in range(2):
            np.testing.assert_array_equal(ro.median_binarize(pred[i]), evo.binarize(A[i], S))
        assert norm[0].min() == 0 and norm[0].max() == 1
        np.testing.assert_array_equal(norm[1], np.full((S, S), 0.25, np.float32))  # constant: left as it is
        np.testing.assert_array_equal(pred[1], np.full((S, S), 1.25, np.float32))


def test_jet_table():
    t = render.JET
    assert tuple(t.shape) == (256, 3) and t.dtype == torch.uint8 and not t.is_cuda
    assert t[0].tolist() == [128, 0, 0] and t[255].tolist() == [0, 0, 128]  # BGR: dark blue ... dark red
    j = t.numpy().astype(int)
    assert (j[:, 1].argmax() > 64) and (j[:, 1].max() == 255) and j[128, 1] == 255   # green in the middle
    assert (np.diff(j[:96, 0]) >= 0).all() and (np.diff(j[96:, 0]) <= 0).all()       # blue up, then down
    assert (np.diff(j[:160, 2]) >= 0).all() and (np.diff(j[160:, 2]) <= 0).all()     # red up, then down
    assert np.abs(np.diff(j, axis=0)).max() <= 4
    with pytest.raises(ValueError, match="colour table"):
        render._device_lut(torch.zeros(255, 3, dtype=torch.uint8), "cpu")


class _FakeModel:
    """FullModel's call convention: model(spec, frames) -> (A, logits), A [t,1,2,2]."""

    def __init__(self):
        self.training = True
        self.calls = []

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode

    def __call__(self, spec, frames):
        assert not self.training
        self.calls.append(frames[0, 0, :, 0, 0].tolist())  # each frame carries its index
        return torch.zeros(frames.shape[2], 1, 2, 2), None


def test_evaluate_tube_indices_and_averaging(monkeypatch):
    """Three videos, sampling_rate 4.  Stubbed localize: frame j of video k has the cIoU listed below; stubbed mtc.
      video 0: T = 13 -> frames 4, 8        cIoUs .5, .2          cIoU@.5 = 1/2
      video 1: T = 14 -> frames 4, 8, 12    cIoUs .9, .6, .1      cIoU@.5 = 2/3
      video 2: T = 21 -> frames 4 .. 16     cIoUs 1, 0, .3, .49   cIoU@.5 = 1/4
    The AUC is the trapezoid area under the fraction of frames with cIoU >= threshold, thresholds 0, .05 .. 1."""
    assert ev.tube_indices(13, 4) == [4, 8] and ev.tube_indices(14, 4) == [4, 8, 12]
    assert ev.tube_indices(21, 4) == [4, 8, 12, 16] and ev.tube_indices(17, 16) == [] and ev.tube_indices(18, 16) == [16]
    assert ev.tube_indices(300, 16) == list(range(16, 299, 16))
    cious = [[0.5, 0.2], [0.9, 0.6, 0.1], [1.0, 0.0, 0.3, 0.49]]
    mtcs = [0.25, 0.5, 1.0]
    state = {"k": -1}

    def fake_localize(A, gt, size=224, return_maps=False):
        state["k"] += 1
        c = cious[state["k"]]
        assert A.shape[0] == len(c) == gt.shape[0] and return_maps
        stats = torch.tensor([[v, 0.0, 0.0] for v in c], dtype=torch.float64)
        return stats, torch.full((len(c), 2, 2), state["k"], dtype=torch.uint8)

    def fake_mtc(maps):
        return mtcs[int(maps[0, 0, 0])]

    monkeypatch.setattr(ev, "localize", fake_localize)
    monkeypatch.setattr(ev, "mtc", fake_mtc)

    def video(T, n):
        frames = torch.arange(T, dtype=torch.float32).view(1, 1, T, 1, 1).expand(1, 3, T, 2, 2)
        return frames, torch.zeros(1, 1, 5, 5), torch.zeros(n, 224, 224)

    model = _FakeModel()
    res = ev.evaluate_tube(model, [video(13, 2), video(14, 3), video(21, 4)], sampling_rate=4)
    assert model.calls == [[4, 8], [4, 8, 12], [4, 8, 12, 16]]
    assert model.training is True
    assert [v["cious"] for v in res["per_video"]] == cious
    assert [v["ciou"] for v in res["per_video"]] == [1 / 2, 2 / 3, 1 / 4]
    assert [v["mtc"] for v in res["per_video"]] == mtcs

    def auc_by_hand(cs):
        x = [0.05 * i for i in range(21)]
        y = [sum(c >= 0.05 * i for c in cs) / len(cs) for i in range(21)]
        return sum((x[i + 1] - x[i]) * (y[i + 1] + y[i]) / 2 for i in range(20))

    aucs = [auc_by_hand(c) for c in cious]
    # video 0 by hand: both frames up to .2 (4 intervals of 1), one frame up to .5 (6 of 1/2), the step intervals
    # averaging their ends: .05 (4 + (1 + .5) / 2 + 5 * .5 + (.5 + 0) / 2) = .05 * 7.5
    assert abs(aucs[0] - 0.05 * 7.5) < 1e-12
    for v, a, c in zip(res["per_video"], aucs, cious):
        assert abs(v["auc"] - a) < 1e-12 and abs(v["auc"] - evo.cal_auc(c)) < 1e-12
    assert abs(res["ciou"] - (1 / 2 + 2 / 3 + 1 / 4) / 3) < 1e-15
    assert abs(res["auc"] - sum(aucs) / 3) < 1e-15
    assert abs(res["mtc"] - (0.25 + 0.5 + 1.0) / 3) < 1e-15
    # mean over videos, not over frames
    assert abs(res["ciou"] - np.mean(np.concatenate(cious) >= 0.5)) > 1e-3

    # fewer than two sampled frames: no mTC
    state["k"] = -1
    model = _FakeModel()
    model.training = False
    with pytest.raises(ValueError, match="at least two frames"):
        ev.evaluate_tube(model, [video(9, 1)], sampling_rate=4)   # range(4, 8, 4) = [4]
    assert model.training is False and model.calls == []
    with pytest.raises(ValueError, match="one video at a time"):
        ev.evaluate_tube(model, [(torch.zeros(2, 3, 13, 2, 2), torch.zeros(2, 1, 5, 5), torch.zeros(2, 224, 224))], 4)


# ---- the comparator against four injected faults ---------------------------------------------------------------
def _fault_inputs():
    rng = np.random.default_rng(7)
    N, H, W = 3, 17, 33
    frames = rng.standard_normal((N, 3, H, W)).astype(np.float32)
    frames[1] = frames[1] * 4 + 3        # another range per frame
    frames[2] = -1.5                      # a constant frame
    m = rng.random((N, H, W)).astype(np.float32)
    m.flat[::7] = np.float32((np.arange(m.size)[::7] % 255 + 0.75) / 255)   # products whose fraction is >= .5
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    return frames, m, lut


def test_comparator_flags_injected_faults():
    frames, m, lut = _fault_inputs()
    ref = ro.overlay(frames, lut, [(m, 255)], wimg=0.5, w0=0.5)
    assert ro.first_difference(ref.copy(), ref) is None

    # 1. min and max over the batch instead of the frame
    g = evo.normalize_img(frames)
    batch = np.stack([np.clip(np.add((g[i] * 255).transpose(1, 2, 0) * np.float32(0.5), lut[ro.lut_index(m[i], 255)] * 0.5),
                              0, 255).astype(np.uint8) for i in range(len(frames))])
    assert ro.first_difference(batch, ref) is not None

    # 2. idx rounded instead of truncated
    rounded = np.stack([np.clip(np.add(ro.frame_term(frames[i], 0.5),
                                       lut[np.rint(m[i] * np.float32(255)).astype(np.uint8)] * 0.5), 0, 255).astype(np.uint8)
                        for i in range(len(frames))])
    assert ro.first_difference(rounded, ref) is not None

    # 3. the table's channels swapped (BGR -> RGB)
    assert ro.first_difference(ro.overlay(frames, lut[:, ::-1], [(m, 255)], wimg=0.5, w0=0.5), ref) is not None
    #    ... and the frame's
    assert ro.first_difference(ro.overlay(frames[:, ::-1], lut, [(m, 255)], wimg=0.5, w0=0.5), ref) is not None

    # 4. the constant branch normalising anyway: the constant frame -1.5 would become 0 (or NaN), here it stays -1.5
    forced = ref.copy()
    forced[2] = np.clip(lut[ro.lut_index(m[2], 255)] * 0.5, 0, 255).astype(np.uint8)  # frame term 0 instead of -1.5*255*.5
    assert ro.first_difference(forced, ref) is not None
    #    and for the heat map: a constant map normalised anyway is 0 / 0
    A = np.full((1, 3, 3), 0.25, np.float32)
    href = ro.heatmap(A, 8, "norm")
    assert ro.first_difference(np.zeros_like(href), href) is not None
    assert ro.first_difference(href.copy(), href) is None
