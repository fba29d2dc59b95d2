"""evaluate.evaluate_tube: the per-video test protocol of tube training (train_3D.py:146-186, flow.py:170-210) on a
seeded FullModel / AVENet, against oracle/eval_oracle.py run on the host over the model's own heat maps.

Two videos of 32 x 32 frames (the smallest size test_tube_gpu.py runs the tube at) whose sampled frame counts differ
(2 and 5 at sampling_rate 2), box-shaped ground truth.  Per video the model's A -- one eval forward of the sampled
frames with the one spectrogram -- goes to the host and through binarize / cal_ciou / cal_auc / mtc: the per-frame
cIoUs must be equal exactly, the three metrics to 1e-12."""
import numpy as np
import pytest
import torch

import avenet_oracle as orc
import eval_oracle as evo
import tube_oracle as tor
from avt_amd import evaluate as ev
from avt_amd import render

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
RATE = 2


def _fullmodel():
    from avt_amd.model import FullModel

    m = FullModel(orc.Args())
    m.load_state_dict(tor.make_tube_state(0))
    return m.to(DEV)


def _gt(n, seed):
    """[n,224,224] VGG-SS style maps: one or two boxes per frame, moving with the frame"""
    out = []
    for i in range(n):
        x0 = 0.05 + 0.1 * ((i + seed) % 5)
        boxes = [[x0, 0.1, x0 + 0.45, 0.8]] + ([[0.5, 0.55, 0.95, 0.9]] if (i + seed) % 2 else [])
        out.append(evo.gt_map_vggss(boxes))
    gt = np.stack(out)
    assert set(np.unique(gt)) == {0.0, 1.0}
    return gt


def _videos(size=32, lengths=(6, 12)):
    """T = 6 -> frames 2, 4; T = 12 -> frames 2, 4, 6, 8, 10"""
    vids = []
    for k, T in enumerate(lengths):
        frames = tor.make_video(1, T, size, seed=3 + k).to(DEV)
        spec = orc.make_spectrogram(1, 65, 76, seed=2 + k).to(DEV)
        vids.append((frames, spec, _gt(len(ev.tube_indices(T, RATE)), k)))
    assert [len(v[2]) for v in vids] == [2, 5][:len(lengths)]
    return vids


def _host_protocol(A, gt):
    """the reference's per-video loop on the host, from heat maps A [n,1,h,w]"""
    A = A.detach().float().cpu().numpy()
    preds = [evo.binarize(A[i, 0]) for i in range(len(A))]
    cious = [evo.cal_ciou(p, g, 0.5)[0] for p, g in zip(preds, gt)]
    return dict(cious=cious, ciou=np.sum(np.array(cious) >= 0.5) / len(cious), auc=evo.cal_auc(cious),
                mtc=evo.mtc(preds))


def _check(res, refs):
    assert len(res["per_video"]) == len(refs)
    for v, r in zip(res["per_video"], refs):
        assert v["cious"] == [float(c) for c in r["cious"]]
        for k in ("ciou", "auc", "mtc"):
            assert abs(v[k] - r[k]) < 1e-12, (k, v[k], r[k])
    for k in ("ciou", "auc", "mtc"):
        assert abs(res[k] - np.sum([r[k] for r in refs]) / len(refs)) < 1e-12, k
    assert all(0.0 <= res[k] <= 1.0 for k in ("ciou", "auc", "mtc"))


def _own_maps_full(m, vids):
    m.eval()
    with torch.no_grad():
        return [m(spec, frames[:, :, ev.tube_indices(frames.shape[2], RATE)])[0] for frames, spec, _ in vids]


@pytest.mark.parametrize("folded", [False, True])
def test_fullmodel_per_video_metrics(folded):
    m = _fullmodel()
    if folded:
        m.enable_folded_inference()
    vids = _videos()
    refs = [_host_protocol(A, gt) for A, (_, _, gt) in zip(_own_maps_full(m, vids), vids)]
    for training in (True, False):
        m.train(training)
        res = ev.evaluate_tube(m, vids, sampling_rate=RATE)
        assert m.training is training
        _check(res, refs)
    assert [len(v["cious"]) for v in res["per_video"]] == [2, 5]
    assert [v["name"] for v in res["per_video"]] == [0, 1]


def test_too_few_sampled_frames_and_restored_mode():
    m = _fullmodel().train()
    frames, spec, gt = _videos(lengths=(6,))[0]
    with pytest.raises(ValueError, match="at least two frames"):
        ev.evaluate_tube(m, [(frames[:, :, :4], spec, gt[:1])], sampling_rate=RATE)   # range(2, 3, 2) = [2]
    assert m.training is True
    with pytest.raises(ValueError, match="at least two frames"):
        ev.evaluate_tube(m, [(frames, spec, gt)])   # the default sampling_rate 16 samples nothing of 6 frames
    assert m.training is True


def test_avenet_runs_frame_by_frame():
    from avt_amd.model import AVENet

    m = AVENet(orc.Args(), False)
    m.load_state_dict(orc.make_state(0))
    m = m.to(DEV).eval()
    vids = _videos(size=64)
    refs = []
    with torch.no_grad():
        for frames, spec, gt in vids:
            A = torch.cat([m(frames[:, :, i], spec)[0] for i in ev.tube_indices(frames.shape[2], RATE)])
            refs.append(_host_protocol(A, gt))
    m.train()
    res = ev.evaluate_tube(m, vids, sampling_rate=RATE)
    assert m.training is True
    _check(res, refs)


def test_render_to_receives_the_overlays():
    """224 x 224 frames (the gt maps' size): the callback gets, per video, exactly render.overlay of the sampled
    frames, the binarised predictions and the gt maps."""
    m = _fullmodel().eval()
    frames = tor.make_video(1, 6, 224, seed=5).to(DEV)
    spec = orc.make_spectrogram(1, 65, 76).to(DEV)
    gt = _gt(2, 1)
    seen = []
    res = ev.evaluate_tube(m, [("clip_a", frames, spec, gt)], sampling_rate=RATE,
                           render_to=lambda name, images: seen.append((name, images)))
    assert len(seen) == 1 and seen[0][0] == "clip_a" and res["per_video"][0]["name"] == "clip_a"
    images = seen[0][1]
    assert images.shape == (2, 224, 224, 3) and images.dtype == torch.uint8 and images.is_cuda
    idx = ev.tube_indices(6, RATE)
    with torch.no_grad():
        A = m(spec, frames[:, :, idx])[0]
    _, maps = ev.localize(A, torch.from_numpy(gt), return_maps=True)
    assert torch.equal(images, render.overlay(frames[:, :, idx], pred=maps, gt=torch.from_numpy(gt)))
    _check(res, [_host_protocol(A, gt)])
