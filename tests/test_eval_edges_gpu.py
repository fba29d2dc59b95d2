"""avt_localize_ciou / avt_pair_ciou (avt_amd.evaluate) at their edges, bit-exact against the restated
test protocol (oracle/eval_oracle.py): output sizes other than 224 (odd S, S below and above the
1024-thread loops' trip, h or w of 1, downscales), maps that are negative, span many binades, sit on
large ties at the median, or are constant, fractional ground truth, and pair cIoU at lengths that are
no multiple of the block.

All inputs are finite.  NaN heat maps are outside the protocol (numpy's min propagates NaN, the
kernel's fminf does not), and so is 0 / 0 (an empty prediction against an empty gt, or two empty
maps in mTC): neither is produced here."""
import numpy as np
import pytest
import torch

import eval_oracle as evo
from avt_amd import evaluate as ev

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N_MAPS = 8


def _maps(h, w, seed):
    """[8, h, w] float32 heat maps, one kind each."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    A = np.empty((N_MAPS, h, w), dtype=np.float64)
    A[0] = rng.standard_normal((h, w)) - 3.0                  # every value negative
    A[0] = np.minimum(A[0], -1e-3)
    mag = 10.0 ** rng.uniform(-30, 30, (h, w))                # 1e-30 .. 1e30, mixed signs
    A[1] = mag * rng.choice([-1.0, 1.0], (h, w))
    A[1].flat[0] = 1e30
    A[1].flat[-1] = -1e-30 if h * w > 1 else 1e30
    A[2] = np.where(yy < (h + 1) // 2, 0.75, -0.25)           # two values: top half a, bottom half b
    A[3] = np.where(xx < w // 2, -2.0, 5.0)                   # ... and left / right, the other order
    A[4] = (yy - xx) * 0.25                                   # minus its own transpose; ties on diagonals
    A[5] = -3.0                                               # constant: pred = 1 + map < 0 everywhere
    A[6] = 0.25                                               # constant: pred = 1.25 everywhere
    A[7] = 0.5 + 1e-3 * rng.standard_normal((h, w))           # one outlier squeezes the rest to ~1 ulp steps
    A[7].flat[(h * w) // 2] = 1e6
    A = A.astype(np.float32)
    assert np.isfinite(A).all()
    return A


def _flickr_gts(S):
    """Flickr-style maps of two overlapping boxes: values 0, 0.5 and 1."""
    out = []
    for i in range(N_MAPS):
        boxes = [[16 * i, 0, 256, 128 + 8 * i], [128, 16 * i, 256, 256]]
        out.append(evo.gt_map_flickr(boxes, size=S))
    gt = np.stack(out)
    assert set(np.unique(gt)) <= {0.0, 0.5, 1.0} and 0.5 in gt and (gt.sum(axis=(1, 2)) > 0).all()
    return gt


def _reference(A, S):
    """The protocol's binarised maps, computed once per (maps, S)."""
    return [evo.binarize(a, size=S) for a in A]


def _check(A, gt, S, preds, stats, maps):
    stats, maps = stats.cpu().numpy(), maps.cpu().numpy()
    assert stats.shape == (len(A), 3) and stats.dtype == np.float64
    assert maps.shape == (len(A), S, S) and maps.dtype == np.uint8
    for i, pred in enumerate(preds):
        np.testing.assert_array_equal(maps[i], (pred >= 0.5).astype(np.uint8), err_msg=f"map {i} S={S}")
        c, inter, den = evo.cal_ciou(pred, gt[i], 0.5)
        assert (stats[i, 0], stats[i, 1], stats[i, 2]) == (c, inter, den), (i, S)


SIZES = [(14, 14, 3), (14, 14, 2), (7, 9, 33), (1, 1, 16), (1, 9, 16), (9, 1, 16), (14, 14, 225), (14, 14, 512),
         (40, 40, 16), (300, 17, 64)]


@pytest.mark.parametrize("h,w,S", SIZES)
def test_localize_sizes_maps_and_gts(h, w, S):
    """Every map kind at every size, against fractional (Flickr), all-ones and exactly-the-prediction
    ground truth; then the three return_maps / gt combinations agree with each other."""
    A = _maps(h, w, 1000 * h + 10 * w + S)
    preds = _reference(A, S)
    dA = torch.from_numpy(A).to(DEV)
    exact = np.stack([(p >= 0.5).astype(np.float64) if (p >= 0.5).any() else np.ones((S, S)) for p in preds])
    gts = {"flickr": _flickr_gts(S), "ones": np.ones((N_MAPS, S, S)), "exact": exact}
    for name, gt in gts.items():
        stats, maps = ev.localize(dA[:, None], torch.from_numpy(gt).to(DEV), size=S, return_maps=True)
        _check(A, gt, S, preds, stats, maps)
        if name == "exact":
            for i, p in enumerate(preds):
                if (p >= 0.5).any():
                    assert stats[i, 0].item() == 1.0, i
    only_stats, none = ev.localize(dA, torch.from_numpy(gt).to(DEV), size=S)
    assert none is None and torch.equal(only_stats, stats)
    none, only_maps = ev.localize(dA, size=S, return_maps=True)
    assert none is None and torch.equal(only_maps, maps)
    with pytest.raises(ValueError, match="return_maps"):
        ev.localize(dA, size=S)


def test_the_kinds_hit_what_they_are_for():
    """CPU: the maps above put the median on a tie (two-valued maps: more than a third of the pixels
    equal the threshold), give an empty prediction (negative constant) and a full one (positive
    constant), at an odd and an even S."""
    for S in (33, 16):
        A = _maps(7, 9, 5)
        for k in (2, 3):
            resized = evo.cv2_resize_linear(A[k], S)
            pred = 1 - evo.normalize_img(-resized)
            thr = np.sort(pred.flatten())[S * S // 2]
            assert (pred == thr).sum() > (S * S) // 3, (S, k)
        preds = _reference(A, S)
        assert not (preds[5] >= 0.5).any() and (preds[6] >= 0.5).all()
        assert (1 - evo.normalize_img(-evo.cv2_resize_linear(A[5], S)) < 0).all()


def test_size_above_the_table_is_an_error():
    A = torch.from_numpy(_maps(14, 14, 7)).to(DEV)
    with pytest.raises((RuntimeError, ValueError), match="S=513"):
        ev.localize(A, size=513, return_maps=True)
    with pytest.raises((RuntimeError, ValueError)):
        ev.localize(A, size=1, return_maps=True)


def test_rows_of_a_large_batch_equal_single_runs():
    """N = 300 maps of 7 x 9 at S = 16 in one launch: rows 0, 150 and 299 are bit-equal to the same
    maps run as N = 1, and to the protocol."""
    S, N = 16, 300
    rng = np.random.default_rng(11)
    A = (rng.standard_normal((N, 7, 9)) * 0.3 + 0.5).astype(np.float32)
    gt = np.stack([evo.gt_map_flickr([[8 * (i % 16), 0, 256, 200], [100, 40, 256, 256]], size=S) for i in range(N)])
    dA, dgt = torch.from_numpy(A).to(DEV), torch.from_numpy(gt).to(DEV)
    stats, maps = ev.localize(dA, dgt, size=S, return_maps=True)
    for i in (0, 150, 299):
        s1, m1 = ev.localize(dA[i:i + 1].clone(), dgt[i:i + 1].clone(), size=S, return_maps=True)
        assert torch.equal(s1, stats[i:i + 1]) and torch.equal(m1, maps[i:i + 1]), i
    rows = [0, 1, 149, 150, 151, 298, 299]
    _check(A[rows], gt[rows], S, _reference(A[rows], S), stats[rows], maps[rows])


def _pair_cases(T, n, seed):
    rng = np.random.default_rng(seed)
    half = np.zeros(n, dtype=np.uint8)
    half[: (n + 1) // 2] = 1
    same = np.tile(half, (T, 1))                                     # identical neighbours: cIoU 1
    disjoint = np.stack([half if t % 2 == 0 else 1 - half for t in range(T)])   # cIoU 0
    rand = (rng.random((T, n)) < 0.4).astype(np.uint8)
    rand[:, -1] = 1                                                  # no map is empty
    return {"same": (same, 1.0), "disjoint": (disjoint, 0.0), "random": (rand, None)}


@pytest.mark.parametrize("T", [2, 5])
@pytest.mark.parametrize("n", [1, 1023, 1025, 224 * 224])
def test_pair_ciou_lengths_and_extremes(n, T):
    for name, (p, expect) in _pair_cases(T, n, 13 * n + T).items():
        assert all(p[t].any() or p[t + 1].any() for t in range(T - 1))  # never 0 / 0
        got = ev.mtc(torch.from_numpy(p).to(DEV))
        ref = evo.mtc([m.astype(np.float64) for m in p])
        assert abs(got - ref) < 1e-12, (name, n, T, got, ref)
        if expect is not None:
            assert got == expect, (name, n, T)
    if n == 224 * 224:  # the [T, S, S] form mtc() documents
        p = _pair_cases(T, n, 17)["random"][0]
        got = ev.mtc(torch.from_numpy(p.reshape(T, 224, 224)).to(DEV))
        assert abs(got - evo.mtc([m.astype(np.float64) for m in p])) < 1e-12
    with pytest.raises(ValueError, match="two frames"):
        ev.mtc(torch.ones(1, n, dtype=torch.uint8, device=DEV))
