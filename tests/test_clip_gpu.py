"""avt_clip_transform (avt_amd.frames.ClipTransform) against the same pipeline done with Pillow, frame by
frame (tests/clip_oracle.py): every comparison is bitwise on the float32 outputs, no tolerance, nothing
excluded.  Every device buffer the transform allocates (both outputs and the workspace) sits between
256-byte guard bands of a sentinel that must survive the call."""
import ctypes
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import avenet_oracle as orc
import clip_oracle as co
import frames_oracle as fo
from avt_amd import frames as fr
from avt_amd._lib import lib, query
from avt_amd.frames import ClipParams, ClipTransform, FrameTransform
from avt_amd.trunk import P, stream_ptr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GUARD = 256
FILL = 0xA5
B, C, S_, H_ = fr.BRIGHTNESS, fr.CONTRAST, fr.SATURATION, fr.HUE


@contextmanager
def guarded():
    """fr._empty carves every buffer out of a 0xA5-filled one with GUARD bytes on either side; on exit the
    guards must still hold the fill"""
    made = []

    def alloc(shape, dtype, device):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        raw = torch.full((2 * GUARD + n,), FILL, dtype=torch.uint8, device=device)
        made.append((raw, n))
        return raw[GUARD:GUARD + n].view(dtype).reshape(shape)

    real = fr._empty
    fr._empty = alloc
    try:
        yield made
        torch.cuda.synchronize()
        for raw, n in made:
            assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + n:] == FILL).all()), \
                f"a write outside a {n}-byte buffer"
    finally:
        fr._empty = real


def _frames(h, w, t, seed):
    """t different uint8 [h, w, 3] frames: random, with a smooth ramp and saturated corners in every other one
    (the bicubic overshoot is clipped at 0 and 255)"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(t):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if k % 2:
            yy, xx = np.mgrid[0:h, 0:w]
            img[..., 0] = (yy * 255 // max(h - 1, 1)).astype(np.uint8)
            img[: h // 4, : w // 4] = 255
            img[-(h // 4):, -(w // 4):] = 0
        out.append(img)
    return out


def _run(t, clips, params):
    with guarded() as made:
        out = t(clips, params=params)
        assert len(made) == (3 if t.mode == "train" else 2)
    return out


def _check(t, clips, params, tag=""):
    got = _run(t, clips, params)
    ref_f, ref_a = co.pil_clips(clips, params, t.size, train=t.mode == "train")
    if t.mode != "train":
        got = (got, None)
    shape = (len(clips), 3, len(clips[0]), t.size, t.size)
    assert got[0].shape == shape and got[0].dtype == torch.float32
    np.testing.assert_array_equal(got[0].cpu().numpy(), ref_f, err_msg=f"frames {tag}")
    if ref_a is not None:
        assert got[1].shape == shape and got[1].dtype == torch.float32
        a = got[1].cpu().numpy()
        for i in range(len(clips)):
            np.testing.assert_array_equal(a[i], ref_a[i], err_msg=f"augmented, clip {i} {params[i]} {tag}")
    return got


FOUR = ((B, 1.37), (C, 0.73), (S_, 1.5), (H_, -0.2))


# ------------------------------------------------------------------------------- small geometry
@pytest.mark.parametrize("corner", range(4))
def test_small_geometry_corners_and_flips(corner):
    """image_size 32 (resize to 35, second crop 22), b = 2, t = 3, sources 40x56 and 71x45; the second clip is
    resized to 32 x 50, its width equal to the crop.  Both views' crops at one corner per case, all four
    combinations of the two flips over the cases, and each clip the opposite of the other."""
    t = ClipTransform(32, "train")
    assert (t.resize_to, t.size2) == (35, 22)
    clips = [_frames(40, 56, 3, 10 + corner), _frames(71, 45, 3, 20 + corner)]
    top, left = bool(corner & 2), bool(corner & 1)
    f1, f2 = bool(corner & 1), bool(corner & 2)
    rw, rh = fo.resized_size(56, 40, 35)
    assert (rw, rh) == (49, 35)
    params = [
        ClipParams(rw, rh, (rh - 32) * top, (rw - 32) * left, f1, 10 * (not top), 10 * left, FOUR[corner:] + FOUR[:corner], f2),
        ClipParams(32, 50, 18 * (not top), 0, not f1, 10 * top, 10 * (not left), FOUR[:2], not f2),
    ]
    _check(t, clips, params, f"corner {corner}")


# ----------------------------------------------------------------------- each op at its edges
def _content():
    """uint8 [32, 32, 3] whose top-left 22 x 22 (the second view's crop) holds random colours, gray pixels
    (max == min), pixels whose maximum is R, G, B in turn (and ties), and saturated / black pixels"""
    rng = np.random.default_rng(31)
    a = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    a[0, :22] = a[0, :22, :1]                                    # gray
    a[1, :22] = np.sort(a[1, :22], axis=1)[:, ::-1]              # max is R
    a[2, :22] = np.sort(a[2, :22], axis=1)[:, [1, 2, 0]]         # max is G
    a[3, :22] = np.sort(a[3, :22], axis=1)                       # max is B
    a[4, :8] = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (0, 0, 0),
                (255, 255, 255)]
    a[5, :22] = rng.integers(250, 256, (22, 3), dtype=np.uint8)  # saturate under a factor > 1
    a[6, :22] = rng.integers(0, 4, (22, 3), dtype=np.uint8)
    return a


def _identity(ops, top=0, left=0, flip2=False):
    """32 x 32 sources pass view 1 unchanged, so the jitter's input is the source itself"""
    return ClipParams(32, 32, 0, 0, False, top, left, tuple(ops), flip2)


def test_each_op_alone_at_its_edges():
    """One clip per (op, factor): factors 0, 0.5, 1, 1.5 of the three blends, hue -0.5, 0, 0.5, on content with
    gray pixels, each channel as the maximum, and pixels that saturate (the clipping branch of factor 1.5)."""
    t = ClipTransform(32, "train")
    a = _content()
    chains = [((k, f),) for k in (B, C, S_) for f in (0.0, 0.5, 1.0, 1.5)] + [((H_, h),) for h in (-0.5, 0.0, 0.5)]
    clips = [[a, a[::-1].copy()] for _ in chains]
    crop = a[:22, :22]
    # the content does what the case is about (CPU)
    assert (crop.max(-1) == crop.min(-1)).any()
    for c in range(3):
        assert ((crop.argmax(-1) == c) & (crop.max(-1) != crop.min(-1))).any()
    assert (crop.astype(np.float32) * 1.5 > 255).any()
    m = co.np_contrast_mean(crop)
    assert ((m + 1.5 * (crop.astype(np.float32) - m)) < 0).any() and ((m + 1.5 * (crop.astype(np.float32) - m)) > 255).any()
    assert not np.array_equal(co.np_op(crop, co.HUE, 0.0), crop)  # hue 0 is not the identity
    _check(t, clips, [_identity(ch) for ch in chains])


def test_contrast_mean_constant_frame_and_half():
    """Contrast on a constant frame, and on crops whose mean gray is exactly 100.5 (rounds to 101): per frame --
    the clip's second frame has another mean."""
    t = ClipTransform(32, "train")
    const = np.full((32, 32, 3), 77, dtype=np.uint8)
    half = np.full((32, 32, 3), 100, dtype=np.uint8)
    half[:11] = 101  # 11 of the crop's 22 rows
    other = np.full((32, 32, 3), 30, dtype=np.uint8)
    other[:, ::2] = 201
    assert co.np_contrast_mean(half[:22, :22]) == 101 and int(co.np_gray(half[:22, :22]).sum()) * 2 == 201 * 484
    assert co.np_contrast_mean(other[:22, :22]) != 101
    clips, params = [], []
    for f in (0.0, 0.5, 1.0, 1.5):
        clips += [[const, other], [half, other]]
        params += [_identity([(C, f)])] * 2
    _check(t, clips, params)


# ----------------------------------------------------------------------------------- chains
def test_chains_with_contrast_first_middle_last_and_empty():
    """All four ops in five orders (Contrast first, second, third, last: its mean depends on the ops before
    it), the empty chain and a two-op chain, one clip each; frames differ inside a clip."""
    t = ClipTransform(32, "train")
    orders = [(1, 0, 2, 3), (0, 1, 2, 3), (3, 2, 1, 0), (2, 3, 0, 1), (3, 0, 2, 1)]
    chains = [tuple(FOUR[i] for i in o) for o in orders] + [(), ((H_, 0.31), (C, 1.44))]
    a = _content()
    clips = [[a, _frames(32, 32, 1, 40 + k)[0], a.transpose(1, 0, 2).copy()] for k in range(len(chains))]
    _check(t, clips, [_identity(ch, top=k % 11, left=10 - k, flip2=bool(k % 2)) for k, ch in enumerate(chains)])
    # the prefix matters: Contrast's mean differs between the orders (CPU)
    crop = a[:22, :22]
    means = {co.np_contrast_mean(co.np_chain(crop, ch[:[k for k, _ in ch].index(C)])) for ch in chains[:5]}
    assert len(means) > 1


# ------------------------------------------------------------------- placement, modes, sizes
def test_ncthw_placement():
    """Frames of a clip differ from each other and t != 3, so a swapped t / channel stride cannot pass; against
    the oracle, and frame by frame against the single-clip runs."""
    t = ClipTransform(32, "train")
    clips = [_frames(40, 56, 4, 50), _frames(64, 48, 4, 51)]
    rnd = __import__("random").Random(52)
    params = [t.params(c[0].shape[1], c[0].shape[0], rnd) for c in clips]
    fa = _check(t, clips, params)
    for i in range(2):
        for k in range(4):
            one = _run(t, [[clips[i][k]]], [params[i]])
            assert torch.equal(one[0][0, :, 0], fa[0][i, :, k]) and torch.equal(one[1][0, :, 0], fa[1][i, :, k])


def test_test_mode():
    t = ClipTransform(32, "test")
    clips = [_frames(40, 56, 3, 60), _frames(71, 45, 3, 61), _frames(32, 32, 3, 62)]
    params = [t.params(c[0].shape[1], c[0].shape[0]) for c in clips]
    assert params[0] == ClipParams(44, 32, 0, 6, False)
    out = _check(t, clips, params)[0]
    assert isinstance(t(clips), torch.Tensor) and torch.equal(t(clips), out)


def test_real_geometry():
    """image_size 224, b = 1, t = 2, 360 x 640 sources: 246 -> 224 and 156 -> 224, drawn parameters."""
    t = ClipTransform(224, "train")
    clips = [_frames(360, 640, 2, 70)]
    p = t.params(640, 360, __import__("random").Random(71))
    assert (p.rw, p.rh, t.size2, len(p.ops)) == (437, 246, 156, 4)
    _check(t, clips, [p])


def test_two_calls_are_bitwise_equal():
    t = ClipTransform(32, "train")
    clips = [_frames(40, 56, 3, 80), _frames(71, 45, 3, 81)]
    a = t(clips, rng=__import__("random").Random(82))
    b = t(clips, rng=__import__("random").Random(82))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], a[1])


def test_view1_of_a_one_frame_clip_equals_frame_transform():
    frames = _frames(150, 200, 3, 90)
    ct, ft = ClipTransform(32, "train"), FrameTransform(32, "train")
    rw, rh = fo.resized_size(200, 150, 35)
    ps = [(rw, rh, 1, 9, True), (rw, rh, 3, 0, False), (rw, rh, 0, rw - 32, True)]
    ref = ft(frames, params=ps)
    got = _run(ct, [[f] for f in frames], [ClipParams(*p, 2, 3, ((S_, 0.8),), False) for p in ps])[0]
    assert got.shape == (3, 3, 1, 32, 32) and torch.equal(got[:, :, 0], ref)


# ------------------------------------------------------------------------------ C-ABI refusals
def test_c_abi_refusals():
    """negative code + avt_last_error() for null pointers, bad sizes, a short workspace, view2 without augmented
    and misaligned pointers; nothing is written."""
    b, t, s, hmax = 1, 2, 32, 40
    n_ws = int(query("avt_clip_workspace_bytes", b, t, s, hmax, 1))
    assert n_ws > 0 and n_ws % 16 == 0 and int(query("avt_clip_workspace_bytes", b, t, s, hmax, 0)) == b * t * 3 * hmax * s
    assert query("avt_clip_workspace_bytes", 0, t, s, hmax, 1) == 0 and query("avt_clip_workspace_bytes", b, t, 257, hmax, 1) == 0
    src = torch.zeros(t * 40 * 56 * 3 + 16, dtype=torch.uint8, device=DEV)
    desc = torch.zeros(t * 8 + 1, dtype=torch.int64, device=DEV)
    view2 = torch.zeros(80 + 8, dtype=torch.uint8, device=DEV)
    ws = torch.full((n_ws + 16,), FILL, dtype=torch.uint8, device=DEV)
    out = torch.full((2, b * 3 * t * s * s + 1), 7.0, device=DEV)
    mean, std = (ctypes.c_float * 3)(*fr.MEAN), (ctypes.c_float * 3)(*fr.STD)
    m, sd = ctypes.cast(mean, ctypes.c_void_p), ctypes.cast(std, ctypes.c_void_p)
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    good = dict(src=vp(src), desc=vp(desc), view2=vp(view2), b=b, t=t, S=s, Hmax=hmax, ws=vp(ws), ws_bytes=n_ws,
                mean=m, std=sd, frames=vp(out[0]), augmented=vp(out[1]))
    cases = [
        (dict(src=None), "null"), (dict(desc=None), "null"), (dict(ws=None), "null"), (dict(frames=None), "null"),
        (dict(mean=None), "null"), (dict(std=None), "null"),
        (dict(augmented=None), "go together"), (dict(view2=None), "go together"),
        (dict(b=0), "need"), (dict(t=0), "need"), (dict(S=0), "need"), (dict(S=257), "need"), (dict(Hmax=0), "need"),
        (dict(b=256, t=256), "need"), (dict(S=1), "empty"),
        (dict(ws_bytes=n_ws - 1), "workspace"), (dict(ws_bytes=0), "workspace"),
        (dict(ws=vp(ws, 8)), "misaligned"), (dict(desc=vp(desc, 4)), "misaligned"),
        (dict(view2=vp(view2, 4)), "misaligned"), (dict(frames=vp(out[0], 2)), "misaligned"),
        (dict(augmented=vp(out[1], 1)), "misaligned"),
    ]
    fn = lib().avt_clip_transform
    for change, msg in cases:
        a = {**good, **change}
        rc = fn(a["src"], a["desc"], a["view2"], a["b"], a["t"], a["S"], a["Hmax"], a["ws"], a["ws_bytes"], a["mean"],
                a["std"], a["frames"], a["augmented"], stream_ptr())
        err = lib().avt_last_error().decode()
        assert rc < 0 and msg in err, (change, rc, err)
    torch.cuda.synchronize()
    assert bool((ws == FILL).all()) and bool((out == 7.0).all())


# -------------------------------------------------------------------------- into the train step
def test_two_view_step_runs_on_the_transform_outputs():
    """TwoViewTrainStep.step(*tf(clips), spec) at image_size 64, the smallest the two-view tests run the
    2-D trunks at (tests/test_twoview_gpu.py)."""
    from avt_amd.model import AVENet
    from avt_amd.train import TwoViewTrainStep

    tf = ClipTransform(64, "train")
    clips = [_frames(90, 120, 3, 95), _frames(100, 80, 3, 96)]
    frames, augmented = tf(clips, rng=__import__("random").Random(97))
    assert frames.shape == augmented.shape == (2, 3, 3, 64, 64)
    m = AVENet(orc.Args(), False)
    m.load_state_dict(orc.make_state(0))
    step = TwoViewTrainStep(m.to(DEV).train(), lr=1e-4)
    losses = step.step(frames, augmented, orc.make_spectrogram(2, 65, 76).to(DEV))
    torch.cuda.synchronize()
    assert losses.shape == (5,) and bool(torch.isfinite(losses).all())
