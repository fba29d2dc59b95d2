"""csrc/flow.hip on the GPU against tests/flow_oracle.py: avt_flow_warp and avt_flow_consistency bit for bit,
avt_flow_loss bit for bit on exactly summable inputs and within the oracle's rounding bounds on random ones,
avt_flow_color byte for byte outside the oracle's guard band, and evaluate_tube(flow_fn=...).

Raw entry points run on outputs that lie between two 256-byte guard bands of a sentinel inside a larger buffer."""
import ctypes

import numpy as np
import pytest
import torch

import flow_cases as fc
import flow_oracle as fo
from avt_amd import _lib
from avt_amd import evaluate as ev
from avt_amd import flow
from avt_amd.losses import FlowLoss
from avt_amd.trunk import P, stream_ptr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F = np.float32
GUARD = 256
COORDS = {"grid": 0, "pixels": 1}


class Guarded:
    """`nbytes` of output between two guard bands, the whole buffer filled with `fill`"""

    def __init__(self, nbytes, fill=0xA5):
        self.fill, self.nbytes = fill, nbytes
        self.buf = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=DEV)

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + GUARD)

    def view(self, dtype, shape):
        return self.buf[GUARD:GUARD + self.nbytes].view(dtype).reshape(shape)

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.fill).all() and (self.buf[GUARD + self.nbytes:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def raw_warp(src, field, coords, fill=0xA5):
    N, H, W = src.shape
    Ho, Wo = field.shape[1:3]
    out = Guarded(N * Ho * Wo * 4, fill)
    d_src, d_field = dev(src), dev(field)             # held until the synchronize below
    _lib.call("avt_flow_warp", P(d_src), int(src.dtype == np.uint8), N, H, W, P(d_field), Ho, Wo, COORDS[coords],
              out.ptr(), stream_ptr())
    torch.cuda.synchronize()
    assert out.guards_intact()
    return out.view(torch.float32, (N, Ho, Wo)).cpu().numpy()


def raw_consistency(pred, field, coords, fill=0xA5):
    T, S, _ = pred.shape
    out = Guarded((T - 1) * 24, fill)
    ws = Guarded(int(_lib.query("avt_flow_workspace_bytes", T - 1, S * S)), fill)
    d_pred, d_field = dev(pred), dev(field)
    _lib.call("avt_flow_consistency", P(d_pred), T, S, P(d_field), COORDS[coords], out.ptr(), ws.ptr(), stream_ptr())
    torch.cuda.synchronize()
    assert out.guards_intact() and ws.guards_intact()
    return out.view(torch.float64, (T - 1, 3)).cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_rows(got, want):
    """consistency rows against the host's: bit for bit, except that 0 / 0 is a NaN whose sign the host and the
    device choose differently"""
    nan = np.isnan(want)
    return same_bits(np.where(nan, 0.0, got), np.where(nan, 0.0, want)) and np.array_equal(np.isnan(got), nan)


# ---------------------------------------------------------------- warp / consistency
@pytest.mark.parametrize("H,W", fc.SHAPES)
def test_warp_bitwise(H, W):
    for k, kind in enumerate(fc.FIELD_KINDS):
        N = 1 + (k + H) % 3
        for src in (fc.float_maps(N, H, W, 10 * H + k), fc.binary_maps(N, H, W, 10 * W + k)):
            pf = fc.pixel_field(kind, N, H, W, 7 * H + W + k)
            got = raw_warp(src, pf, "pixels", fill=0xA5 if k % 2 else 0x5A)
            assert same_bits(got, fo.warp(src, pf, "pixels")), (kind, "pixels", src.dtype)
            if kind == "zero":
                assert same_bits(got, fo.as_map(src))                      # the identity
            if kind == "shift_out":
                assert not got.any() and not np.signbit(got).any()
            Ho, Wo = W + 1, H + 2                                          # the field's own size
            gf = fc.grid_field(kind, N, Ho, Wo, 3 * H + W + k)
            assert same_bits(raw_warp(src, gf, "grid"), fo.warp(src, gf, "grid")), (kind, "grid", src.dtype)
    # the module's wrapper: both ranks, same bytes, twice
    src, pf = fc.float_maps(2, H, W, 1), fc.pixel_field("random", 2, H, W, 2)
    a = flow.warp(dev(src), dev(pf), "pixels")
    b = flow.warp(dev(src)[:, None], dev(pf), "pixels")
    assert a.shape == (2, H, W) and b.shape == (2, 1, H, W) and torch.equal(a, b[:, 0])
    assert same_bits(a.cpu().numpy(), fo.warp(src, pf, "pixels"))


def test_warp_half_pixel_checkerboard_and_more_maps_than_the_grid():
    board = fc.checkerboard(2, 14, 14)
    got = raw_warp(board, fc.pixel_field("half", 2, 14, 14, 0), "pixels")
    assert np.all(got[:, :, :-1] == F(0.5)) and np.all((got[:, :, -1] == 0) | (got[:, :, -1] == F(0.5)))
    # grid.y holds at most 65535 maps: the rest come by the stride loop
    N = 65535 + 70
    rng = np.random.default_rng(3)
    src = rng.standard_normal((N, 1, 1)).astype(F)
    pf = (rng.integers(-4, 5, (N, 1, 1, 2)) / 4).astype(F)
    assert same_bits(raw_warp(src, pf, "pixels"), fo.warp(src, pf, "pixels"))


@pytest.mark.parametrize("S", [1, 2, 3, 14, 17, 33, 64, 224])
def test_consistency_bitwise_and_zero_field_is_pair_ciou(S):
    for k, kind in enumerate(fc.FIELD_KINDS):
        T = 2 + (k + S) % 3
        pred = fc.binary_maps(T, S, S, 5 * S + k)
        if kind == "half":
            pred = fc.checkerboard(T, S, S)
        pf = fc.pixel_field(kind, T - 1, S, S, S + k)
        with np.errstate(invalid="ignore"):
            want = fo.consistency(pred, pf, "pixels")
        got = raw_consistency(pred, pf, "pixels", fill=0x5A if k % 2 else 0xA5)
        assert same_rows(got, want), (kind, got, want)
        assert same_bits(raw_consistency(pred, pf, "pixels"), got)           # twice the same bytes
        gf = fc.grid_field(kind, T - 1, S, S, 2 * S + k)
        with np.errstate(invalid="ignore"):
            assert same_rows(raw_consistency(pred, gf, "grid"), fo.consistency(pred, gf, "grid")), (kind, "grid")
        if kind == "zero":
            # the tie to the uncompensated metric: avt_pair_ciou's output, bit for bit
            plain = torch.empty(T - 1, device=DEV, dtype=torch.float64)
            d_pred = dev(pred)
            _lib.call("avt_pair_ciou", P(d_pred), T, S * S, P(plain), stream_ptr())
            assert same_bits(got[:, 0], plain.cpu().numpy())
            if np.isfinite(got[:, 0]).all():
                assert flow.mtc_flow(dev(pred), dev(pf)) == ev.mtc(dev(pred))
        if kind == "half" and S > 1:
            # every interior sample is exactly 0.5 and counts as infer (and so does 0.5 * 1 in the last column)
            assert got[0, 1] + (got[0, 2] - (pred[1] != 0).sum()) == S * (S - 1) + pred[0][:, -1].sum()
    out = flow.consistency(dev(pred), dev(pf))
    assert out.shape == (T - 1, 3) and out.dtype == torch.float64 and same_bits(out.cpu().numpy(), got)


def test_refusals_leave_the_outputs_alone():
    src, f = dev(fc.float_maps(2, 4, 5, 0)), dev(fc.pixel_field("random", 2, 4, 5, 1))
    pred, pf = dev(fc.binary_maps(3, 4, 4, 0)), dev(fc.pixel_field("random", 2, 4, 4, 1))
    out, ws = Guarded(4096), Guarded(4096)
    st = stream_ptr()
    bad_warps = [
        (None, 0, 2, 4, 5, P(f), 4, 5, 1, out.ptr(), st), (P(src), 0, 2, 4, 5, None, 4, 5, 1, out.ptr(), st),
        (P(src), 0, 2, 4, 5, P(f), 4, 5, 1, None, st), (P(src), 0, 0, 4, 5, P(f), 4, 5, 1, out.ptr(), st),
        (P(src), 0, 2, 0, 5, P(f), 4, 5, 1, out.ptr(), st), (P(src), 0, 2, 4, 0, P(f), 4, 5, 1, out.ptr(), st),
        (P(src), 0, 2, 4, 5, P(f), 0, 5, 0, out.ptr(), st), (P(src), 0, 2, 4, 5, P(f), 4, -1, 0, out.ptr(), st),
        (P(src), 0, 2, 4, 5, P(f), 4, 5, 2, out.ptr(), st), (P(src), 0, 2, 4, 5, P(f), 4, 5, -1, out.ptr(), st),
        (P(src), 2, 2, 4, 5, P(f), 4, 5, 1, out.ptr(), st), (P(src), 0, 2, 4, 5, P(f), 5, 4, 1, out.ptr(), st),
        # a field pointer that is only 4-byte aligned is refused (include/avt.h)
        (P(src), 0, 1, 4, 5, ctypes.c_void_p(f.data_ptr() + 4), 4, 5, 1, out.ptr(), st),
    ]
    for args in bad_warps:
        with pytest.raises(RuntimeError, match="flow_warp"):
            _lib.call("avt_flow_warp", *args)
    bad_cons = [
        (None, 3, 4, P(pf), 1, out.ptr(), ws.ptr(), st), (P(pred), 3, 4, None, 1, out.ptr(), ws.ptr(), st),
        (P(pred), 3, 4, P(pf), 1, None, ws.ptr(), st), (P(pred), 3, 4, P(pf), 1, out.ptr(), None, st),
        (P(pred), 1, 4, P(pf), 1, out.ptr(), ws.ptr(), st), (P(pred), 3, 0, P(pf), 1, out.ptr(), ws.ptr(), st),
        (P(pred), 3, 4, P(pf), 2, out.ptr(), ws.ptr(), st),
        (P(pred), 2, 4, ctypes.c_void_p(pf.data_ptr() + 4), 1, out.ptr(), ws.ptr(), st),
    ]
    for args in bad_cons:
        with pytest.raises(RuntimeError, match="flow_consistency"):
            _lib.call("avt_flow_consistency", *args)
    x, lf = dev(fc.loss_inputs(1, 2, 33, 32, 0, True)[0]), dev(fc.loss_inputs(1, 2, 33, 32, 0, True)[1])
    for args in [(P(x), 1, 2, 33, 32, P(lf), 1, out.ptr(), None, ws.ptr(), st),     # 1056 pixels
                 (P(x), 1, 1, 4, 4, P(lf), 1, out.ptr(), None, ws.ptr(), st),
                 (P(x), 1, 2, 4, 4, P(lf), 3, out.ptr(), None, ws.ptr(), st),
                 (None, 1, 2, 4, 4, P(lf), 1, out.ptr(), None, ws.ptr(), st),
                 (P(x), 1, 2, 4, 4, P(lf), 1, out.ptr(), None, None, st)]:
        with pytest.raises(RuntimeError, match="flow_loss"):
            _lib.call("avt_flow_loss", *args)
    wheel = flow.WHEEL.to(DEV)
    for args in [(None, 2, 4, 4, P(wheel), out.ptr(), ws.ptr(), st), (P(pf), 0, 4, 4, P(wheel), out.ptr(), ws.ptr(), st),
                 (P(pf), 2, 4, 0, P(wheel), out.ptr(), ws.ptr(), st), (P(pf), 2, 4, 4, None, out.ptr(), ws.ptr(), st),
                 (P(pf), 2, 4, 4, P(wheel), out.ptr(), None, st)]:
        with pytest.raises(RuntimeError, match="flow_color"):
            _lib.call("avt_flow_color", *args)
    torch.cuda.synchronize()
    assert out.untouched() and ws.untouched()
    # the module's own checks come before any call
    with pytest.raises(RuntimeError, match="GPU"):
        flow.warp(src.cpu(), f.cpu())
    with pytest.raises(ValueError, match="coords"):
        flow.warp(src, f, "normalised")
    with pytest.raises(ValueError):
        flow.warp(src, f[:1], "pixels")
    with pytest.raises(ValueError, match="two frames"):
        flow.consistency(pred[:1], pf[:0])
    with pytest.raises(ValueError):
        flow.consistency(pred, pf[:1])
    with pytest.raises(ValueError):
        flow.flow_to_image(pf[..., :1])


# ---------------------------------------------------------------- loss
def raw_loss(x, field, with_dx=True, fill=0xA5):
    b, t, h, w = x.shape
    loss, ws = Guarded(4, fill), Guarded(b * (t - 1) * 4, fill)
    dx = Guarded(x.size * 4, fill) if with_dx else None
    d_x, d_field = dev(x), dev(field)
    _lib.call("avt_flow_loss", P(d_x), b, t, h, w, P(d_field), 1, loss.ptr(), dx.ptr() if dx else None, ws.ptr(),
              stream_ptr())
    torch.cuda.synchronize()
    assert loss.guards_intact() and ws.guards_intact() and (dx is None or dx.guards_intact())
    return (loss.view(torch.float32, ()).cpu().numpy(),
            dx.view(torch.float32, x.shape).cpu().numpy() if dx else None)


@pytest.mark.parametrize("b,t,h,w", [(2, 2, 14, 14), (2, 3, 14, 14), (3, 3, 1, 1), (1, 3, 32, 32), (1, 2, 16, 16)])
def test_loss_bitwise_on_exactly_summable_inputs(b, t, h, w):
    x, field = fc.loss_inputs(b, t, h, w, 100 * t + h, exact=True)
    want_loss, want_dx = fo.flow_loss_ordered(x, field, "pixels")
    loss, dx = raw_loss(x, field)
    assert same_bits(loss, np.asarray(want_loss)) and same_bits(dx, want_dx)
    if h * w > 1:
        assert dx[0, 1, 0, 0] == 0 or t > 2                       # d = 0 at frame 1 pixel 0: its own term is +0
        if t == 2:
            assert not np.signbit(dx[0, 1, 0, 0])
    again_loss, again_dx = raw_loss(x, field, fill=0x5A)
    assert same_bits(again_loss, loss) and same_bits(again_dx, dx)
    only_loss, none = raw_loss(x, field, with_dx=False)
    assert none is None and same_bits(only_loss, loss)


@pytest.mark.parametrize("b,t,h,w", [(2, 3, 14, 14), (1, 2, 32, 32), (4, 4, 5, 7)])
def test_loss_within_the_rounding_bound_on_random_inputs(b, t, h, w):
    x, field = fc.loss_inputs(b, t, h, w, 7 * h + t, exact=False)
    ref = fo.flow_loss_f64(x, field, "pixels")
    assert ref["min_margin"] > 0                                  # every sign is settled: a condition on the inputs
    loss, dx = raw_loss(x, field)
    print(f"loss {float(loss)!r} fp64 {ref['loss']!r} bound {ref['loss_bound']:.3e}; "
          f"dx worst ratio {np.max(np.abs(dx - ref['dx']) / ref['dx_bound']):.3f}")
    assert abs(float(loss) - ref["loss"]) <= ref["loss_bound"]
    assert np.all(np.abs(dx - ref["dx"]) <= ref["dx_bound"])
    want_loss, want_dx = fo.flow_loss_ordered(x, field, "pixels")
    assert same_bits(dx, want_dx) and same_bits(loss, np.asarray(want_loss))


def test_flowloss_module_backward_scale_and_refusals():
    x, field = fc.loss_inputs(2, 3, 14, 14, 3, exact=True)
    want_loss, want_dx = fo.flow_loss_ordered(x, field, "pixels")
    crit = FlowLoss(14 * 14)                                      # flow.py:117, unchanged
    xt = dev(x).requires_grad_(True)
    loss = crit(xt, dev(field))
    assert same_bits(loss.detach().cpu().numpy(), np.asarray(want_loss))
    (loss * 0.5).backward()
    assert same_bits(xt.grad.cpu().numpy(), want_dx * F(0.5))
    assert crit(dev(x), dev(field)).item() == float(want_loss)    # no gradient asked for
    gx, gf = fc.loss_inputs(1, 2, 4, 4, 1, exact=False)
    gf = (gf / 4).astype(F)
    assert FlowLoss(coords="grid")(dev(gx), dev(gf)).item() == pytest.approx(
        float(np.mean(np.abs(fo.warp(gx[0, :1], gf[0], "grid") - gx[0, 1:]))), rel=1e-5)
    with pytest.raises(ValueError, match="no gradient"):
        crit(xt, dev(field).requires_grad_(True))
    with pytest.raises(ValueError, match="t >= 2"):
        crit(dev(x)[:, :1], dev(field)[:, :0])
    with pytest.raises(ValueError, match="1024"):
        crit(torch.zeros(1, 2, 33, 32, device=DEV), torch.zeros(1, 1, 33, 32, 2, device=DEV))
    with pytest.raises(ValueError, match="field"):
        crit(dev(x), dev(field)[:, :1])
    with pytest.raises(RuntimeError, match="GPU"):
        crit(torch.from_numpy(x), torch.from_numpy(field))
    with pytest.raises(ValueError, match="coords"):
        FlowLoss(coords="flow")


# ---------------------------------------------------------------- colour
@pytest.mark.parametrize("name", sorted(fc.color_fields()))
def test_color_against_the_oracle(name):
    f = fc.color_fields()[name]
    img, excused, alt = fo.flow2img_report(f)
    H, W, _ = f.shape
    N = 2 if H * W < 1000 else 1
    stack = np.stack([f, f[::-1].copy()][:N])                     # the second field: the rows mirrored
    d = dev(stack)
    before = d.clone()
    out = Guarded(N * H * W * 3, 0x5A)
    ws = Guarded(int(_lib.query("avt_flow_workspace_bytes", N, H * W)))
    wheel = flow.WHEEL.to(DEV)
    _lib.call("avt_flow_color", P(d), N, H, W, P(wheel), out.ptr(), ws.ptr(), stream_ptr())
    torch.cuda.synchronize()
    assert out.guards_intact() and ws.guards_intact()
    assert same_bits(d.cpu().numpy(), before.cpu().numpy())       # the input is left alone
    got = out.view(torch.uint8, (N, H, W, 3)).cpu().numpy()
    if N == 2:
        assert np.array_equal(got[1][::-1][~excused], got[0][~excused])
    g = got[0].astype(int)
    assert np.array_equal(g[~excused], img[~excused]), name
    ok = (np.abs(g - img) <= 1).all(axis=2) | (np.abs(g - alt) <= 1).all(axis=2)
    print(f"{name}: {int(excused.sum())} excused of {excused.size}, {int((g != img).any(axis=2).sum())} differ")
    assert ok[excused].all(), name
    again = flow.flow_to_image(d[0])
    assert again.shape == (H, W, 3) and again.dtype == torch.uint8 and same_bits(again.cpu().numpy(), got[0])
    if name == "zero":
        assert not got.any()


# ---------------------------------------------------------------- evaluate_tube
def test_evaluate_tube_with_a_flow_fn():
    import avenet_oracle as orc
    import tube_oracle as tor
    from avt_amd.model import FullModel

    m = FullModel(orc.Args())
    m.load_state_dict(tor.make_tube_state(0))
    m = m.to(DEV).eval()
    vids = []
    for k, T in enumerate((6, 12)):
        n = len(ev.tube_indices(T, 2))
        gt = np.zeros((n, 224, 224))
        gt[:, 40:150, 30 + 10 * k:160] = 1
        vids.append((tor.make_video(1, T, 32, seed=3 + k).to(DEV), orc.make_spectrogram(1, 65, 76, seed=2 + k).to(DEV), gt))
    plain = ev.evaluate_tube(m, vids, sampling_rate=2)
    assert set(plain) == {"ciou", "auc", "mtc", "per_video"}
    assert all(set(v) == {"name", "ciou", "auc", "mtc", "cious"} for v in plain["per_video"])
    seen = []

    def zero_flow(name, sampled):
        seen.append((name, tuple(sampled.shape)))
        return torch.zeros(sampled.shape[2] - 1, 224, 224, 2, device=DEV)

    res = ev.evaluate_tube(m, vids, sampling_rate=2, flow_fn=zero_flow)
    assert seen == [(0, (1, 3, 2, 32, 32)), (1, (1, 3, 5, 32, 32))]
    assert set(res) == {"ciou", "auc", "mtc", "mtc_flow", "per_video"}
    for v, p in zip(res["per_video"], plain["per_video"]):
        assert v["mtc_flow"] == v["mtc"] == p["mtc"] and {k: v[k] for k in p} == p
    assert res["mtc_flow"] == res["mtc"] == plain["mtc"]

    def shift(name, sampled):                                      # a known whole-pixel motion: 3 right, 2 up
        f = torch.zeros(sampled.shape[2] - 1, 224, 224, 2, device=DEV)
        f[..., 0] = 3
        f[..., 1] = -2
        return f

    res = ev.evaluate_tube(m, vids, sampling_rate=2, flow_fn=shift)
    want = []
    with torch.no_grad():
        for frames, spec, gt in vids:
            A = m(spec, frames[:, :, ev.tube_indices(frames.shape[2], 2)])[0]
            maps = ev.localize(A, return_maps=True)[1].cpu().numpy()
            rows = fo.consistency(maps, shift(None, frames[:, :, :len(maps)]).cpu().numpy(), "pixels")
            want.append(float(rows[:, 0].sum() / len(rows)))
    assert all(abs(v["mtc_flow"] - w) < 1e-12 for v, w in zip(res["per_video"], want))   # the bound of the
    assert abs(res["mtc_flow"] - sum(want) / 2) < 1e-12 and res["mtc_flow"] != res["mtc"]  # existing metric checks
