"""tests/flow_oracle.py checked on the host, before any GPU run: its warp against torch's grid_sample, its two
coordinate conventions against each other, its loss gradient against fp64 autograd, the .flo functions of
avt_amd.flow against the oracle's and against a file the reference's writer wrote, the injected faults, and the
excused share of every colour field the GPU test draws."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import flow_cases as fc
import flow_oracle as fo

F = np.float32


def _grid_sample(src, field, dtype=torch.float32):
    out = TF.grid_sample(torch.from_numpy(src).to(dtype)[:, None], torch.from_numpy(field).to(dtype), mode="bilinear",
                         padding_mode="zeros", align_corners=False)
    return out[:, 0].numpy()


def test_warp_against_torch_grid_sample():
    """Random maps, grids reaching to +-1.3.  torch's vectorised CPU kernel may contract a product into the sum after
    it or add the four terms in another order, so the comparison is in units of ulp32(sum |w m|) per pixel.
    Measured here (the torch CPU build of this project's environment): 356 ulp.  It is not the sum that differs:
    torch's vectorised kernel un-normalises as (g + 1) * (size / 2) - 0.5 where its scalar definition, and this
    library, have ((g + 1) * size - 1) / 2, so a position can differ by an ulp of itself, and where a weight is
    tiny that moves the sample by many ulp of sum |w m|.  The assertion is twice the measured value."""
    worst = 0.0
    for seed, (N, H, W, Ho, Wo) in enumerate([(3, 14, 14, 14, 14), (2, 17, 33, 9, 40), (1, 64, 64, 224, 224),
                                              (2, 1, 1, 3, 2), (2, 2, 3, 17, 33)]):
        src = fc.float_maps(N, H, W, seed)
        field = fc.grid_field("random", N, Ho, Wo, 100 + seed)
        ours = fo.warp(src, field, "grid")
        theirs = _grid_sample(src, field)
        ix, iy = fo.positions(field, H, W, "grid")
        for n in range(N):
            cells, weights = fo.taps(ix[n], iy[n], H, W)
            mag = fo.taps_sum(np.abs(src[n]), cells, np.abs(weights))
            ulp = np.spacing(np.maximum(mag, np.finfo(F).tiny).astype(F))
            worst = max(worst, float(np.max(np.abs(ours[n].astype(np.float64) - theirs[n]) / ulp)))
    print(f"warp vs torch grid_sample: worst difference {worst} ulp of sum|w m|")
    assert worst <= 2 * MEASURED_ULP


MEASURED_ULP = 356.0


def test_warp_equals_torch_on_dyadic_inputs():
    """weights in quarters, integer values: every product and sum is exact, so any order and any contraction agree"""
    for seed, (N, H, W) in enumerate([(2, 8, 16), (3, 4, 4), (1, 32, 8)]):
        src = np.random.default_rng(seed).integers(-8, 9, (N, H, W)).astype(F)
        disp = fc.quarter_field((N, H, W, 2), seed, reach=3.0)
        yy, xx = np.mgrid[0:H, 0:W]
        grid = np.stack([(xx + disp[..., 0] + 0.5) * 2 / W - 1, (yy + disp[..., 1] + 0.5) * 2 / H - 1], axis=-1)
        assert np.array_equal(grid.astype(F).astype(np.float64), grid)          # the grid itself is exact
        ours_grid = fo.warp(src, grid.astype(F), "grid")
        assert np.array_equal(ours_grid, _grid_sample(src, grid.astype(F)))
        # "pixels" is "grid" on the normalised grid
        assert np.array_equal(fo.warp(src, disp, "pixels"), ours_grid)
        assert np.any(ours_grid != 0) and np.any(ours_grid != np.round(ours_grid))


def test_flow_loss_gradient_against_autograd():
    for seed, (b, t, h, w) in enumerate([(2, 3, 5, 7), (1, 2, 14, 14), (2, 4, 3, 3)]):
        x, field = fc.loss_inputs(b, t, h, w, seed, exact=False)
        ref = fo.flow_loss_f64(x, field, "pixels")
        assert ref["min_margin"] > 0
        ix, iy = fo.positions(field, h, w, "pixels")
        grid = np.stack([(ix.astype(np.float64) + 0.5) * 2 / w - 1, (iy.astype(np.float64) + 0.5) * 2 / h - 1], axis=-1)
        xt = torch.from_numpy(x).double().requires_grad_(True)
        warped = TF.grid_sample(xt[:, :-1].reshape(b * (t - 1), 1, h, w), torch.from_numpy(grid).reshape(-1, h, w, 2),
                                mode="bilinear", padding_mode="zeros", align_corners=False)
        loss = (warped.reshape(b, t - 1, h, w) - xt[:, 1:]).abs().mean()
        loss.backward()
        assert abs(ref["loss"] - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
        np.testing.assert_allclose(ref["dx"], xt.grad.numpy(), rtol=0, atol=1e-12)
        # the float32 evaluation in the kernel's order lies within the oracle's own bounds of it
        l32, dx32 = fo.flow_loss_ordered(x, field, "pixels")
        assert abs(float(l32) - ref["loss"]) <= ref["loss_bound"]
        assert np.all(np.abs(dx32 - ref["dx"]) <= ref["dx_bound"])


def test_flow_loss_exact_inputs_are_exactly_summable():
    """on the integer / quarter-pixel inputs the ordered float32 evaluation equals fp64 up to the final scale"""
    for b, t, h, w in [(2, 3, 14, 14), (1, 2, 1, 1), (1, 3, 32, 32)]:
        x, field = fc.loss_inputs(b, t, h, w, 5, exact=True)
        ref = fo.flow_loss_f64(x, field, "pixels")
        l32, dx32 = fo.flow_loss_ordered(x, field, "pixels")
        n = b * (t - 1) * h * w
        assert float(l32) == float(F(ref["loss"] * n) * (F(1) / F(n)))
        if h * w > 1:
            sg = dx32[0, 1, 0, 0]      # frame 1 pixel 0 of clip 0: d = 0 against frame 0
            assert ref["dx"].reshape(b, t, -1)[0, 1, 0] * 0 == 0 and not np.signbit(sg)


def test_flo_round_trip_bad_magic_and_reference_bytes(tmp_path, golden_dir):
    from avt_amd import flow

    uv = (np.arange(5 * 7 * 2, dtype=np.float64).reshape(5, 7, 2) / 8 - 3).astype(F)
    uv[1, 2] = (1e-3, -2.5e6)
    p = tmp_path / "a.flo"
    flow.write_flo(p, uv)
    back = flow.read_flo(p)
    assert back.dtype == F and back.shape == (5, 7, 2) and np.array_equal(back, uv)
    assert np.array_equal(fo.read_flo(p), uv)
    q = tmp_path / "b.flo"
    flow.write_flo(q, uv[:, :, 0], uv[:, :, 1])                 # the two-argument form
    fo.write_flo(tmp_path / "c.flo", uv)
    assert p.read_bytes() == q.read_bytes() == (tmp_path / "c.flo").read_bytes()
    # the reference's writeFlow wrote tests/golden/flow_5x7.flo from this very array
    with open(os.path.join(golden_dir, "flow_5x7.flo"), "rb") as f:
        assert p.read_bytes() == f.read()
    raw = bytearray(p.read_bytes())
    raw[0] ^= 1
    (tmp_path / "bad.flo").write_bytes(bytes(raw))
    with pytest.raises(ValueError, match="magic"):
        flow.read_flo(tmp_path / "bad.flo")
    (tmp_path / "short.flo").write_bytes(p.read_bytes()[:40])
    with pytest.raises(ValueError, match="bytes"):
        flow.read_flo(tmp_path / "short.flo")
    with pytest.raises(ValueError):
        flow.write_flo(tmp_path / "x.flo", uv[:, :, :1])


def test_injected_faults_are_told_apart():
    """each wrong reading changes the oracle's answer on inputs the GPU test uses"""
    H, W = 17, 33
    pred = fc.binary_maps(3, H, W, 1)
    rnd = fc.pixel_field("random", 2, H, W, 2)
    good = fo.consistency(pred, rnd, "pixels")
    assert not np.array_equal(fo.consistency(pred, rnd, "pixels", fault_swap_uv=True), good)
    assert not np.array_equal(fo.consistency(pred, rnd, "pixels", fault_no_padding=True), good)
    half = fc.pixel_field("half", 2, H, W, 0)
    board = fc.checkerboard(3, H, W)
    assert not np.array_equal(fo.consistency(board, half, "pixels", fault_gt=True),
                              fo.consistency(board, half, "pixels"))
    interior = fo.warp(board[:1], half[:1], "pixels")[0, :, :-1]
    assert np.all(interior == F(0.5))
    src = fc.float_maps(2, H, W, 3)
    g = fc.grid_field("random", 2, 9, 40, 4)
    assert not np.array_equal(fo.warp(src, g, "grid", fault_align_corners=True), fo.warp(src, g, "grid"))
    assert not np.array_equal(fo.warp(src, g, "grid", fault_no_padding=True), fo.warp(src, g, "grid"))
    assert not np.array_equal(fo.warp(src, rnd, "pixels", fault_swap_uv=True), fo.warp(src, rnd, "pixels"))
    fields = fc.color_fields()
    with pytest.raises(IndexError):                     # colour 56 does not exist: the wheel field reaches k0 = 55
        fo.flow2img(fields["wheel"], fault_no_wrap=True)
    # rad > 1 survives the normalisation only at the maximum-radius pixel, where u / maxrad + eps rounds above 1
    assert tuple(fo.flow2img(fields["wheel"])[0, 0]) == (191, 0, 0)
    assert tuple(fo.flow2img(fields["wheel"], fault_no_dim=True)[0, 0]) == (255, 0, 0)


def test_color_wheel_and_special_fields():
    from avt_amd import flow

    wheel = fo.color_wheel()
    assert wheel.shape == (55, 3) and np.array_equal(wheel, flow.WHEEL.numpy().astype(np.float64))
    fields = fc.color_fields()
    assert not fo.flow2img(fields["zero"]).any()                        # maxrad = 0: every pixel NaN, black
    f = fields["unknown_nan"]
    img = fo.flow2img(f)
    clean = f.copy()
    for y, x in ((2, 3), (4, 5), (6, 7), (8, 9)):
        assert not img[y, x].any()
        clean[y, x] = 0
    rest = np.ones(img.shape[:2], dtype=bool)
    rest[[2, 4, 6, 8], [3, 5, 7, 9]] = False
    assert np.array_equal(img[rest], fo.flow2img(clean)[rest]) and img[rest].any()
    # the wheel field shows each of the 55 colours (k0 from 1 to 55) and the wrap
    u, v, _ = fo.normalise(fields["wheel"])
    fk = fo.compute_color(u, v)[2]
    assert list(np.floor(fk[1]).astype(int)) == list(range(1, 56))
    assert np.all(np.abs(fk[1, :54] - np.floor(fk[1, :54]) - 0.5) < 1e-4) and np.all(fk[:, 54] == 55)
    before = f.copy()
    fo.flow2img(f)
    assert np.array_equal(before, f, equal_nan=True)


def test_color_fields_keep_the_excused_share_under_the_cap():
    """A condition on the inputs.  The pixel that attains the maximum radius has rad = 1 up to rounding and is always
    in the rad band; it is counted apart, and the other excused pixels stay within 1 % of the field."""
    assert 1e-11 < fo.DELTA < 1e-10
    for name, f in fc.color_fields().items():
        img, excused, alt = fo.flow2img_report(f)
        u, v, unknown = fo.normalise(f)
        rad = fo.compute_color(u, v)[1]
        at_max = excused & (np.abs(rad - 1) <= fo.DELTA_RAD)
        assert at_max.sum() <= 1, name
        assert (excused & ~at_max).sum() <= 0.01 * excused.size, (name, int(excused.sum()), excused.size)
        assert np.array_equal(alt[~at_max], img[~at_max])
