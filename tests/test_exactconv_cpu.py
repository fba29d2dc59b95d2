"""The instrument of the exact conv tests (tests/exactconv.py) checked on the CPU, no GPU:

  * every case of test_conv_exact_gpu.py and test_conv3d_exact_gpu.py passes the conditions under which its sums are
    exact in any order (this test sizes the draws);
  * the fp32 and the fp64 CPU references are equal -- the order-independence claim, checked once;
  * sensitivity: ten faults, injected one at a time into a torch emulation of the conv (operands or index maps
    edited, no kernel), are each flagged by the equality comparator.  For the record the test prints whether the
    per-kernel files' old criterion (max|got - ref| / max|ref| < 8e-3, 2e-4 for a weight gradient) would have caught
    the same fault on its own kind of operands, a randn draw of the same shape; that is not asserted."""
import pytest
import torch
import torch.nn.functional as F

import exactconv as ec

KINDS = ("y", "dx", "dw")


def _show(case, kind, fig):
    print(case, kind, {k: (round(v, 5) if isinstance(v, float) else v) for k, v in fig.items()})


@pytest.mark.parametrize("case", ec.cases_2d() + ec.STEM_CASES + ec.cases_3d(), ids=str)
def test_conditions_and_order_independence(case):
    """The conditions of exactconv's docstring for forward, dgrad and wgrad draws of the case; fp32 == fp64."""
    c = ec.get_case(case)
    for kind in KINDS:
        _show(case, kind, c.figures(kind))
        r64, r32 = c.ref(kind), c.ref(kind, torch.float32)
        assert r32.dtype == torch.float32 and torch.equal(r32.double(), r64), (case, kind)
    if len(case) == 8 and case[3] == case[4] == 64 and case[5] == 3:
        # the layer-1 kernel's bias epilogue rounds once, the others twice: both must be the identity
        assert c.figures("y")["one_rounding_safe"], case


@pytest.mark.parametrize("shape", ec.VIDEO_STEM_SHAPES, ids=str)
def test_video_stem_conditions(shape):
    v = ec.get_video_stem(shape)
    for kind in KINDS:
        _show(shape, kind, v.fig[kind])
    assert v.y.shape[-1] == 64 and v.dx.shape == v.video.shape and v.dw.shape == v.w.shape


def test_dgrad_bn_operands_stay_exact():
    """The chosen BN statistics keep the epilogue's products multiples of 1/4 and its sums below 2^24."""
    for case in ec.cases_2d():
        c = ec.get_case(case)
        g = ec.rne2(c.ref("dx"), c.add)
        xc = ec.ints(c.x.shape, -3, 3, case, "xc")
        xc2 = ec.ints(c.x.shape, -3, 3, case, "xc2")
        st, st2 = ec.exact_bn_stats(c.C, (case, 1)), ec.exact_bn_stats(c.C, (case, 2))
        gm, s1, s2, s3 = ec.dgrad_bn_ref(g, xc, st, None, xc2, st2)
        for s in (s1, s2, s3):
            assert torch.equal(s * 4, (s * 4).round()) and torch.equal(s.float().double(), s)
        assert 0.2 < float((gm != 0).double().mean()) / max(float((g != 0).double().mean()), 1e-9) < 0.8  # a real mask


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity
# ---------------------------------------------------------------------------------------------------------------------
def _taps_fwd(c, x, w, pad_value=None):
    """A 2-D forward as explicit per-tap GEMMs over a padded input (rows x taps), so that index maps can be edited:
    returns (cols [rows][R*R][C], wt [K][R*R][C]); y = einsum('rtc,ktc->rk')."""
    xp = F.pad(x.double(), (0, 0, c.pad, c.pad, c.pad, c.pad))
    if pad_value is not None:
        xp = pad_value(xp)
    cols = []
    for r in range(c.R):
        for s in range(c.R):
            cols.append(xp[:, r:r + c.st * (c.P - 1) + 1:c.st, s:s + c.st * (c.Q - 1) + 1:c.st, :].reshape(-1, c.C))
    return torch.stack(cols, 1), w.double().reshape(c.K, c.R * c.R, c.C)


def _emu_fwd(c, cols, wt):
    return torch.einsum("rtc,ktc->rk", cols, wt).reshape(c.N, c.P, c.Q, c.K)


def _judge(name, case, fault):
    """Is the fault flagged by equality on the exact operands?  And, for the record, by the old relative bound on the
    old kind of operands (a randn draw of the same shape)?  The device would hand back bf16_rne(.) / fp32(.)."""
    faulty, ref, fp32 = fault(ec.get_case(case))
    assert not torch.equal(faulty, ref), f"{name}: the injected fault changed nothing"
    got, want = (faulty.float().double(), ref) if fp32 else (ec.bf16_rne(faulty), ec.bf16_rne(ref))
    flagged = bool(ec.mismatches(got, want))
    n = int((got != want).sum())
    faulty_r, ref_r, _ = fault(ec.RandnCase(case))
    got_r = faulty_r.float().double() if fp32 else ec.bf16_rne(faulty_r)
    tol = 2e-4 if fp32 else 8e-3
    rel = ((got_r - ref_r).abs().max() / ref_r.abs().max()).item()
    print(f"fault {name!r} on {case}: {n} outputs differ, equality flags it: {flagged}; on a randn draw of the shape "
          f"the old criterion measures rel_err {rel:.2e} against {tol:g}: {'caught' if rel >= tol else 'MISSED'}")
    return flagged


BIG = (2, 17, 19, 512, 512, 3, 1, 1)
MID = (3, 14, 14, 256, 256, 3, 1, 1)
S2 = (2, 9, 11, 64, 128, 3, 2, 1)
STEM = ec.STEM_CASES[0]
CLIP = (3, 5, 28, 28, 128, 128, 1)


def _fault_chunk_dropped(c):
    cols, wt = _taps_fwd(c, c.x, c.w)
    if c.exact:
        assert torch.equal(_emu_fwd(c, cols, wt), c.ref("y"))  # the emulation is the conv
    row, tap = 127, 4  # the last row of the first 128-row tile, the centre tap, channels 8..15
    y = c.ref("y").clone().reshape(-1, c.K)
    y[row] -= cols[row, tap, 8:16] @ wt[:, tap, 8:16].T
    return y.reshape(c.ref("y").shape), c.ref("y"), False


def _fault_taps_swapped(c):
    w = c.w.clone()
    w[5] = c.w[5].transpose(0, 1)  # (r, s) <-> (s, r) for output channel 5
    return c.conv(c.x, w), c.ref("y"), False


def _fault_halo_wraps(c):

    def wrap(xp):  # the right pad column of image row h holds the first pixel of row h + 1 (the next address)
        xp = xp.clone()
        xp[:, c.pad:c.pad + c.H - 1, c.pad + c.W, :] = xp[:, c.pad + 1:c.pad + c.H, c.pad, :]
        return xp

    cols, wt = _taps_fwd(c, c.x, c.w, wrap)
    return _emu_fwd(c, cols, wt), c.ref("y"), False


def _fault_clip_end_reads_next_clip(c):
    xp = F.pad(c.x.double(), (0, 0, 0, 0, 0, 0, 1, 1))  # time padded by hand
    if c.exact:
        assert torch.equal(c._cl(F.conv3d(c._cf(xp), c.w.double(), stride=(1, c.st, c.st), padding=(0, 1, 1))), c.ref("y"))
    xp[:-1, c.T + 1] = c.x[1:, 0].double()  # past the last frame of clip n lies frame 0 of clip n + 1
    y = c._cl(F.conv3d(c._cf(xp), c.w.double(), stride=(1, c.st, c.st), padding=(0, 1, 1)))
    return y, c.ref("y"), False


def _fault_chunk_in_two_splits(c):
    x, w = c.x.clone(), c.w.clone()
    x[..., 64:], w[..., 64:] = 0, 0  # the first 64-channel k-chunk, counted once more
    return c.ref("y") + c.conv(x, w), c.ref("y"), False


def _fault_last_ktile_skipped(c):
    npix = c.N * c.P * c.Q
    assert npix % 32, "the case needs a partial last k-tile"
    dy = c.dyg.clone().reshape(npix, c.K)
    dy[npix // 32 * 32:] = 0
    return c.conv_weight(c.xg, dy.reshape(c.dyg.shape)), c.ref("dw"), True


def _fault_parity_class_taps(c):
    other = c.conv_input(c.dy, torch.roll(c.w, 1, dims=2))  # the taps of the class one column over
    dx = c.ref("dx").clone()
    dx[:, 0::2, 0::2] = other[:, 0::2, 0::2]
    return dx, c.ref("dx"), False


def _fault_add_twice(c):
    want = ec.rne2(c.ref("dx"), c.add)
    return ec.rne2(ec.rne2(c.ref("dx"), c.add), c.add), want, False


def _fault_mask_bits_reversed(c):
    keep = ec.mask_from_bits(c.bits, c.x.shape)
    rev = keep.reshape(-1, 8).flip(1).reshape(c.x.shape)
    zero = torch.zeros_like(c.add)
    want = ec.rne2(c.ref("dx"), torch.where(keep, c.add, zero))
    return ec.rne2(c.ref("dx"), torch.where(rev, c.add, zero)), want, False


def _fault_stem_pad_channel(c):
    # the fourth (padding) channel of the Cp = 4 operands read as data: ones against a copy of channel 0's weights
    x4 = torch.cat([c.x, torch.ones_like(c.x[..., :1]) * c.x.max()], -1)
    w4 = torch.cat([c.w, c.w[..., :1]], -1)
    y = F.conv2d(x4.double().permute(0, 3, 1, 2), w4.double().permute(0, 3, 1, 2), stride=2, padding=3)
    return y.permute(0, 2, 3, 1).contiguous(), c.ref("y"), False


FAULTS = {
    "one 8-channel chunk of one tap dropped in a 128-row tile's last row": (_fault_chunk_dropped, BIG),
    "taps (r, s) and (s, r) swapped for one output channel": (_fault_taps_swapped, MID),
    "right halo column at w = W-1 reads the next row's first pixel": (_fault_halo_wraps, MID),
    "last frame of clip n reads frame 0 of clip n+1": (_fault_clip_end_reads_next_clip, CLIP),
    "one k-chunk counted in two split-K partials": (_fault_chunk_in_two_splits, BIG),
    "last partial 32-pixel k-tile of a wgrad skipped": (_fault_last_ktile_skipped, MID),
    "a stride-2 parity class uses the neighbouring class's taps": (_fault_parity_class_taps, S2),
    "add applied twice": (_fault_add_twice, MID),
    "mask bits of avt_conv2d_dgrad_mask reversed within a byte": (_fault_mask_bits_reversed, MID),
    "the stem's padded fourth channel read as non-zero": (_fault_stem_pad_channel, STEM),
}


@pytest.mark.parametrize("name", list(FAULTS), ids=lambda n: n.replace(" ", "_")[:48])
def test_fault_is_flagged(name):
    fault, case = FAULTS[name]
    assert _judge(name, case, fault), name


def test_comparator_reports_and_zero_signs():
    """-0 equals +0, a NaN never passes, and a report names the index, the values and the edges it lies on."""
    ref = torch.zeros(1, 2, 3, 8, dtype=torch.float64)
    got = torch.zeros(1, 2, 3, 8).to(torch.bfloat16)
    got[0, 1, 2, 7] = -0.0
    ec.assert_bf16(got, ref)
    got[0, 1, 2, 7] = float("nan")
    with pytest.raises(AssertionError, match=r"1 of 48 elements differ \(1 NaN\)"):
        ec.assert_bf16(got, ref)
    got[0, 1, 2, 7] = 1.0
    with pytest.raises(AssertionError, match=r"\(0, 1, 2, 7\): got 1.0 want 0.0.*h=last,w=last.*c%8=last"):
        ec.assert_bf16(got, ref)
    with pytest.raises(AssertionError):
        ec.assert_fp32(torch.full((2, 2), 0.25), torch.full((2, 2), 0.25, dtype=torch.float64) + 2.0 ** -20)
    assert ec.bf16_rne(torch.tensor([257.0, 258.0, 259.0, 261.0])).tolist() == [256.0, 258.0, 260.0, 260.0]  # RNE
