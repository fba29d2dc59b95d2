"""The instrument of the exact conv tests (tests/exactconv.py) checked on the CPU, no GPU:

  * every case of test_conv_exact_gpu.py and test_conv3d_exact_gpu.py passes the conditions under which its sums are
    exact in any order (this test sizes the draws);
  * the fp32 and the fp64 CPU references are equal -- the order-independence claim, checked once;
  * the off-grid cases of the domain files (exactconv.DOMAIN_*) pass the same conditions, and the generalised Case
    leaves the old cases' draws as they were (tests/golden/exactconv_draws.json);
  * sensitivity: fifteen faults, injected one at a time into a torch emulation of the conv (operands or index maps
    edited, no kernel), are each flagged by the equality comparator.  For the record the test prints whether the
    per-kernel files' old criterion (max|got - ref| / max|ref| < 8e-3, 2e-4 for a weight gradient) would have caught
    the same fault on its own kind of operands, a randn draw of the same shape; that is not asserted."""
import json
import os
import zlib

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


def test_old_cases_keep_their_draws():
    """The generalised Case leaves the draws of the two short tuple forms as they were: the CRC-32 of the operands'
    bytes for one strided, one c64 and two 3-D cases, recorded from the commit before the generalisation."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exactconv_draws.json")) as f:
        golden = json.load(f)
    assert len(golden) == 4
    for key, digests in golden.items():
        case = tuple(int(v) for v in key.strip("()").split(","))
        assert case in ec.STRIDED_CASES + ec.C64_CASES + ec.cases_3d(), case
        c = ec.Case(case)
        assert set(digests) == {"x", "w", "dy", "xg", "dyg"}
        for name, crc in digests.items():
            assert zlib.crc32(getattr(c, name).contiguous().numpy().tobytes()) == crc, (case, name)


DOMAIN = ([(c, ("y",)) for c in ec.DOMAIN_2D] + [(c, ("dx",)) for c in ec.DOMAIN_DGRAD]
          + [(c, ("dw",)) for c in ec.DOMAIN_WGRAD]
          + [(c, ("y", "dw") if ec.wgrad3d_ok(c) else ("y",)) for c in ec.DOMAIN_3D]
          + [(c, ("dx",)) for c in ec.DOMAIN_3D_DGRAD])


@pytest.mark.parametrize("case,kinds", DOMAIN, ids=lambda v: str(v) if isinstance(v, tuple) and len(v) > 3 else "")
def test_domain_conditions(case, kinds):
    """The same conditions, unrelaxed, for every off-grid case of the domain files and the kinds they compare; the
    shapes keep N <= 3, H, W <= 13, T <= 5."""
    c = ec.get_case(case)
    assert c.N <= 3 and c.H <= 13 and c.W <= 13 and c.T <= 5, case
    for kind in kinds:
        _show(case, kind, c.figures(kind))
        r64, r32 = c.ref(kind), c.ref(kind, torch.float32)
        assert torch.equal(r32.double(), r64), (case, kind)
    if "y" in kinds and not c.d3 and c.R * c.S <= 9:
        assert c.figures("y")["one_rounding_safe"], case  # whichever kernel takes the bias epilogue


def test_domain_lists_cover_the_issue():
    """The sweeps the lists promise: channel counts, tap shapes, pads, strides, the Bottleneck trio, M off the
    multiples of 64 and P*Q < 32."""
    f = [ec.get_case(c) for c in ec.DOMAIN_2D]
    assert {c.C for c in f} >= {32, 96, 160, 192, 320, 1024, 2048} and {c.K for c in f} >= {64, 192, 320, 384, 1024, 2048}
    assert {(c.R, c.S) for c in f} >= {(1, 1), (1, 3), (3, 1), (2, 2), (3, 3), (5, 5), (1, 7), (7, 7)}
    assert {c.pad for c in f} >= {0, 1, 2} and {c.st for c in f} == {1, 2}
    assert all(c.R * c.S == 1 or c.P * c.Q <= 16 for c in f if max(c.C, c.K) >= 1024)
    for st in (1, 2):
        assert {(c.C, c.K, c.R) for c in f if c.st == st} >= {(256, 64, 1), (64, 64, 3), (64, 256, 1)}
    assert any((c.N * c.P * c.Q) % 64 for c in f) and any(c.P * c.Q < 32 for c in f)
    d = [ec.get_case(c) for c in ec.DOMAIN_DGRAD]
    assert {c.C for c in d} >= {64, 192, 320, 1024} and {c.K for c in d} >= {32, 96, 160, 192, 2048}
    assert any(c.R != c.S and c.st == 2 for c in d) and any(c.R != c.S and c.st == 1 for c in d)
    w = [ec.get_case(c) for c in ec.DOMAIN_WGRAD]
    assert {c.Cw for c in w} >= {8, 16, 24, 40, 96, 160, 192} and {c.K for c in w} >= {64, 192, 320}
    assert {(c.R, c.S) for c in w} >= {(1, 1), (3, 3), (1, 3), (5, 5)} and len(ec.SPLIT_WGRAD) >= 2
    v = [ec.get_case(c) for c in ec.DOMAIN_3D]
    assert {(c.KT, c.R, c.S) for c in v} >= {(3, 3, 3), (1, 3, 3), (3, 1, 1), (1, 1, 1), (2, 2, 2), (5, 3, 3)}
    assert {c.pad_t for c in v} >= {0, 1, 2} and {c.C for c in v} >= {32, 96, 192} and {c.K for c in v} >= {64, 192}
    assert any((c.KT, c.R, c.S, c.st) == (1, 1, 1, 2) for c in v)
    g = [ec.get_case(c) for c in ec.DOMAIN_3D_DGRAD]
    assert {c.C for c in g} >= {64, 192} and {c.K for c in g} >= {32, 96, 192}


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


# faults only a shape off the ResNet-18 grid can show, on the cases of the domain files
C96 = (1, 5, 6, 96, 192, 3, 3, 1, 1)
R1S3 = (3, 7, 9, 192, 384, 1, 3, 1, 1)
COLS216 = (2, 8, 8, 24, 64, 3, 3, 1, 1)
PADT2 = (2, 3, 7, 6, 96, 64, 3, 3, 3, 1, 2, 0)


def _fault_last_32_channels_dropped(c):
    assert c.C % 64 == 32
    x = c.x.clone()
    x[..., c.C - 32:] = 0  # a 64-deep k-tile walked over C // 64 whole chunks only
    return c.conv(x, c.w), c.ref("y"), False


def _shifted_taps(c, swap):
    """A stride-1 2-D forward as a sum over taps of the input displaced by (r - pad, s - pad), zero outside the image;
    swap: the displacement built as (s - pad, r - pad)."""
    m = max(c.R, c.S) + c.pad
    xp = F.pad(c.x.double(), (0, 0, m, m, m, m))
    y = torch.zeros(c.N, c.P, c.Q, c.K, dtype=torch.float64)
    for r in range(c.R):
        for s in range(c.S):
            dy, dx = (s - c.pad, r - c.pad) if swap else (r - c.pad, s - c.pad)
            y += xp[:, m + dy:m + dy + c.P, m + dx:m + dx + c.Q, :] @ c.w[:, r, s, :].double().T
    return y


def _fault_r_s_swapped_in_displacement(c):
    assert c.R != c.S and c.st == 1
    if c.exact:
        assert torch.equal(_shifted_taps(c, False), c.ref("y"))  # the emulation is the conv
    return _shifted_taps(c, True), c.ref("y"), False


def _fault_wgrad_tail_columns_zeroed(c):
    ncols = c.R * c.S * c.Cw
    assert ncols % 128 and ncols > 128
    dw = c.ref("dw").clone().reshape(c.K, ncols)
    dw[:, ncols // 128 * 128:] = 0  # the partial last 128-column tile never stored
    return dw.reshape(c.ref("dw").shape), c.ref("dw"), True


def _fault_pad_t_applied_as_pad(c):
    assert c.d3 and c.pad_t != c.pad
    xp = F.pad(c.x.double(), (0, 0, 0, 0, 0, 0, c.pad, 2 * c.pad_t - c.pad))  # frames displaced by kt - pad
    y = c._cl(F.conv3d(c._cf(xp), c.w.double(), stride=(1, c.st, c.st), padding=(0, c.pad, c.pad)))
    return y, c.ref("y"), False


def _fault_k192_last_tile_from_previous(c):
    assert c.K == 192
    y = c.ref("y").clone()
    y[..., 128:] = y[..., 64:128]  # the third 64-wide column tile addressed as the second
    return y, c.ref("y"), False


FAULTS = {
    "the last 32 channels of every tap dropped at C % 64 == 32": (_fault_last_32_channels_dropped, C96),
    "R and S swapped in the tap displacement": (_fault_r_s_swapped_in_displacement, R1S3),
    "the wgrad columns past the last full 128 zeroed": (_fault_wgrad_tail_columns_zeroed, COLS216),
    "pad_t applied as pad": (_fault_pad_t_applied_as_pad, PADT2),
    "the last 64 output channels of a K = 192 conv taken from the tile before": (_fault_k192_last_tile_from_previous, C96),
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
