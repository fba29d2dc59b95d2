"""The Conv3d family pinned term by term, as tests/test_conv_exact_gpu.py pins the 2-D one: avt_conv3d_fwd / _fwd_bias /
_dgrad / _wgrad on the geometry edges of test_r3d_backward_gpu.py's CASES, and the video stem as R3DTrunk launches it
(avt_video_stem_im2col + the packed stem conv, its folded wgrad + avt_stem3d_wgrad_unfold, avt_video_stem_dgrad in both
forms) -- on operands whose sums are exact in fp32 in any order (tests/exactconv.py), compared for EQUALITY with the
fp64 torch reference.  No tolerance other than the BN accumulator's M2 column.  Each test prints the number of distinct
plans it ran and the share of outputs above 255."""
import ctypes

import pytest
import torch

import exactconv as ec
from avt_amd._lib import call, lib, query

pytestmark = pytest.mark.gpu
DEV = "cuda"
P, S, Knobs, _tag = ec.P, ec.S, ec.Knobs, ec.tag


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    ec.KEEP.clear()


SWEEP = ec.SWEEP_3D  # shared with test_conv3d_domain_gpu.py
CASES = ec.cases_3d()
SPLIT_CASES = CASES[7:9]
_OPS = {}
_RAN = {}


def _nan(*shape, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _ops(case):
    if case not in _OPS:
        c = ec.get_case(case)
        w = c.w.to(DEV)
        taps = c.KT * c.R * c.S
        wp = torch.empty(c.K, taps * c.C, device=DEV, dtype=torch.bfloat16)
        wt = torch.empty(c.C, taps * c.K, device=DEV, dtype=torch.bfloat16)
        call("avt_pack_conv3d_weight", P(w), P(wp), c.K, c.C, c.KT, c.R, c.S, 0, S())
        if c.K % 64 == 0:
            call("avt_pack_conv3d_weight_dgrad", P(w), P(wt), c.K, c.C, c.KT, c.R, c.S, S())
        else:  # the pack kernel takes K % 64 == 0, avt_conv3d_dgrad K % 32 == 0: the same layout by hand (include/avt.h)
            wt = w.flip(2, 3, 4).permute(1, 2, 3, 4, 0).reshape(c.C, taps * c.K).to(torch.bfloat16).contiguous()
        torch.cuda.synchronize()
        bf = lambda t: t.to(torch.bfloat16).to(DEV)
        _OPS[case] = dict(wp=wp, wt=wt, x=bf(c.x), xg=bf(c.xg), dy=bf(c.dy), dyg=bf(c.dyg), add=bf(c.add),
                          res=bf(c.res), bias=c.bias.to(DEV))
    return _OPS[case]


def _geo(c):
    return (c.N, c.T, c.H, c.W, c.C, c.K, c.KT, c.R, c.S, c.st, c.pad_t, c.pad)


def _plans(case, epi, dgrad=False):
    """[(plan, setting)] of SWEEP's settings with distinct avt_conv_fwd_plan tuples (T and KT set; a stride-1 dgrad is
    the forward of dy with C and K swapped)."""
    c = ec.get_case(case)
    return ec.fwd_plans(c, c.C, SWEEP, epi, dgrad)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_conv3d_fwd_every_plan(case, record=True):
    """avt_conv3d_fwd with its BN accumulator under every distinct plan of the sweep, and avt_conv3d_fwd_bias with a
    residual and ReLU (the fp32 bias joins the accumulator before the first rounding, residual and ReLU the rounded
    value: DESIGN 6l)."""
    c = ec.get_case(case)
    fig = c.figures("y")
    o = _ops(case)
    ref = c.ref("y")
    plans = _plans(case, 0)
    for plan, setting in plans:
        with Knobs(setting):
            y = _nan(c.N, c.To, c.P, c.Q, c.K)
            acc = _nan(int(query("avt_bn_acc_doubles", c.N * c.To * c.P * c.Q, c.K)), dtype=torch.float64)
            call("avt_conv3d_fwd", P(o["x"]), P(o["wp"]), P(y), P(acc), *_geo(c), S())
            torch.cuda.synchronize()
            what = f"conv3d_fwd {case} [{_tag(setting)}] plan {plan}"
            ec.assert_bf16(y, ref, what)
            ec.assert_fwd_acc(acc, ref, what)
    fams = {p[0] for p, _ in plans}
    if record:  # (test_conv3d_domain_gpu.py runs this body on its own cases)
        _RAN[case] = fams
    v = ec.bf16_rne(ref + c.bias.double())
    want = {False: v, True: ec.bf16_rne(v + c.res.double()).clamp_min(0)}
    bplans = _plans(case, 2)
    for plan, setting in bplans:
        with Knobs(setting):
            for full in (False, True):
                y = _nan(c.N, c.To, c.P, c.Q, c.K)
                call("avt_conv3d_fwd_bias", P(o["x"]), P(o["wp"]), P(y), *_geo(c), P(o["bias"]),
                     P(o["res"]) if full else None, int(full), S())
                torch.cuda.synchronize()
                ec.assert_rounded(y, want[full], f"conv3d_fwd_bias {case} [{_tag(setting)}] plan {plan} res+relu={full}")
    print(f"conv3d fwd {case}: {len(plans)} + {len(bplans)} (bias) distinct plans, families {sorted(fams)}, "
          f"above 255: {fig['above255']:.2e}")


def test_three_patch_family_is_reached():
    """Family 2 of avt_conv_fwd_plan (the halo kernel's Conv3d three-patch form) and family 3 (the tap gather's Conv3d
    form) each run on at least one case of test_conv3d_fwd_every_plan."""
    fams = set()
    for case in CASES:
        fams |= {p[0] for p, _ in _plans(case, 0)}
    assert fams >= {2, 3}, fams
    if len(_RAN) == len(CASES):
        assert set().union(*_RAN.values()) >= {2, 3}, _RAN


@pytest.mark.parametrize("case", CASES, ids=str)
def test_conv3d_dgrad_exact(case):
    """avt_conv3d_dgrad plain, + add and in place (the add joining the rounded result), on the default form of the
    shape (avt_set_halo3d(-1)) and, at stride 1, on every other distinct plan of the sweep (the tap gather included)."""
    c = ec.get_case(case)
    fig = c.figures("dx")
    o = _ops(case)
    plain, added = ec.bf16_rne(c.ref("dx")), ec.rne2(c.ref("dx"), c.add)
    settings = _plans(case, 0, dgrad=True) if c.st == 1 else [(None, [])]
    for plan, setting in settings:
        with Knobs(setting):
            dx, dxa = _nan(*c.x.shape), _nan(*c.x.shape)
            dxi = o["add"].clone()
            for out, add in ((dx, None), (dxa, o["add"]), (dxi, dxi)):
                call("avt_conv3d_dgrad", P(o["dy"]), P(o["wt"]), P(out), P(add), *_geo(c), S())
            torch.cuda.synchronize()
            what = f"{case} [{_tag(setting)}] plan {plan}"
            ec.assert_rounded(dx, plain, "conv3d_dgrad " + what)
            ec.assert_rounded(dxa, added, "conv3d_dgrad + add " + what)
            ec.assert_rounded(dxi, added, "conv3d_dgrad in place " + what)
    print(f"conv3d dgrad {case}: {len(settings)} distinct plans, above 255: {fig['above255']:.2e}")


@pytest.mark.parametrize("case", CASES, ids=str)
def test_conv3d_wgrad_exact(case):
    """avt_conv3d_wgrad into a 0.25 pre-fill == the fp64 conv3d_weight + 0.25 exactly; the two split cases reach >= 2
    splits (asserted from the workspace size, as test_conv3d_wgrad does)."""
    c = ec.get_case(case)
    fig = c.figures("dw")
    o = _ops(case)
    wsb = int(query("avt_conv3d_wgrad_workspace", *_geo(c)))
    assert wsb > 0
    Ng = (c.KT * c.R * c.S * c.C + 127) // 128 * 128  # slab bytes = splits * K * Ng * 4
    if case in SPLIT_CASES:
        assert wsb % (c.K * Ng * 4) == 0 and wsb // (c.K * Ng * 4) >= 2, (wsb, c.K, Ng)
    ws = _nan(wsb // 4, dtype=torch.float32)  # any contents
    dw = torch.full((c.K, c.C, c.KT, c.R, c.S), ec.PREFILL, device=DEV)
    rc = lib().avt_conv3d_wgrad(P(o["xg"]), P(o["dyg"]), P(dw), *_geo(c), P(ws), wsb, S())
    assert rc == 0, lib().avt_last_error()
    torch.cuda.synchronize()
    ec.assert_fp32(dw, c.ref("dw") + ec.PREFILL, f"conv3d_wgrad {case} ({wsb // (c.K * Ng * 4)} slab splits); index "
                   "(k, c, kt, r, s)", channels_last=False)
    print(f"conv3d wgrad {case}: {wsb // (c.K * Ng * 4)} slab splits, max |dw| {fig['max_abs']:.0f}")


# ---------------------------------------------------------------------------------------------------------------------
# the video stem
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ec.VIDEO_STEM_SHAPES, ids=str)
def test_video_stem_exact(shape):
    """Conv3d(3, 64, 7x7x7, s(1, 2, 2), p3) on an integer video: im2col + the packed 49-tap conv (with its BN
    accumulator), the folded wgrad + avt_stem3d_wgrad_unfold into a 0.25 pre-fill, and avt_video_stem_dgrad in both
    forms (fp32 out) -- every one the fp64 answer exactly, so both dgrad forms the same."""
    b, T, H, W = shape
    v = ec.get_video_stem(shape)
    Ho, Wo = v.P, v.Q
    w = v.w.to(DEV)
    wp = torch.empty(64, 49 * 32, device=DEV, dtype=torch.bfloat16)
    call("avt_pack_conv3d_weight", P(w), P(wp), 64, 3, 7, 7, 7, 1, S())
    x = _nan(b, T, H, W, 32)
    call("avt_video_stem_im2col", P(v.video.to(DEV)), P(x), b, 3, T, H, W, 7, 3, S())
    y = _nan(b * T, Ho, Wo, 64)
    acc = _nan(int(query("avt_bn_acc_doubles", b * T * Ho * Wo, 64)), dtype=torch.float64)
    call("avt_conv2d_fwd", P(x), P(wp), P(y), P(acc), b * T, H, W, 32, 64, 7, 7, 2, 3, 49 * 32, S())
    torch.cuda.synchronize()
    ref = v.y.reshape(b * T, Ho, Wo, 64)
    ec.assert_bf16(y, ref, f"video stem forward {shape}")
    ec.assert_fwd_acc(acc, ref, f"video stem forward {shape}")
    # weight gradient: the 2-D wgrad over the folded input of the {0..3} video, unfolded into OIDHW
    xg = _nan(b, T, H, W, 32)
    call("avt_video_stem_im2col", P(v.videog.to(DEV)), P(xg), b, 3, T, H, W, 7, 3, S())
    dwf = torch.zeros(64, 7, 7, 32, device=DEV)
    wsb = int(query("avt_conv2d_wgrad_workspace", b * T, H, W, 32, 32, 64, 7, 7, 2, 3))
    ws = _nan(max(wsb // 4, 4), dtype=torch.float32)
    call("avt_conv2d_wgrad", P(xg), P(v.dyg.to(torch.bfloat16).to(DEV)), P(dwf), b * T, H, W, 32, 32, 64, 7, 7, 2, 3,
         P(ws), wsb, S())
    dw = torch.full((64, 3, 7, 7, 7), ec.PREFILL, device=DEV)
    call("avt_stem3d_wgrad_unfold", P(dwf), P(dw), 64, 3, 7, 7, 7, S())
    torch.cuda.synchronize()
    ec.assert_fp32(dw, v.dw + ec.PREFILL, f"video stem wgrad {shape}; index (k, c, kt, r, s)", channels_last=False)
    # input gradient, both forms
    gy = v.dy.to(torch.bfloat16).to(DEV)
    wpk = torch.empty(int(query("avt_video_stem_dgrad_pack_bytes")), device=DEV, dtype=torch.uint8)
    call("avt_pack_video_stem_dgrad", P(w), P(wpk), S())
    for form in (0, 1):
        with Knobs([("avt_set_video_stem_dgrad", form)]):
            gx = _nan(b, 3, T, H, W, dtype=torch.float32)
            call("avt_video_stem_dgrad", P(gy), P(w) if form == 0 else None, P(wpk) if form == 1 else None, P(gx), b, T,
                 H, W, S())
            torch.cuda.synchronize()
            ec.assert_fp32(gx, v.dx, f"video stem dgrad form {form} {shape}; index (n, c, t, h, w)", channels_last=False)
    print(f"video stem {shape}: forward above 255: {v.fig['y']['above255']:.2e}, max |dw| {v.fig['dw']['max_abs']:.0f}, "
          f"max |dx| {v.fig['dx']['max_abs']:.0f}")
