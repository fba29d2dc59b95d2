"""avt_conv3d_fwd_bias -- y = [relu](conv3d(x, w) + bias[k] (+ residual)) -- in every kernel form avt_conv3d_fwd's
planner picks for an R3D-18 shape (the halo kernel's three-patch form on its three tiles, the tap-gather kernel's
Conv3d form at stride 1 and 2, the 49-tap folded video stem), against fp64 F.conv3d on the identical bf16 operands.
Each form is forced with avt_set_halo3d (restored afterwards) at the smallest shapes that cross its edges (taken from
test_tube_gpu.CONV3D_CASES, which the plain forward passes); the bound is the project's own for conv outputs, 8e-3 of
the output's largest magnitude."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL = 8e-3

# (form, avt_set_halo3d value, (N, T, H, W, C, K, stride))
CASES = [
    ("halo336", 2, (2, 4, 9, 11, 128, 128, 1)),  # clip ends inside a tile, ragged M
    ("halo336", 2, (1, 2, 5, 39, 128, 128, 1)),
    ("halo336", 2, (3, 1, 14, 14, 128, 256, 1)),  # T = 1
    ("halo416", 2, (1, 2, 5, 40, 128, 128, 1)),
    ("halo416", 2, (1, 2, 5, 79, 128, 128, 1)),
    ("halo488", 2, (3, 2, 21, 30, 64, 64, 1)),
    ("halo488", 2, (1, 2, 5, 115, 64, 64, 1)),
    ("gather_s1", 2, (1, 2, 5, 80, 128, 128, 1)),  # past the halo limits under the default knob
    ("gather_s1", 2, (1, 2, 5, 116, 64, 64, 1)),
    ("gather_s1", 0, (1, 2, 3, 3, 512, 512, 1)),
    ("gather_s1", 0, (2, 4, 9, 11, 128, 128, 1)),
    ("gather_s2", 2, (2, 4, 9, 11, 64, 128, 2)),
    ("gather_s2", 2, (1, 5, 7, 6, 128, 256, 2)),
    ("one_column", 2, (20, 4, 2, 1, 64, 128, 1)),
    ("one_column", 0, (20, 4, 2, 1, 64, 128, 1)),
]
STEM_CASES = [(2, 1, 9, 8), (1, 3, 16, 16)]  # video (b, T, H, W)
# what a form's name claims of avt_conv_fwd_plan's answer (include/avt_tuning.h): the family (2 the halo kernel's
# three-patch form, 3 tap gather) and the halo form's patch rows; "one_column" runs whichever avt_set_halo3d leaves
NAMED = {"halo336": (2, 336), "halo416": (2, 416), "halo488": (2, 488), "gather_s1": (3, None), "gather_s2": (3, None)}
MODES = ["bias", "bias_relu", "bias_res_relu"]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Halo3d:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        from avt_amd._lib import call

        call("avt_set_halo3d", self.v)

    def __exit__(self, *exc):
        from avt_amd._lib import call

        call("avt_set_halo3d", -1)


_OPS = {}


def _operands(shape):
    """Seeded bf16 operands of a 3x3x3 shape, packed by the library, and the fp64 conv of exactly those values."""
    if shape not in _OPS:
        from avt_amd._lib import call

        N, T, H, W, C, K, st = shape
        g = torch.Generator().manual_seed(sum(shape) + 7 * H)
        x = torch.randn(N, T, H, W, C, generator=g).to(torch.bfloat16)
        w = (torch.randn(K, C, 3, 3, 3, generator=g) / (27 * C) ** 0.5).to(torch.bfloat16)
        bias = torch.randn(K, generator=g)
        ref = F.conv3d(x.double().permute(0, 4, 1, 2, 3), w.double(), stride=(1, st, st), padding=1)
        ref = ref.permute(0, 2, 3, 4, 1).contiguous()
        res = torch.randn(ref.shape, generator=g).to(torch.bfloat16)
        wd = w.float().to(DEV)
        wp = torch.empty(K, 27 * C, device=DEV, dtype=torch.bfloat16)
        call("avt_pack_conv3d_weight", _p(wd), _p(wp), K, C, 3, 3, 3, 0, _stream())
        torch.cuda.synchronize()
        _OPS[shape] = (x.to(DEV), wp, bias.to(DEV), res.to(DEV), ref)
    return _OPS[shape]


def _run(shape, x, wp, bias, res, relu, plain=False):
    from avt_amd._lib import call

    N, T, H, W, C, K, st = shape
    Ho, Wo = (H + 2 - 3) // st + 1, (W + 2 - 3) // st + 1
    y = torch.full((N, T, Ho, Wo, K), float("nan"), device=DEV, dtype=torch.bfloat16)
    if plain:
        call("avt_conv3d_fwd", _p(x), _p(wp), _p(y), None, N, T, H, W, C, K, 3, 3, 3, st, 1, 1, _stream())
    else:
        call("avt_conv3d_fwd_bias", _p(x), _p(wp), _p(y), N, T, H, W, C, K, 3, 3, 3, st, 1, 1, _p(bias), _p(res),
             int(relu), _stream())
    torch.cuda.synchronize()
    return y


def _check(tag, y, ref, bias, res, mode):
    want = ref + bias.cpu().double()
    if mode == "bias_res_relu":
        want = want + res.cpu().double()
    if mode != "bias":
        want = want.clamp_min(0)
    got = y.cpu().double()
    assert torch.isfinite(got).all()  # no NaN of the pre-fill left, none made
    err = (got - want).abs().max().item()
    scale = want.abs().max().item()
    print(f"{tag} {mode}: max err {err:.3e} = {err / scale:.2e} of max |out| {scale:.3f}")
    assert err <= TOL * scale


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form,halo3d,shape", CASES)
def test_bias_epilogue_vs_fp64(form, halo3d, shape, mode):
    """Each form, three modes: within 8e-3 of the fp64 result's largest magnitude everywhere, no NaN left."""
    x, wp, bias, res, ref = _operands(shape)
    with Halo3d(halo3d):
        y = _run(shape, x, wp, bias, res if mode == "bias_res_relu" else None, mode != "bias")
    _check(f"{form} halo3d={halo3d} {shape}", y, ref, bias, res, mode)


@pytest.mark.parametrize("form,halo3d,shape", CASES)
def test_zero_bias_is_the_plain_forward(form, halo3d, shape):
    """bias = 0, no residual, no ReLU: bitwise avt_conv3d_fwd on the same operands -- one main loop, one tile store."""
    x, wp, bias, _, _ = _operands(shape)
    with Halo3d(halo3d):
        y = _run(shape, x, wp, torch.zeros_like(bias), None, False)
        y0 = _run(shape, x, wp, None, None, False, plain=True)
    assert torch.equal(y.view(torch.int16), y0.view(torch.int16))


@pytest.mark.parametrize("form,halo3d,shape", CASES)
def test_case_runs_the_form_it_names(form, halo3d, shape):
    """The planner's own account of the call (avt_conv_fwd_plan under the case's knob): the family and patch rows the
    form's name claims, on the bias epilogue's Conv3d form."""
    from avt_amd._lib import call

    N, T, H, W, C, K, st = shape
    plan = (ctypes.c_int * 10)()
    with Halo3d(halo3d):
        call("avt_conv_fwd_plan", N, T, H, W, C, K, 3, 3, 3, st, 1, 1, 2, plan)
    family, rows_or_bk, opt, ksplit, epi = plan[0], plan[6], plan[7], plan[8], plan[9]
    want_family, want_rows = NAMED.get(form, (2 if halo3d else 3, None))
    assert (family, ksplit, epi) == (want_family, 1, 2), list(plan)
    assert want_rows is None or rows_or_bk == want_rows, list(plan)
    assert opt == (4 if family == 2 else 0), list(plan)


@pytest.mark.parametrize("case", STEM_CASES)
def test_stem_case_runs_the_long_tap_list_gather(case):
    """The 49-tap stem: the tap-gather kernel on the bias epilogue's long-tap-list form."""
    from avt_amd._lib import call

    b, T, H, W = case
    plan = (ctypes.c_int * 10)()
    call("avt_conv_fwd_plan", b * T, 1, H, W, 32, 64, 1, 7, 7, 2, 0, 3, 2, plan)
    assert (plan[0], plan[8], plan[9]) == (3, 1, 2), list(plan)


def test_residual_rows_at_clip_boundaries():
    """A residual that is nonzero only in the last frame of clip 0 and the first frame of clip 1 (halo form, the tile
    straddles the clip end): rows with a zero residual are bitwise the residual-free result, the others are that
    result plus the residual of their own row, added in fp32 and rounded once (epi_store_act)."""
    shape = (2, 4, 9, 11, 128, 128, 1)
    x, wp, bias, res, ref = _operands(shape)
    r = torch.zeros_like(res)
    r[0, 3] = res[0, 3]
    r[1, 0] = res[1, 0]
    with Halo3d(2):
        y0 = _run(shape, x, wp, bias, None, False)
        y1 = _run(shape, x, wp, bias, r, False)
    want = (y0.float() + r.float()).to(torch.bfloat16)
    assert torch.equal(y1.view(torch.int16), want.view(torch.int16))
    touched = (y1.view(torch.int16) != y0.view(torch.int16)).flatten(2).any(-1).cpu()  # [clip, frame]
    assert touched.tolist() == [[False, False, False, True], [True, False, False, False]]
    _check("residual at clip ends", y1, ref + r.cpu().double(), bias, res, "bias")


_STEM = {}


def _stem_operands(case):
    """The folded stem's operands: avt_video_stem_im2col's 32-channel input and the fold-1 pack of seeded bf16 values;
    the reference is the fp64 7x7x7 Conv3d on those values."""
    if case not in _STEM:
        from avt_amd._lib import call

        b, T, H, W = case
        g = torch.Generator().manual_seed(100 + H)
        video = torch.randn(b, 3, T, H, W, generator=g).to(torch.bfloat16)
        w = (torch.randn(64, 3, 7, 7, 7, generator=g) / (3 * 343) ** 0.5).to(torch.bfloat16)
        bias = torch.randn(64, generator=g)
        ref = F.conv3d(video.double(), w.double(), stride=(1, 2, 2), padding=3)
        Ho, Wo = ref.shape[-2:]
        ref = ref.permute(0, 2, 3, 4, 1).reshape(b * T, Ho, Wo, 64).contiguous()
        res = torch.randn(ref.shape, generator=g).to(torch.bfloat16)
        vd, wd = video.float().to(DEV), w.float().to(DEV)
        x = torch.empty(b, T, H, W, 32, device=DEV, dtype=torch.bfloat16)
        call("avt_video_stem_im2col", _p(vd), _p(x), b, 3, T, H, W, 7, 3, _stream())
        wp = torch.empty(64, 49 * 32, device=DEV, dtype=torch.bfloat16)
        call("avt_pack_conv3d_weight", _p(wd), _p(wp), 64, 3, 7, 7, 7, 1, _stream())
        torch.cuda.synchronize()
        _STEM[case] = (x, wp, bias.to(DEV), res.to(DEV), ref)
    return _STEM[case]


def _run_stem(case, x, wp, bias, res, relu, plain=False):
    from avt_amd._lib import call

    b, T, H, W = case
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    y = torch.full((b * T, Ho, Wo, 64), float("nan"), device=DEV, dtype=torch.bfloat16)
    if plain:
        call("avt_conv2d_fwd", _p(x), _p(wp), _p(y), None, b * T, H, W, 32, 64, 7, 7, 2, 3, 49 * 32, _stream())
    else:
        call("avt_conv3d_fwd_bias", _p(x), _p(wp), _p(y), b * T, 1, H, W, 32, 64, 1, 7, 7, 2, 0, 3, _p(bias), _p(res),
             int(relu), _stream())
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", STEM_CASES)
def test_stem_bias_epilogue_vs_fp64(case, mode):
    """The 49-tap stem (KT = 1, 7x7 / stride 2 over the b*T im2col frames) against the fp64 7x7x7 Conv3d."""
    x, wp, bias, res, ref = _stem_operands(case)
    y = _run_stem(case, x, wp, bias, res if mode == "bias_res_relu" else None, mode != "bias")
    _check(f"stem {case}", y, ref, bias, res, mode)


@pytest.mark.parametrize("case", STEM_CASES)
def test_stem_zero_bias_is_the_plain_forward(case):
    """bias = 0, no residual, no ReLU: bitwise the avt_conv2d_fwd the unfolded trunk runs for the stem."""
    x, wp, bias, _, _ = _stem_operands(case)
    y = _run_stem(case, x, wp, torch.zeros_like(bias), None, False)
    y0 = _run_stem(case, x, wp, None, None, False, plain=True)
    assert torch.equal(y.view(torch.int16), y0.view(torch.int16))


def test_refusals():
    """Every refusal of include/avt.h, by the library's error convention; the good call still runs."""
    from avt_amd._lib import call

    shape = (2, 4, 9, 11, 64, 128, 2)
    x, wp, bias, res, _ = _operands(shape)
    y = torch.empty(2, 4, 5, 6, 128, device=DEV, dtype=torch.bfloat16)

    def go(x=x, y=y, bias=bias, res=None, N=2, H=9, C=64, K=128, KT=3, k=3, stride=2):
        call("avt_conv3d_fwd_bias", _p(x), _p(wp), _p(y), N, 4, H, 11, C, K, KT, k, k, stride, 1, 1, _p(bias), _p(res),
             1, _stream())

    with pytest.raises(RuntimeError, match="bias is required"):
        go(bias=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        go(x=None)
    with pytest.raises(RuntimeError, match="alias"):
        go(res=y)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        go(K=96)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        go(C=48)
    with pytest.raises(RuntimeError, match="at most 49 taps"):
        go(k=5)  # 3 x 5 x 5 = 75 taps
    with pytest.raises(RuntimeError, match="stride"):
        go(stride=3)
    with pytest.raises(RuntimeError, match="2 GiB"):
        go(N=1 << 16, H=1 << 10)  # refused from the sizes alone: no buffer is touched
    try:
        call("avt_set_conv_variant", 0)
        with pytest.raises(RuntimeError, match="LDS-DMA"):
            go()
    finally:
        call("avt_set_conv_variant", 1)
    go()
    torch.cuda.synchronize()
