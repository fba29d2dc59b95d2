"""avt_conv2d_fwd_bias -- out = [relu](conv(x, w) + bias[k] (+ residual)) -- in every kernel form the forward planner
picks for a ResNet-18 shape, against fp64 on the identical bf16 operands.  Each form is forced with the library's
knobs (restored afterwards) at the smallest shapes that cross its edges; the bound is the project's own for conv
outputs, 8e-3 of the output's largest magnitude."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL = 8e-3


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# form -> (knobs set before the call, [(N, H, W, C, K, k, stride)])
FORMS = {
    "c64": ({}, [(1, 9, 9, 64, 64, 3, 1), (2, 17, 15, 64, 64, 3, 1)]),
    "halo4": ({"avt_set_halo8": 0, "avt_set_small_tiles": 0}, [(1, 7, 5, 128, 128, 3, 1), (2, 14, 19, 128, 128, 3, 1)]),
    "halo8": ({"avt_set_halo8": 1, "avt_set_small_tiles": 0}, [(1, 20, 20, 128, 128, 3, 1), (1, 13, 79, 256, 256, 3, 1)]),
    "halo8x64": ({"avt_set_halo": 2, "avt_set_c64": 0, "avt_set_small_tiles": 0}, [(1, 9, 9, 64, 64, 3, 1)]),
    "halo64": ({"avt_set_small_tiles": -1}, [(1, 7, 5, 128, 128, 3, 1), (2, 9, 17, 256, 256, 3, 1)]),
    "gather_s2": ({"avt_set_small_tiles": 0}, [(2, 9, 9, 64, 128, 3, 2), (2, 9, 9, 64, 128, 1, 2)]),
    "gather_s1": ({"avt_set_halo": 0, "avt_set_small_tiles": 0}, [(1, 7, 7, 256, 256, 3, 1), (1, 4, 4, 512, 512, 3, 1)]),
    "gather_small": ({"avt_set_halo": 0, "avt_set_small_tiles": -1},
                     [(2, 9, 9, 64, 128, 3, 2), (2, 9, 9, 64, 128, 1, 2), (1, 9, 9, 64, 64, 3, 1)]),
    "gather_128x64": ({"avt_set_c64": 0, "avt_set_small_tiles": 0}, [(2, 17, 15, 64, 64, 3, 1)]),
    # the 8-wave 256 x 128 tap-gather tile is the planner's choice from 65536 GEMM rows: the smallest such 1x1/s2 conv
    "gather_256x128": ({"avt_set_small_tiles": 0}, [(1, 511, 511, 64, 128, 1, 2)]),
}
RESTORE = {"avt_set_halo8": -1, "avt_set_small_tiles": -2, "avt_set_halo": 1, "avt_set_c64": 1,
           "avt_set_nt128_config": -1}
CASES = [(f, s) for f, (_, shapes) in FORMS.items() for s in shapes]
# what a form's name claims of avt_conv_fwd_plan's answer (include/avt_tuning.h): the family (0 c64, 1 halo, 3 tap
# gather) and, where the name says one, the tile's rows x columns
NAMED = {"c64": (0, None), "halo4": (1, (128, 128)), "halo8": (1, (256, 128)), "halo8x64": (1, (256, 64)),
         "halo64": (1, (64, 128)), "gather_s2": (3, None), "gather_s1": (3, None), "gather_small": (3, (64, None)),
         "gather_128x64": (3, (128, 64)), "gather_256x128": (3, (256, 128))}


class Knobs:
    def __init__(self, knobs):
        self.knobs = knobs

    def __enter__(self):
        from avt_amd._lib import call

        for k, v in self.knobs.items():
            call(k, v)

    def __exit__(self, *exc):
        from avt_amd._lib import call

        for k in self.knobs:
            call(k, RESTORE[k])


_OPS = {}


def _operands(shape):
    """Seeded bf16 operands of a shape and the fp64 conv of exactly those values (once per shape)."""
    if shape not in _OPS:
        N, H, W, C, K, k, stride = shape
        g = torch.Generator().manual_seed(hash(shape) % 10000)
        pad = k // 2
        x = torch.randn(N, H, W, C, generator=g).to(torch.bfloat16)
        w = (torch.randn(K, k, k, C, generator=g) / (k * k * C) ** 0.5).to(torch.bfloat16)
        bias = torch.randn(K, generator=g)
        ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), stride=stride, padding=pad)
        ref = ref.permute(0, 2, 3, 1).contiguous()
        res = torch.randn(ref.shape, generator=g).to(torch.bfloat16)
        _OPS[shape] = (x.to(DEV), w.reshape(K, -1).contiguous().to(DEV), bias.to(DEV), res.to(DEV), ref)
    return _OPS[shape]


def _run(shape, x, w, bias, res, relu, entry="avt_conv2d_fwd_bias"):
    from avt_amd._lib import call

    N, H, W, C, K, k, stride = shape
    P, Q = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    y = torch.full((N, P, Q, K), float("nan"), device=DEV, dtype=torch.bfloat16)
    if entry == "avt_conv2d_fwd":
        call(entry, _p(x), _p(w), _p(y), None, N, H, W, C, K, k, k, stride, k // 2, k * k * C, _stream())
    else:
        call(entry, _p(x), _p(w), _p(y), N, H, W, C, K, k, k, stride, k // 2, k * k * C, _p(bias), _p(res), int(relu),
             _stream())
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("mode", ["bias", "bias_relu", "bias_res_relu"])
@pytest.mark.parametrize("form,shape", CASES)
def test_bias_epilogue_vs_fp64(form, shape, mode):
    """Each form, three modes: within 8e-3 of the fp64 result's largest magnitude everywhere, no NaN left."""
    x, w, bias, res, ref = _operands(shape)
    want = ref + bias.cpu().double()
    if mode == "bias_res_relu":
        want = want + res.cpu().double()
    if mode != "bias":
        want = want.clamp_min(0)
    with Knobs(FORMS[form][0]):
        y = _run(shape, x, w, bias, res if mode == "bias_res_relu" else None, mode != "bias")
    got = y.cpu().double()
    assert torch.isfinite(got).all()
    err = (got - want).abs().max().item()
    scale = want.abs().max().item()
    print(f"{form} {shape} {mode}: max err {err:.3e} = {err / scale:.2e} of max |out| {scale:.3f}")
    assert err <= TOL * scale


@pytest.mark.parametrize("form,shape", CASES)
def test_zero_bias_is_the_plain_forward(form, shape):
    """(a) bias = 0, no residual, no ReLU: bitwise avt_conv2d_fwd on the same operands -- one main loop, one tile store."""
    x, w, bias, _, _ = _operands(shape)
    with Knobs(FORMS[form][0]):
        y = _run(shape, x, w, torch.zeros_like(bias), None, False)
        y0 = _run(shape, x, w, None, None, False, entry="avt_conv2d_fwd")
    assert torch.equal(y.view(torch.int16), y0.view(torch.int16))


@pytest.mark.parametrize("form,shape", CASES)
def test_case_runs_the_form_it_names(form, shape):
    """The planner's own account of the call (avt_conv_fwd_plan under the case's knobs): the family and tile the form's
    name claims, on the bias epilogue's narrow argument form, without split-K."""
    from avt_amd._lib import call

    N, H, W, C, K, k, stride = shape
    plan = (ctypes.c_int * 10)()
    with Knobs(FORMS[form][0]):
        call("avt_conv_fwd_plan", N, 1, H, W, C, K, 1, k, k, stride, 0, k // 2, 1, plan)
    family, wm, wn, tm, tn, _, _, _, ksplit, epi = plan
    want_family, want_tile = NAMED[form]
    tile = (wm * tm * 32, wn * tn * 32)
    assert (family, ksplit, epi) == (want_family, 1, 1), list(plan)
    assert want_tile is None or all(w is None or w == t for w, t in zip(want_tile, tile)), list(plan)


def test_tile_override_does_not_reach_the_bias_epilogue():
    """avt_set_nt128_config(3) moves the plain forward of this shape to the 256 x 128 k32 tile; the bias epilogue stays
    on the planner's default (128 x 128 k64): with a zero bias it is, bit for bit, the plain forward at config -1."""
    from avt_amd._lib import call

    shape = (1, 7, 7, 256, 256, 3, 1)
    x, w, bias, _, _ = _operands(shape)
    base = {"avt_set_halo": 0, "avt_set_small_tiles": 0}
    with Knobs(dict(base, avt_set_nt128_config=3)):
        plan = (ctypes.c_int * 10)()
        call("avt_conv_fwd_plan", 1, 1, 7, 7, 256, 256, 1, 3, 3, 1, 0, 1, 0, plan)
        assert list(plan)[:7] == [3, 2, 2, 4, 2, 3, 32]  # the override is live for the plain forward
        y = _run(shape, x, w, torch.zeros_like(bias), None, False)
    with Knobs(base):
        y0 = _run(shape, x, w, None, None, False, entry="avt_conv2d_fwd")
    assert torch.isfinite(y.float()).all()
    assert torch.equal(y.view(torch.int16), y0.view(torch.int16))


@pytest.mark.parametrize("form,shape", CASES)
def test_relu_clamps_exactly(form, shape):
    """(b) a large negative bias on every third channel: exactly 0.0 wherever the fp64 pre-activation is below minus
    the tolerance, and nothing negative anywhere."""
    x, w, bias, res, ref = _operands(shape)
    b = bias.clone()
    b[::3] = -50.0
    pre = ref + b.cpu().double() + res.cpu().double()
    with Knobs(FORMS[form][0]):
        y = _run(shape, x, w, b, res, True)
    got = y.cpu().double()
    tol = TOL * pre.clamp_min(0).abs().max().item()
    assert (got >= 0).all()
    assert (got[pre < -tol] == 0.0).all()
    assert (pre[..., ::3] < -tol).all()  # the case is exercised: those channels are all clamped
    assert (got - pre.clamp_min(0)).abs().max().item() <= TOL * max(pre.clamp_min(0).max().item(), 1.0)


def test_refusals():
    """(c) NULL bias, and the channel counts / geometries the plain forward refuses, by the library's error convention."""
    shape = (1, 9, 9, 64, 64, 3, 1)
    x, w, bias, res, _ = _operands(shape)
    from avt_amd._lib import call

    y = torch.empty(1, 9, 9, 64, device=DEV, dtype=torch.bfloat16)

    def go(x=x, w=w, y=y, bias=bias, res=None, N=1, H=9, W=9, C=64, K=64, k=3, stride=1, Kg=576):
        call("avt_conv2d_fwd_bias", _p(x), _p(w), _p(y), N, H, W, C, K, k, k, stride, 1, Kg, _p(bias), _p(res), 1,
             _stream())

    with pytest.raises(RuntimeError, match="bias is required"):
        go(bias=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        go(x=None)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        go(K=96)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        go(C=4, Kg=64)
    with pytest.raises(RuntimeError, match="Kg"):
        go(Kg=608)
    with pytest.raises(RuntimeError, match="stride"):
        go(stride=3)
    with pytest.raises(RuntimeError, match="9 taps"):
        go(k=5, Kg=1600)
    with pytest.raises(RuntimeError, match="alias"):
        go(res=y)
    go()  # and the good call still runs
    torch.cuda.synchronize()
