"""The trainable R3D-18 video trunk on the GPU: the Conv3d dgrad / wgrad kernels, the MaxPool3d backward and the stem's
folded weight gradient against fp64 torch on identical bf16 inputs, and a standalone ``generate_model(18, ...)`` after
``enable_backward()`` against ``tube_oracle.r3d18_forward`` under autograd (every parameter's gradient bounded by its
own yardstick: the same oracle under bf16 autocast, gradcheck.check_grads' rules).

Tolerances are the suite's own for the same kinds of output: 8e-3 for a bf16 conv result from bf16-rounded operands
(test_tube_gpu.py, test_kernels_gpu.py), 2e-4 for an fp32 weight gradient (test_kernels_gpu.py)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tube_oracle as tor
from avt_amd._lib import call, lib, query

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
_KEEP = []


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _KEEP.clear()


def P(t):
    if t is None:
        return None
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


# N, T, H, W, C, K, stride
CASES = [
    (2, 4, 9, 11, 64, 64, 1),
    (2, 4, 9, 11, 64, 128, 2),    # odd H and W
    (1, 5, 7, 6, 128, 256, 2),    # even W: the last input column sees one tap only
    (3, 1, 14, 14, 128, 256, 1),  # T = 1 on the halo form
    (1, 2, 3, 3, 512, 512, 1),
    (3, 5, 28, 28, 128, 128, 1),  # clip ends inside a tile
    (1, 16, 14, 14, 256, 512, 2),
    # the wgrad's frames of fewer than 32 positions (several frames per k-tile), as the stock trunk's layer4 has them
    (8, 5, 4, 4, 256, 512, 1),    # 640 positions = 20 k-tiles, >= 2 splits; odd T: a clip end inside a k-tile
    (8, 4, 7, 7, 256, 512, 2),    # stride 2 into 4 x 4 frames, 16 k-tiles, >= 2 splits
    (4, 3, 4, 4, 512, 512, 1),    # several k-tiles, one split
    (20, 4, 2, 1, 64, 128, 1),    # Q = 1: a k-tile steps 32 rows and no columns; P*Q = 2
    (5, 3, 1, 1, 64, 64, 1),      # one position per frame
    (2, 3, 4, 8, 64, 64, 1),      # P*Q = 32: the first size off that branch
    (2, 3, 3, 11, 64, 64, 1),     # P*Q = 33
    (2, 3, 1, 31, 64, 64, 1),     # P*Q = 31: the last size on it
    # stride-2 dgrad parity classes
    (2, 3, 8, 7, 64, 128, 2),     # even H, odd W
    (3, 2, 1, 5, 64, 128, 2),     # H = 1: the ph = 1 classes are empty
    (3, 2, 5, 1, 64, 128, 2),     # W = 1: the pw = 1 classes are empty
    # stride-1 dgrad on every patch form of the forward's launch path, either side of each switch in width
    (1, 2, 5, 39, 128, 128, 1),   # the last width on the 336-row patch (C % 128 == 0)
    (1, 2, 5, 40, 128, 128, 1),   # the first on the two-weight-stage form
    (1, 2, 5, 79, 128, 128, 1),   # its last
    (1, 2, 5, 80, 128, 128, 1),   # the tap gather
    (1, 2, 56, 56, 128, 128, 1),  # layer2's width, 416-row patch
    (1, 2, 5, 115, 64, 64, 1),    # the last width on the 488-row patch (C = 64)
    (1, 2, 5, 116, 64, 64, 1),    # the tap gather
    (1, 2, 20, 112, 64, 64, 1),   # layer1's width, 488-row patch
]
SPLIT_CASES = CASES[7:9]  # must reach the wgrad's split-K (asserted from the workspace size)


def _pack_dgrad(w):
    K, C = w.shape[:2]
    wt = torch.empty(C, 27 * K, device=DEV, dtype=torch.bfloat16)
    call("avt_pack_conv3d_weight_dgrad", P(w), P(wt), K, C, 3, 3, 3, S())
    return wt


@pytest.mark.parametrize("K,C", [(128, 64), (64, 64)])
def test_dgrad_pack_layout(K, C):
    """out[c][(KT-1-kt, R-1-r, S-1-s, k)] = bf16(w[k][c][kt][r][s]), bitwise; the batched form gives the same bits."""
    w = torch.randn(K, C, 3, 3, 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    wt = _pack_dgrad(w)
    ref = w.flip(2, 3, 4).permute(1, 2, 3, 4, 0).reshape(C, 27 * K).to(torch.bfloat16)
    torch.cuda.synchronize()
    assert torch.equal(wt, ref)
    import struct

    wt2 = torch.zeros_like(wt)
    desc = struct.pack("<QQiiii", w.data_ptr(), wt2.data_ptr(), K, C, 27, 0)
    assert len(desc) == int(query("avt_pack3d_desc_bytes"))
    table = torch.frombuffer(bytearray(desc), dtype=torch.uint8).to(DEV)
    call("avt_pack_conv3d_weights_dgrad_batched", P(table), 1, C * (K // 64), S())
    torch.cuda.synchronize()
    assert torch.equal(wt2, ref)


_REF = {}


def _case_data(case):
    """bf16 operands of a case and its fp64 references (computed once, shared by the dgrad and wgrad tests)."""
    if case not in _REF:
        N, T, H, W, C, K, st = case
        g = torch.Generator().manual_seed(17)
        Ho, Wo = conv_out(H, 3, st, 1), conv_out(W, 3, st, 1)
        x = torch.randn(N, T, H, W, C, generator=g).relu().to(torch.bfloat16)
        dy = torch.randn(N, T, Ho, Wo, K, generator=g).to(torch.bfloat16)
        add = torch.randn(N, T, H, W, C, generator=g).to(torch.bfloat16)
        w = (torch.randn(K, C, 3, 3, 3, generator=g) * (2.0 / (K * 27)) ** 0.5).float()
        xn, dyn = x.double().permute(0, 4, 1, 2, 3), dy.double().permute(0, 4, 1, 2, 3)
        dx = torch.nn.grad.conv3d_input(xn.shape, w.to(torch.bfloat16).double(), dyn, stride=(1, st, st), padding=1)
        dw = torch.nn.grad.conv3d_weight(xn, (K, C, 3, 3, 3), dyn, stride=(1, st, st), padding=1)
        _REF[case] = dict(x=x, dy=dy, add=add, w=w, dx=dx.permute(0, 2, 3, 4, 1).contiguous(), dw=dw)
    return _REF[case]


def _dgrad(dy, wt, dx, add, case):
    N, T, H, W, C, K, st = case
    call("avt_conv3d_dgrad", P(dy), P(wt), P(dx), P(add), N, T, H, W, C, K, 3, 3, 3, st, 1, 1, S())


@pytest.mark.parametrize("case", CASES)
def test_conv3d_dgrad(case):
    """avt_conv3d_dgrad vs torch.nn.grad.conv3d_input in fp64 on the same bf16 operands: plain, + add, add aliasing dx.
    A stride-1 case runs the forward's launch path: on its default form for the shape (avt_set_halo3d(-1)) and on the
    tap gather (0)."""
    N, T, H, W, C, K, st = case
    d = _case_data(case)
    wt = _pack_dgrad(d["w"].to(DEV))
    dy, add = d["dy"].to(DEV), d["add"].to(DEV)
    ref_add = d["dx"] + d["add"].double()
    try:
        for halo3d in ((-1, 0) if st == 1 else (-1,)):
            call("avt_set_halo3d", halo3d)
            dx = torch.full((N, T, H, W, C), float("nan"), device=DEV, dtype=torch.bfloat16)
            _dgrad(dy, wt, dx, None, case)
            e0 = rel_err(dx, d["dx"])
            dx1 = torch.full_like(dx, float("nan"))
            _dgrad(dy, wt, dx1, add, case)
            e1 = rel_err(dx1, ref_add)
            dx2 = add.clone()
            _dgrad(dy, wt, dx2, dx2, case)
            torch.cuda.synchronize()
            print(f"{case} halo3d={halo3d}: dgrad rel err {e0:.3e}, +add {e1:.3e}")
            assert e0 < 8e-3, (halo3d, e0)
            assert e1 < 8e-3, (halo3d, e1)
            assert torch.equal(dx2, dx1), halo3d  # in place: the same bits as out of place
    finally:
        call("avt_set_halo3d", -1)


def _wgrad(x, dy, dw, case, ws="auto"):
    N, T, H, W, C, K, st = case
    wsb = int(query("avt_conv3d_wgrad_workspace", N, T, H, W, C, K, 3, 3, 3, st, 1, 1))
    assert wsb > 0
    if ws == "auto":
        ws = torch.full((wsb // 4,), float("nan"), device=DEV)  # any contents
    return lib().avt_conv3d_wgrad(P(x), P(dy), P(dw), N, T, H, W, C, K, 3, 3, 3, st, 1, 1, P(ws),
                                  0 if ws is None else ws.numel() * 4, S())


@pytest.mark.parametrize("case", CASES)
def test_conv3d_wgrad(case):
    """avt_conv3d_wgrad vs fp64 conv3d_weight; dw pre-filled with 0.25 (+=), two runs bitwise equal, and no atomic path:
    a NULL workspace is an error."""
    N, T, H, W, C, K, st = case
    d = _case_data(case)
    if case in SPLIT_CASES:  # slab bytes = splits * K * Ng * 4, Ng = 27 C rounded up to 128
        wsb = int(query("avt_conv3d_wgrad_workspace", N, T, H, W, C, K, 3, 3, 3, st, 1, 1))
        Ng = (27 * C + 127) // 128 * 128
        assert wsb % (K * Ng * 4) == 0 and wsb // (K * Ng * 4) >= 2, (wsb, K, Ng)
    x, dy = d["x"].to(DEV), d["dy"].to(DEV)
    dw = torch.full((K, C, 3, 3, 3), 0.25, device=DEV)
    dw2 = dw.clone()
    assert _wgrad(x, dy, dw, case) == 0, lib().avt_last_error()
    assert _wgrad(x, dy, dw2, case) == 0
    dw3 = dw.clone()
    assert _wgrad(x, dy, dw3, case, ws=None) != 0  # refused, not computed with atomics
    torch.cuda.synchronize()
    err = rel_err(dw - 0.25, d["dw"])
    print(f"{case}: wgrad rel err {err:.3e}")
    assert err < 2e-4, err
    assert torch.equal(dw, dw2)
    assert torch.equal(dw3, dw)  # untouched by the refused call


@pytest.mark.parametrize("N,T", [(2, 2), (3, 1)])
@pytest.mark.parametrize("st", [1, 2])
def test_clip_isolation_exact(N, T, st):
    """x non-zero only in clip 1's first frame, dy only in clip 0's last frame: the two never meet, so dw stays
    exactly at its pre-fill and the dgrad of that dy is exactly zero over all of clip 1."""
    H, W, C, K = 6, 7, 64, 128
    case = (N, T, H, W, C, K, st)
    Ho, Wo = conv_out(H, 3, st, 1), conv_out(W, 3, st, 1)
    g = torch.Generator().manual_seed(23)
    x = torch.zeros(N, T, H, W, C)
    x[1, 0] = torch.randn(H, W, C, generator=g) + 3.0
    dy = torch.zeros(N, T, Ho, Wo, K)
    dy[0, T - 1] = torch.randn(Ho, Wo, K, generator=g) + 3.0
    x, dy = x.to(torch.bfloat16).to(DEV), dy.to(torch.bfloat16).to(DEV)
    dw = torch.full((K, C, 3, 3, 3), 0.25, device=DEV)
    assert _wgrad(x, dy, dw, case) == 0, lib().avt_last_error()
    w = torch.randn(K, C, 3, 3, 3, generator=g).to(DEV)
    dx = torch.full((N, T, H, W, C), float("nan"), device=DEV, dtype=torch.bfloat16)
    _dgrad(dy, _pack_dgrad(w), dx, None, case)
    torch.cuda.synchronize()
    assert torch.equal(dw, torch.full_like(dw, 0.25))
    assert torch.equal(dx[1:].float(), torch.zeros_like(dx[1:].float()))
    assert dx[0, T - 1].float().abs().max() > 0  # (the gradient did reach clip 0)


@pytest.mark.parametrize("shape", [(1, 5, 7, 9, 8), (3, 1, 1, 2, 16), (2, 4, 6, 6, 64)])
def test_maxpool3d_bwd(shape):
    """avt_maxpool3d_bwd vs torch's CPU max_pool3d backward on ReLU'd inputs with many tied zeros and an all-zero window
    (ties go to the first maximum in scan order): bitwise where at most one window contributes, one bf16 ulp elsewhere."""
    N, T, H, W, C = shape
    g = torch.Generator().manual_seed(31)
    x = (torch.randn(N, T, H, W, C, generator=g) - 0.6).relu()
    x[0, :3, :3, :3] = 0  # window (0, 0, 0) of clip 0 is all zero
    x = x.to(torch.bfloat16)
    To, Ho, Wo = (T - 1) // 2 + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = torch.randn(N, To, Ho, Wo, C, generator=g).to(torch.bfloat16)
    xr = x.float().permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    yr = F.max_pool3d(xr, 3, 2, 1)
    assert (yr[0, :, 0, 0, 0] == 0).all()
    yr.backward(gy.float().permute(0, 4, 1, 2, 3).contiguous())
    ref = xr.grad.permute(0, 2, 3, 4, 1).contiguous()
    # contributing windows per voxel: the same backward of a gradient of ones (gy has no zeros)
    xc = x.float().permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    F.max_pool3d(xc, 3, 2, 1).backward(torch.ones_like(yr))
    cnt = xc.grad.permute(0, 2, 3, 4, 1).contiguous()
    xd, gyd = x.to(DEV), gy.to(DEV)
    y = torch.empty(N, To, Ho, Wo, C, device=DEV, dtype=torch.bfloat16)
    call("avt_maxpool3d_fwd", P(xd), P(y), N, T, H, W, C, S())
    gx = torch.full((N, T, H, W, C), float("nan"), device=DEV, dtype=torch.bfloat16)
    call("avt_maxpool3d_bwd", P(gyd), P(xd), P(y), P(gx), N, T, H, W, C, S())
    torch.cuda.synchronize()
    gx = gx.cpu()
    refb = ref.to(torch.bfloat16)
    one = cnt <= 1
    assert torch.equal(gx[one].view(torch.int16), refb[one].view(torch.int16))
    if (~one).any():
        a, b = gx[~one].float(), ref[~one]
        ulp = torch.maximum(b.abs(), torch.tensor(2.0 ** -126)).log2().floor().exp2() * 2.0 ** -7
        assert ((a - b).abs() <= ulp).all()


@pytest.mark.parametrize("vshape", [(2, 3, 4, 32, 32), (1, 3, 3, 17, 9)])
def test_stem_wgrad(vshape):
    """The 7x7x7 stem's weight gradient -- a 2-D wgrad over the folded 32-channel input, unfolded into OIDHW -- vs the
    fp64 conv3d weight gradient on the same bf16 operands; two runs bitwise equal."""
    b, C, T, H, W = vshape
    g = torch.Generator().manual_seed(41)
    video = torch.randn(b, C, T, H, W, generator=g).to(torch.bfloat16).float()  # bf16-exact values
    Ho, Wo = conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3)
    dy = torch.randn(b, T, Ho, Wo, 64, generator=g).to(torch.bfloat16)
    ref = torch.nn.grad.conv3d_weight(video.double(), (64, 3, 7, 7, 7), dy.double().permute(0, 4, 1, 2, 3),
                                      stride=(1, 2, 2), padding=3)
    vd, dyd = video.to(DEV), dy.to(DEV)
    x = torch.empty(b, T, H, W, 32, device=DEV, dtype=torch.bfloat16)
    call("avt_video_stem_im2col", P(vd), P(x), b, C, T, H, W, 7, 3, S())
    outs = []
    for _ in range(2):
        dwf = torch.zeros(64, 7, 7, 32, device=DEV)
        wsb = int(query("avt_conv2d_wgrad_workspace", b * T, H, W, 32, 32, 64, 7, 7, 2, 3))
        ws = torch.empty(max(wsb, 16), device=DEV, dtype=torch.uint8)
        call("avt_conv2d_wgrad", P(x), P(dyd), P(dwf), b * T, H, W, 32, 32, 64, 7, 7, 2, 3, P(ws), wsb, S())
        dw = torch.full((64, 3, 7, 7, 7), 0.25, device=DEV)
        call("avt_stem3d_wgrad_unfold", P(dwf), P(dw), 64, 3, 7, 7, 7, S())
        outs.append(dw)
    torch.cuda.synchronize()
    err = rel_err(outs[0] - 0.25, ref)
    print(f"{vshape}: stem wgrad rel err {err:.3e}")
    assert err < 2e-4, err
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
LABELS = torch.tensor([7, 911])


def _standalone(max_pool, enable=True):
    from avt_amd.resnet3D import generate_model

    sd = tor.make_tube_state(0)
    net = generate_model(18, no_max_pool=not max_pool, n_classes=1039)
    net.load_state_dict({k[len("vidnet."):]: v for k, v in sd.items() if k.startswith("vidnet.")})
    if enable:
        net.enable_backward()
    return net.to(DEV).train(), sd


def _oracle_grads(sd, video, max_pool, autocast):
    """(logits, {name: gradient}) of CE(fc(avgpool(r3d18_forward(video))), LABELS) on the CPU."""
    names = [k for k, v in sd.items() if k.startswith("vidnet.") and v.is_floating_point()
             and not k.endswith(("running_mean", "running_var"))]
    dt = torch.float32 if autocast else torch.float64
    s = {k: (v.detach().to(dt).clone() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for n in names:
        s[n].requires_grad_(True)
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        feat = tor.r3d18_forward(s, "vidnet.", video.to(dt), training=True, max_pool=max_pool)
        logits = F.linear(feat.mean(dim=(2, 3, 4)), s["vidnet.fc.weight"], s["vidnet.fc.bias"])
    loss = F.cross_entropy(logits.float() if autocast else logits, LABELS)
    loss.backward()
    return logits.detach(), {n[len("vidnet."):]: s[n].grad.double() for n in names}, s


class _Conv3dCheckedWgrad(torch.autograd.Function):
    """F.conv3d as torch.autocast("cpu", bfloat16) runs it -- bf16 operands, bf16 result, bf16 gradients -- with the
    weight gradient computed by the fp32 kernel on the same bf16 tensors and rounded to bf16: what a correct bf16
    weight-gradient kernel returns (fp32 sums of bf16 products, one rounding).  For hosts whose CPU bf16 conv3d
    weight-gradient kernel returns non-finite values."""

    @staticmethod
    def forward(ctx, x, w, stride, padding):
        xb, wb = x.to(torch.bfloat16), w.to(torch.bfloat16)
        ctx.save_for_backward(xb, wb)
        ctx.conv, ctx.wdtype = (stride, padding), w.dtype
        with torch.autocast("cpu", enabled=False):
            return _TORCH_CONV3D(xb, wb, stride=stride, padding=padding)

    @staticmethod
    def backward(ctx, gy):
        xb, wb = ctx.saved_tensors
        stride, padding = ctx.conv
        gy = gy.to(torch.bfloat16)
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.nn.grad.conv3d_input(xb.shape, wb, gy, stride=stride, padding=padding)
        gw = torch.nn.grad.conv3d_weight(xb.float(), wb.shape, gy.float(), stride=stride, padding=padding)
        return gx, gw.to(torch.bfloat16).to(ctx.wdtype), None, None


_TORCH_CONV3D = F.conv3d


def _oracle_grads_checked_wgrad(sd, video, max_pool):
    """The bf16-autocast oracle run with every conv's weight gradient from _Conv3dCheckedWgrad."""
    from unittest import mock

    def conv3d(x, w, bias=None, stride=1, padding=0):
        assert bias is None
        return _Conv3dCheckedWgrad.apply(x, w, stride, padding)

    with mock.patch.object(tor.F, "conv3d", conv3d):
        return _oracle_grads(sd, video, max_pool, autocast=True)


@pytest.mark.parametrize("max_pool", [False, True])
def test_r3d_backward_end_to_end(max_pool):
    """Every parameter gradient of a standalone trainable R3D-18 (CE of the fc logits, make_video(2, 4, 64)) vs the
    fp64 oracle, bounded by its own yardstick -- the same oracle under bf16 autocast, computed here -- by
    gradcheck.check_grads' rules: error vector <= max(5e-2, 3 e_ref), cosine >= min(0.999, 1 - 3 (1 - cos_ref)), norm
    deviation <= max(5e-2, 3 d_ref, e_ref).  Parameters whose yardstick error exceeds 0.3 (their bound says nothing)
    are printed; the logits and running statistics stay within test_r3d_forward_standalone's 3e-2.

    Measured yardstick: on this 2-clip batch the bf16-autocast oracle's own error vector is 0.20-0.45 for EVERY
    parameter (e.g. conv1.weight 0.35, layer1.0.conv1.weight 0.35, layer2.0.conv1.weight 0.35, layer3.0.conv1.weight
    0.32, layer4.0.conv1.weight 0.27, layer4.1.conv2.weight 0.20; with the max-pool 0.23-0.45), and 96 x 96 frames do
    not lower it (0.30-0.44): the noise enters at the two-row cross-entropy / batch-statistics end, not through the
    frame size, so the e_ref > 0.3 list is most of the trunk, not only layer4's BN biases.  The rule is kept as stated;
    the kernels' own accuracy is pinned by the per-kernel fp64 tests above.  This build's gradients measured 0.36-0.38
    on conv1.weight / layer2.0.conv1.weight (cosine 0.93), inside 3 x the yardstick.  One host's CPU bf16 conv3d
    returned non-finite weight gradients for a few convs (a different few per run; the stem's conv1.weight every
    time): those parameters' yardstick is recomputed by the same autocast oracle with the conv weight gradients
    summed in fp32 from the same bf16 tensors (_Conv3dCheckedWgrad); where both are finite that run's yardstick
    errors equal the plain autocast run's to 1e-6."""
    video = tor.make_video(2, 4, 64)
    net, sd = _standalone(max_pool)
    logits = net(video.to(DEV))
    loss = F.cross_entropy(logits, LABELS.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    ref_logits, g64, s64 = _oracle_grads(sd, video, max_pool, autocast=False)
    # the yardstick.  Some hosts' CPU bf16 conv3d weight-gradient kernel returns non-finite values (a few convs, a
    # different few per run, the 3-channel stem every time): such a parameter's yardstick comes from a second run of
    # the same autocast oracle whose conv weight gradients are summed by the fp32 kernel from the same bf16 tensors
    _, gbf, _ = _oracle_grads(sd, video, max_pool, autocast=True)
    broken = [n for n, gr in gbf.items() if not bool(torch.isfinite(gr).all())]
    if broken:
        print(f"max_pool={max_pool}: non-finite autocast gradients from the CPU kernels, recomputed: {broken}")
        checked = _oracle_grads_checked_wgrad(sd, video, max_pool)[1]
        for n in broken:
            gbf[n] = checked[n]
    err = rel_err(logits.detach(), ref_logits)
    print(f"max_pool={max_pool}: logits rel err {err:.3e}")
    assert err < 3e-2, err
    rm = rel_err(net.bn1.running_mean, s64["vidnet.bn1.running_mean"])
    rv = rel_err(net.layer4[1].bn2.running_var, s64["vidnet.layer4.1.bn2.running_var"])
    assert rm < 3e-2 and rv < 3e-2, (rm, rv)
    bad, vague = [], []
    named = dict(net.named_parameters())
    for n, ref in g64.items():
        assert named[n].grad is not None, n
        v = named[n].grad.detach().double().cpu().flatten().numpy()
        r, yb = ref.flatten().numpy(), gbf[n].flatten().numpy()
        nr = max(np.linalg.norm(r), 1e-300)
        e, e_ref = np.linalg.norm(v - r) / nr, np.linalg.norm(yb - r) / nr
        cos = float(v @ r / max(np.linalg.norm(v) * nr, 1e-300))
        cos_ref = float(yb @ r / max(np.linalg.norm(yb) * nr, 1e-300))
        d, d_ref = abs(np.linalg.norm(v) / nr - 1), abs(np.linalg.norm(yb) / nr - 1)
        if e_ref > 0.3:
            vague.append((n, round(float(e_ref), 3)))
        if e > max(5e-2, 3 * e_ref):
            bad.append((n, "error", round(float(e), 4), round(float(e_ref), 4)))
        if cos < min(0.999, 1 - 3 * (1 - cos_ref)):
            bad.append((n, "cosine", round(cos, 5), round(cos_ref, 5)))
        if d > max(5e-2, 3 * d_ref, e_ref):
            bad.append((n, "norm", round(float(d), 4), round(float(d_ref), 4)))
    print(f"max_pool={max_pool}: {len(g64)} gradients checked; yardstick error > 0.3 (bound vacuous): {vague}")
    for b in bad:
        print("OUT OF BOUND", b)
    assert not bad, bad


def test_r3d_backward_behaviour():
    """Opt-in and reproducibility: a default module still raises in grad mode, enable_backward() raises on
    FullModel.vidnet, a video that requires grad raises, an eval-mode trunk raises, two forward+backward passes from the
    same state give bitwise-equal gradients, a second backward through one forward raises, and five SGD steps on one
    batch lower the loss."""
    from avt_amd.model import FullModel

    video = tor.make_video(2, 4, 64).to(DEV)
    labels = LABELS.to(DEV)
    net0, _ = _standalone(False, enable=False)
    with pytest.raises(NotImplementedError, match="enable_backward"):
        net0(video)
    with pytest.raises(RuntimeError):
        FullModel().vidnet.enable_backward()
    net, _ = _standalone(False)
    with pytest.raises(NotImplementedError):
        net(video.clone().requires_grad_(True))
    net.eval()
    with pytest.raises(NotImplementedError):
        net(video)
    net.train()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    grads = []
    for _ in range(2):
        net.load_state_dict(state)
        net.zero_grad(set_to_none=True)
        out = net(video)
        loss = F.cross_entropy(out, labels)
        loss.backward()
        grads.append({n: p.grad.clone() for n, p in net.named_parameters()})
    with pytest.raises(RuntimeError):
        loss.backward()
    torch.cuda.synchronize()
    assert all(g is not None for g in grads[0].values())
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n
    net.load_state_dict(state)
    opt = torch.optim.SGD(net.parameters(), lr=1e-2)
    losses = []
    for _ in range(6):
        opt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(net(video), labels)
        losses.append(loss.item())
        loss.backward()
        opt.step()
    print("SGD losses:", [round(v, 4) for v in losses])
    assert losses[5] < losses[0], losses
