"""avt_fold_conv3d_bn_batched (the inference fold of the R3D trunk's frozen BatchNorm3d's into the Conv3d's in front of
them): the bf16 image and the fp32 bias against the same fp32 operation sequence done in torch on the device, bit for
bit, for a 3x3x3, a 1x1x1 and the stem record in one launch; with a scale of exactly 1 the image is bitwise the plain
packs'; the record size."""
import ctypes
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
EPS = 1e-5


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Rec:
    """One record: seeded fp32 OIDHW weights and BN tensors on the GPU, the outputs prefilled with NaN."""

    def __init__(self, K, C, kt, k, seed, stem=False, unit=False):
        g = torch.Generator().manual_seed(seed)
        self.K, self.C, self.kt, self.k, self.stem = K, C, kt, k, stem
        self.kg = k * k * 32 if stem else kt * k * k * C
        self.eps = 0.0 if unit else EPS
        self.w = torch.randn(K, C, kt, k, k, generator=g).to(DEV)
        gamma = 1 + 0.5 * torch.randn(K, generator=g)
        gamma[::5] = 0.0  # dead channels
        gamma[1::7] = -gamma[1::7].abs() - 0.1  # negative gamma
        var = torch.rand(K, generator=g) * 2 + 0.05
        var[::3] = 0.0  # eps alone
        if unit:
            gamma, var = torch.ones(K), torch.ones(K)
        self.gamma, self.var = gamma.to(DEV), var.to(DEV)
        self.beta = torch.randn(K, generator=g).to(DEV)
        self.mean = torch.randn(K, generator=g).to(DEV)
        self.out = torch.full((K, self.kg), float("nan"), device=DEV, dtype=torch.bfloat16)
        self.bias = torch.full((K,), float("nan"), device=DEV, dtype=torch.float32)

    def desc(self):
        ptrs = [t.data_ptr() for t in (self.w, self.out, self.gamma, self.beta, self.mean, self.var, self.bias)]
        return struct.pack("<QQQQQQQiiiiiifi", *ptrs, self.K, self.C, self.kt, self.k, self.k, int(self.stem),
                           self.eps, 0)

    def torch_fold(self):
        """The kernel's operation sequence in torch ops on the device, each rounded on its own: var + eps in fp32, its
        rsqrt as 1 / sqrt in fp64 rounded to fp32 once (tube.hip), the rest in fp32."""
        inv = (1.0 / torch.sqrt((self.var + self.eps).double())).float()
        s = self.gamma * inv
        bias = self.beta - self.mean * s
        ws = self.w * s.view(-1, 1, 1, 1, 1)  # [K][C][kt][r][s]
        if self.stem:  # [K][(r, s)][kt*4 + c], 32 channels per (r, s), zero padded
            img = torch.zeros(self.K, self.k, self.k, 8, 4, device=DEV)
            img[:, :, :, :self.kt, :self.C] = ws.permute(0, 3, 4, 2, 1)
        else:  # [K][(kt, r, s)][c]
            img = ws.permute(0, 2, 3, 4, 1)
        return img.reshape(self.K, self.kg).to(torch.bfloat16), bias


def _fold(recs):
    from avt_amd._lib import call, query

    blob = b"".join(r.desc() for r in recs)
    assert len(blob) == len(recs) * int(query("avt_fold3d_desc_bytes"))  # the table size
    table = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV)
    call("avt_fold_conv3d_bn_batched", _p(table), len(recs), max(r.K for r in recs),
         max(r.C * r.kt * r.k * r.k for r in recs), _stream())
    torch.cuda.synchronize()


def _records(unit=False):
    return [Rec(128, 64, 3, 3, 1, unit=unit), Rec(128, 64, 1, 1, 2, unit=unit), Rec(64, 3, 7, 7, 3, stem=True, unit=unit),
            Rec(512, 512, 3, 3, 4, unit=unit)]  # the last: the longest filter row of the trunk (13824 floats in LDS)


def test_fold3d_matches_the_torch_sequence_bitwise():
    """A 3x3x3, a 1x1x1, the stem and the largest record in one launch: image and bias bit for bit, nothing left
    unwritten, with gamma = 0 and negative gamma channels and running_var = 0 on every third channel."""
    recs = _records()
    _fold(recs)
    for r in recs:
        img, bias = r.torch_fold()
        assert not torch.isnan(r.out.float()).any() and not torch.isnan(r.bias).any()
        nb = (r.bias.view(torch.int32) != bias.view(torch.int32)).sum().item()
        ni = (r.out.view(torch.int16) != img.view(torch.int16)).sum().item()
        print(f"K={r.K} C={r.C} kt={r.kt} k={r.k} stem={r.stem}: {nb} bias and {ni} image elements differ")
        assert torch.equal(r.bias.view(torch.int32), bias.view(torch.int32))
        assert torch.equal(r.out.view(torch.int16), img.view(torch.int16))


def test_unit_scale_is_the_plain_pack():
    """s exactly 1 (gamma = 1, var = 1, eps = 0 in the record): bitwise avt_pack_conv3d_weights_batched's image, and
    avt_pack_conv3d_weight(fold = 1)'s for the stem; the bias is beta - mean."""
    from avt_amd._lib import call, query

    recs = _records(unit=True)
    _fold(recs)
    plain = [r for r in recs if not r.stem]
    outs = [torch.full_like(r.out, float("nan")) for r in plain]
    blob = b"".join(struct.pack("<QQiiii", r.w.data_ptr(), o.data_ptr(), r.K, r.C, r.kt * r.k * r.k, 0)
                    for r, o in zip(plain, outs))
    assert len(blob) == len(plain) * int(query("avt_pack3d_desc_bytes"))
    table = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV)
    call("avt_pack_conv3d_weights_batched", _p(table), len(plain), max(r.K for r in plain),
         max(r.C * r.kt * r.k * r.k for r in plain), _stream())
    stem = next(r for r in recs if r.stem)
    so = torch.full_like(stem.out, float("nan"))
    call("avt_pack_conv3d_weight", _p(stem.w), _p(so), stem.K, stem.C, stem.kt, stem.k, stem.k, 1, _stream())
    torch.cuda.synchronize()
    for r, o in list(zip(plain, outs)) + [(stem, so)]:
        assert torch.equal(r.out.view(torch.int16), o.view(torch.int16)), (r.K, r.C, r.kt)
        assert torch.equal(r.bias, r.beta - r.mean)
