"""avt_fold_conv_bn_batched (the inference fold of a frozen BatchNorm into the conv in front of it) against fp64
numpy: the packed bf16 image of w * s, s = gamma / sqrt(running_var + eps), the bias beta - running_mean * s, the
zero padding, the stem record's (scale, shift), and one record alone against a whole batch of records."""
import ctypes
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
EPS = 1e-5


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _bf16_bits_to_f64(t):
    return (t.view(torch.int16).cpu().numpy().astype(np.int32).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _bf16_ulp(x):
    """The spacing of bf16 (8 significand bits) at |x| (fp64 array); the smallest normal's for tiny values."""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126)))
    return 2.0 ** (e - 7)


class Conv:
    """One record: seeded weights and BN tensors on the GPU, the output buffers prefilled with NaN."""

    def __init__(self, K, k, C, seed, Cp=None, var_zero=False, plain=False):
        g = torch.Generator().manual_seed(seed)
        self.K, self.RS, self.C, self.Cp, self.plain = K, k * k, C, Cp or C, plain
        self.Kg = (self.RS * self.Cp + 31) // 32 * 32
        self.w = torch.randn(K, k, k, C, generator=g).to(DEV)
        gamma = 1 + 0.5 * torch.randn(K, generator=g)
        gamma[::5] = 0.0  # dead channels
        gamma[1::7] = -gamma[1::7].abs() - 0.1  # negative gamma
        self.gamma = gamma.to(DEV)
        self.beta = torch.randn(K, generator=g).to(DEV)
        self.mean = torch.randn(K, generator=g).to(DEV)
        var = torch.rand(K, generator=g) * 2 + 0.05
        if var_zero:
            var[::3] = 0.0  # eps alone
        self.var = var.to(DEV)
        self.fwd = torch.full((K, self.Kg), float("nan"), device=DEV, dtype=torch.bfloat16)
        self.bias = torch.full((2, K) if plain else (K,), float("nan"), device=DEV, dtype=torch.float32)

    def desc(self):
        ptrs = [t.data_ptr() for t in (self.w, self.fwd, self.gamma, self.beta, self.mean, self.var, self.bias)]
        return struct.pack("<QQQQQQQiiiiiifi", *ptrs, self.K, self.RS, self.C, self.Cp, self.Kg, int(self.plain), EPS, 0)

    def check(self):
        w = self.w.cpu().double().numpy().reshape(self.K, self.RS, self.C)
        gamma, beta, mean, var = (t.cpu().double().numpy() for t in (self.gamma, self.beta, self.mean, self.var))
        s = gamma / np.sqrt(var + np.float64(np.float32(EPS)))
        b = beta - mean * s
        got = _bf16_bits_to_f64(self.fwd).reshape(self.K, self.Kg)
        body = got[:, :self.RS * self.Cp].reshape(self.K, self.RS, self.Cp)
        ref = w * (1.0 if self.plain else s[:, None, None])
        err = np.abs(body[:, :, :self.C] - ref)
        assert np.isfinite(got).all()
        assert (err <= _bf16_ulp(ref)).all(), float((err / _bf16_ulp(ref)).max())
        assert (body[:, :, self.C:] == 0).all() and (got[:, self.RS * self.Cp:] == 0).all()  # padding exactly zero
        bias = self.bias.cpu().double().numpy()
        tol = 1e-6 * (np.abs(beta) + np.abs(mean * s))
        if self.plain:
            assert (np.abs(bias[0] - s) <= 1e-6 * np.abs(s)).all()
            assert (np.abs(bias[1] - b) <= tol).all()
        else:
            assert (np.abs(bias - b) <= tol).all(), float((np.abs(bias - b) / np.maximum(tol, 1e-300)).max())


def _fold(convs):
    from avt_amd._lib import call, query

    blob = b"".join(c.desc() for c in convs)
    assert len(blob) == len(convs) * int(query("avt_fold_desc_bytes"))
    table = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV)
    call("avt_fold_conv_bn_batched", _ptr(table), len(convs), max(c.K * c.Kg for c in convs),
         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


def _trunk_records(seed=100):
    """The shapes of one ResNet-18 trunk's records: the stem, then 3x3 and 1x1 convs at K = 64 .. 512."""
    recs = [Conv(64, 7, 3, seed, Cp=4, plain=True)]
    cin = 64
    for i, K in enumerate((64, 128, 256, 512)):
        recs.append(Conv(K, 3, cin, seed + 10 * i + 1, var_zero=(i % 2 == 0)))
        recs.append(Conv(K, 3, K, seed + 10 * i + 2))
        if cin != K:
            recs.append(Conv(K, 1, cin, seed + 10 * i + 3, var_zero=True))
        cin = K
    return recs


@pytest.mark.parametrize("K,k,C", [(64, 3, 64), (128, 3, 64), (128, 1, 64), (256, 3, 128), (256, 1, 128),
                                   (512, 3, 256), (512, 1, 256), (512, 3, 512)])
@pytest.mark.parametrize("var_zero", [False, True])
def test_fold_one_conv(K, k, C, var_zero):
    """One record: every packed weight within one bf16 ulp of w * s (fp64), bias within 1e-6 (|beta| + |mean s|),
    with gamma = 0 and negative gamma channels, and running_var = 0 (eps alone) on every third channel."""
    c = Conv(K, k, C, seed=K + k + C, var_zero=var_zero)
    _fold([c])
    c.check()


def test_fold_trunk_batched_equals_single():
    """A whole trunk's records in one launch: each is right, and bitwise what its own single-record launch gives."""
    batch = _trunk_records()
    _fold(batch)
    for c in batch:
        c.check()
    for c, one in zip(batch, _trunk_records()):
        _fold([one])
        assert torch.equal(c.fwd.view(torch.int16), one.fwd.view(torch.int16))
        assert torch.equal(c.bias.view(torch.int32), one.bias.view(torch.int32))


def test_fold_padded_channels():
    """The general (scalar) path: C = 3 padded to Cp = 4, Kg rounded up to 32 -- scaled, padding columns exactly zero."""
    c = Conv(64, 7, 3, seed=5, Cp=4)
    _fold([c])
    c.check()


def test_fold_stem_scale_shift_matches_bn_finalize():
    """The stem record leaves the unscaled pack and bn1's (scale, shift), equal to what trunk._bn_finalize's eval
    branch computes from the same tensors to 2 fp32 ulps."""
    from avt_amd.trunk import BNSpec, _bn_finalize

    c = Conv(64, 7, 1, seed=9, Cp=1, plain=True, var_zero=True)
    _fold([c])
    c.check()

    class S:
        def param(self, n):
            return c.gamma if n.endswith(".weight") else c.beta

        def buffer(self, n):
            return c.mean if n.endswith("running_mean") else c.var

    st = _bn_finalize(c.fwd, None, 0, BNSpec("bn1", 64), S(), False, eps=EPS)
    torch.cuda.synchronize()
    for i in range(2):
        ref, got = st[i].cpu().double().numpy(), c.bias[i].cpu().double().numpy()
        ulp = np.spacing(np.abs(st[i].cpu().numpy()).astype(np.float32)).astype(np.float64)
        assert (np.abs(got - ref) <= 2 * ulp).all(), (i, float((np.abs(got - ref) / ulp).max()))
