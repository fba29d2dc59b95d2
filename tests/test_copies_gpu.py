"""Two copies on the product path with no test of their own: avt_nhwc_bf16_to_nchw (what hands activations and
gradients back across the Python boundary) and avt_pack_conv_weights_part (the engine's split weight pack)."""
import ctypes
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

from avt_amd._lib import call, query  # noqa: E402

DEV = "cuda"
_KEEP = []  # device temporaries passed to the C-ABI stay alive until the test ends


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _KEEP.clear()


def P(t):
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("N,C,HW", [(2, 64, 63), (3, 512, 1), (1, 8, 197)])
def test_nhwc_bf16_to_nchw(N, C, HW):
    """Exactly x.float().permute(...); and back through avt_nchw_to_nhwc_bf16 with Cp = C it is the identity
    (the values are bf16-representable)."""
    g = torch.Generator().manual_seed(61 + C)
    x = torch.randn(N, HW, C, generator=g).to(torch.bfloat16)
    xd = x.to(DEV)
    y = torch.full((N, C, HW), float("nan"), device=DEV)
    call("avt_nhwc_bf16_to_nchw", P(xd), P(y), N, C, HW, S())
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), x.float().permute(0, 2, 1).contiguous())
    back = torch.full((N, HW, C), float("nan"), device=DEV, dtype=torch.bfloat16)
    call("avt_nchw_to_nhwc_bf16", P(y), P(back), N, C, HW, 1, C, S())
    torch.cuda.synchronize()
    assert torch.equal(_bits(back), _bits(xd))


# K, R, C, Cp, Kg, flat offset (floats): a padded 7x7 stem (no dgrad image), a 3x3, a 1x1 downsample, partial
# 64x64 tiles, a misaligned source
PACK_CASES = [(64, 7, 3, 4, 224, 0), (128, 3, 64, 64, 576, 9408), (256, 1, 128, 128, 128, 83136),
              (96, 3, 40, 40, 360, 115905), (64, 7, 1, 1, 64, 150465)]
SENTINEL = 0x5A5A  # bits of every destination element before a pack


def _pack_table(flat):
    """(device table, [(fwd, dgrad or None)], max elements) with every destination filled with the sentinel."""
    descs, outs, maxel = [], [], 0
    for K, R, C, Cp, Kg, o in PACK_CASES:
        w = flat[o:o + K * R * R * C]
        wf = torch.full((K, Kg), SENTINEL, device=DEV, dtype=torch.int16).view(torch.bfloat16)
        wt = torch.full((C, R * R * K), SENTINEL, device=DEV, dtype=torch.int16).view(torch.bfloat16) \
            if C == Cp else None
        descs.append(struct.pack("<QQQiiiiii", w.data_ptr(), wf.data_ptr(), 0 if wt is None else wt.data_ptr(),
                                 K, R * R, C, Cp, Kg, 0))
        maxel = max(maxel, K * Kg + (0 if wt is None else wt.numel()))
        outs.append((wf, wt))
        _KEEP.extend([wf, wt])
    table = torch.frombuffer(bytearray(b"".join(descs)), dtype=torch.uint8).to(DEV)
    return table, outs, maxel


def _untouched(t):
    return t is None or bool((_bits(t) == SENTINEL).all())


def test_pack_conv_weights_part():
    """which = 1 writes exactly the fwd images of avt_pack_conv_weights_batched and leaves every dgrad destination
    untouched; which = 2 the reverse.  Both images are also compared with the pack restated in torch, and a part
    started further down the table (as the engine starts each trunk's) leaves the convs before it alone."""
    total = max(o + K * R * R * C for K, R, C, _, _, o in PACK_CASES)
    flat = torch.randn(total, generator=torch.Generator().manual_seed(67)).to(DEV)
    _KEEP.append(flat)
    desc_bytes = int(query("avt_pack_desc_bytes"))
    assert desc_bytes == 48

    table_b, both, maxel = _pack_table(flat)
    call("avt_pack_conv_weights_batched", P(table_b), len(PACK_CASES), maxel, S())
    table_1, fwd_only, _ = _pack_table(flat)
    call("avt_pack_conv_weights_part", P(table_1), len(PACK_CASES), maxel, 1, S())
    table_2, dg_only, _ = _pack_table(flat)
    call("avt_pack_conv_weights_part", P(table_2), len(PACK_CASES), maxel, 2, S())
    table_s, sub, _ = _pack_table(flat)
    for which in (1, 2):  # convs 1 .. n-1 only
        call("avt_pack_conv_weights_part", P(table_s[desc_bytes:]), len(PACK_CASES) - 1, maxel, which, S())
    torch.cuda.synchronize()

    for i, (K, R, C, Cp, Kg, o) in enumerate(PACK_CASES):
        w = flat[o:o + K * R * R * C].cpu().reshape(K, R * R, C)
        ref_f = torch.zeros(K, Kg)
        ref_f[:, :R * R * Cp] = torch.nn.functional.pad(w, (0, Cp - C)).reshape(K, R * R * Cp)
        ref_f = ref_f.to(torch.bfloat16)
        ref_t = w.permute(2, 1, 0).reshape(C, R * R * K).to(torch.bfloat16)
        bf, bt = both[i]
        assert torch.equal(_bits(bf.cpu()), _bits(ref_f)), i
        assert bt is None or torch.equal(_bits(bt.cpu()), _bits(ref_t)), i
        assert torch.equal(_bits(fwd_only[i][0]), _bits(bf)) and _untouched(fwd_only[i][1]), i
        assert _untouched(dg_only[i][0]), i
        assert bt is None or torch.equal(_bits(dg_only[i][1]), _bits(bt)), i
        if i == 0:
            assert _untouched(sub[i][0]) and _untouched(sub[i][1])
        else:
            assert torch.equal(_bits(sub[i][0]), _bits(bf)), i
            assert bt is None or torch.equal(_bits(sub[i][1]), _bits(bt)), i
