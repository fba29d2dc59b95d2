"""The tap-gather ("TN") wgrad's per-pixel gather table (avt_wgrad_pixtab_*, conv_tn_pipe.h TAB): the table's
contents against a numpy restatement, and the wgrad reading it against the wgrad recomputing its offsets in the loop
(avt_set_wgrad_pixtab(0)) -- bitwise, through avt_conv2d_wgrad -- and against torch's fp64 weight gradient."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from avt_amd._lib import call, query  # noqa: E402

DEV = "cuda"


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _rand_act(N, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, H, W, C, generator=g).to(torch.bfloat16)


def build_table(N, H, W, C, R, st, pad):
    nb = int(query("avt_wgrad_pixtab_bytes", N, H, W, R, R, st, pad))
    assert nb > 0
    tab = torch.full((nb // 4,), -1, device=DEV, dtype=torch.int32)
    call("avt_wgrad_pixtab_build", P(tab), N, H, W, C, R, R, st, pad, S())
    return tab


def table_ref(N, H, W, C, R, st, pad):
    """[npad, 2] uint32: (byte offset of input pixel (n, oh*st - pad, ow*st - pad) modulo 2^32, tap mask)."""
    Pq, Qq = conv_out(H, R, st, pad), conv_out(W, R, st, pad)
    npix = N * Pq * Qq
    npad = (npix + 31) // 32 * 32
    out = np.zeros((npad, 2), dtype=np.uint32)  # the padded tail: always invalid (0, 0)
    pix = np.arange(npix, dtype=np.int64)
    n, rem = pix // (Pq * Qq), pix % (Pq * Qq)
    y0, x0 = (rem // Qq) * st - pad, (rem % Qq) * st - pad
    out[:npix, 0] = ((((n * H + y0) * W + x0) * C * 2) % (1 << 32)).astype(np.uint32)
    mask = np.zeros(npix, dtype=np.int64)
    for r in range(R):
        for s in range(R):
            ok = (y0 + r >= 0) & (y0 + r < H) & (x0 + s >= 0) & (x0 + s < W)
            mask |= ok.astype(np.int64) << (r * R + s)
    out[:npix, 1] = mask.astype(np.uint32)
    return out


# N, H, W, C, K, R, stride, pad -- the smallest shapes at which the table form can still go wrong
EDGE = (2, 5, 7, 128, 128, 3, 1, 1)      # borders on every side; P*Q = 35: the k-tiles straddle the image boundary
TINY = (2, 9, 11, 64, 128, 3, 2, 1)      # P*Q = 30 < 32: two images in one k-tile; R*S*C = 576 is no multiple of BN
ONE_TAP = (2, 9, 11, 64, 128, 1, 2, 0)   # one tap bit; an odd input size dropped by the stride (a 128 x 64 tile)
RAGGED = (3, 3, 3, 128, 256, 3, 1, 1)    # 27 pixels: one ragged k-tile, padded entries only past the batch
ISSUE_CASES = [EDGE, TINY, ONE_TAP, RAGGED]
# the same geometries with enough k-tiles per block for the steps past the ring's prologue (which keeps the in-loop
# arithmetic for its NST - 1 tiles): these are the launches whose gathers read the table
LONG = [(16,) + c[1:] for c in ISSUE_CASES]
# the other tiles of the planner: 256 x 256 and 256 x 128 (K 512; 128-wide with avt_set_wgrad_tiles(0)), 64 x 128 and
# 64 x 64 (K 64)
WIDE = [(16, 5, 6, 256, 512, 3, 1, 1), (16, 5, 6, 128, 512, 3, 1, 1), (16, 9, 11, 64, 64, 3, 1, 1),
        (16, 9, 11, 64, 64, 1, 2, 0)]


@pytest.mark.parametrize("case", ISSUE_CASES + [WIDE[0]], ids=str)
def test_pixtab_contents(case):
    """Entry for entry, padded tail included, against the numpy restatement."""
    N, H, W, C, K, R, st, pad = case
    tab = build_table(N, H, W, C, R, st, pad)
    torch.cuda.synchronize()
    got = tab.cpu().numpy().view(np.uint32).reshape(-1, 2)
    ref = table_ref(N, H, W, C, R, st, pad)
    assert got.shape == ref.shape
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], got[bad[:8]], ref[bad[:8]])


def test_pixtab_geometry_without_table():
    """More than 32 taps (the 7x7 stems) have no table form: size 0, and build / register refuse."""
    assert int(query("avt_wgrad_pixtab_bytes", 2, 16, 16, 7, 7, 2, 3)) == 0
    t = torch.zeros(64, device=DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        call("avt_wgrad_pixtab_build", P(t), 2, 16, 16, 32, 7, 7, 2, 3, S())
    with pytest.raises(RuntimeError):
        call("avt_wgrad_pixtab_register", P(t), 2, 16, 16, 32, 7, 7, 2, 3)


_REF = {}


def _operands(case):
    """(x, dy on the device, the fp64 weight gradient): computed once per case and left unchanged."""
    if case not in _REF:
        N, H, W, C, K, R, st, pad = case
        Pq, Qq = conv_out(H, R, st, pad), conv_out(W, R, st, pad)
        x = _rand_act(N, H, W, C, 8).relu()
        dy = _rand_act(N, Pq, Qq, K, 9)
        ref = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (K, C, R, R), dy.double().permute(0, 3, 1, 2),
                                          stride=st, padding=pad)
        _REF[case] = (x.to(DEV), dy.to(DEV), ref)
    return _REF[case]


def _wgrad(case, xd, dyd, slab=True, tickets=False):
    N, H, W, C, K, R, st, pad = case
    dw = torch.full((K, R, R, C), 0.25, device=DEV)  # accumulates into an existing gradient
    wsb = int(query("avt_conv2d_wgrad_workspace", N, H, W, C, C, K, R, R, st, pad)) if slab else 0
    ws = torch.empty(max(wsb, 1), device=DEV, dtype=torch.uint8)
    if tickets:
        nt = int(query("avt_conv2d_wgrad_tickets", N, H, W, C, C, K, R, R, st, pad))
        assert nt > 0, "the fused reduce should apply to this plan"
        tk = torch.zeros(nt, device=DEV, dtype=torch.int32)
        call("avt_conv2d_wgrad_tk", P(xd), P(dyd), P(dw), N, H, W, C, C, K, R, R, st, pad, P(ws), wsb, P(tk), nt, S())
    else:
        call("avt_conv2d_wgrad", P(xd), P(dyd), P(dw), N, H, W, C, C, K, R, R, st, pad, P(ws) if slab else None, wsb,
             S())
    torch.cuda.synchronize()
    return dw


def _check(case, policy=(0, 4), tiles=1, fused=False, poison=False):
    """Table form twice (run-to-run bits), the in-loop arithmetic once (the same bits), fp64 (test_conv_wgrad's bound).
    poison: an all-invalid table registered instead must change the result -- the launch does read the table."""
    N, H, W, C, K, R, st, pad = case
    xd, dyd, ref = _operands(case)
    geo = (N, H, W, C, R, R, st, pad)
    tab = build_table(N, H, W, C, R, st, pad)
    try:
        call("avt_set_wgrad_halo", 0)  # every case on the tap-gather kernel
        call("avt_set_wgrad_tiles", tiles)
        call("avt_set_wgrad_policy", *policy)
        if fused:
            call("avt_set_wgrad_fused", 1, -1)
        call("avt_set_wgrad_pixtab", 1)
        call("avt_wgrad_pixtab_register", P(tab), *geo)
        a = _wgrad(case, xd, dyd, tickets=fused)
        b = _wgrad(case, xd, dyd, tickets=fused)
        if poison:
            zero = torch.zeros_like(tab)
            call("avt_wgrad_pixtab_register", P(zero), *geo)
            z = _wgrad(case, xd, dyd, tickets=fused)
            call("avt_wgrad_pixtab_register", P(tab), *geo)
        call("avt_set_wgrad_pixtab", 0)
        c = _wgrad(case, xd, dyd, tickets=fused)
        call("avt_set_wgrad_pixtab", 1)
        call("avt_wgrad_pixtab_register", None, *geo)  # no table: the arithmetic again
        d = _wgrad(case, xd, dyd, tickets=fused)
    finally:
        call("avt_wgrad_pixtab_register", None, *geo)
        call("avt_set_wgrad_pixtab", -1)
        call("avt_set_wgrad_fused", -1, -1)
        call("avt_set_wgrad_policy", 0, 4)
        call("avt_set_wgrad_tiles", 1)
        call("avt_set_wgrad_halo", -1)
    err = rel_err(a.permute(0, 3, 1, 2) - 0.25, ref)
    print(f"{case} policy={policy} tiles={tiles} fused={fused}: rel err vs fp64 {err:.3e}, "
          f"|table - arithmetic| {(a - c).abs().max().item():.3e}")
    assert err < 2e-4
    assert torch.equal(a, b), "table form: run-to-run bits"
    assert torch.equal(a, c), "table form vs in-loop arithmetic (knob 0)"
    assert torch.equal(c, d), "knob 0 vs no registered table"
    if poison:
        assert not torch.equal(z, a), "the launch did not read its table"


@pytest.mark.parametrize("case", ISSUE_CASES, ids=str)
def test_wgrad_pixtab_bitwise_small(case):
    """The edge geometries at their smallest, under the default plan and with one k-tile per block and k group (more
    blocks asked for than there are k-tiles: the planner keeps every split non-empty, so at KG = 2 an odd tile count
    leaves one group of the last block a dummy tile)."""
    _check(case)
    _check(case, policy=(1 << 20, 1))


@pytest.mark.parametrize("case", LONG + WIDE, ids=str)
def test_wgrad_pixtab_bitwise_long(case):
    """Block ranges longer than the ring, so that the steps gather from the table: one block per tile (the deepest
    range), the default plan, and an odd number of k-tiles per block (at KG = 2: one group a tile short)."""
    nkt = (case[0] * conv_out(case[1], case[5], case[6], case[7]) * conv_out(case[2], case[5], case[6], case[7]) + 31) // 32
    _check(case, policy=(1, 1), poison=True)
    _check(case)
    _check(case, policy=(0, 5 if nkt > 10 else 3))


@pytest.mark.parametrize("case", [WIDE[0], WIDE[1]], ids=str)
def test_wgrad_pixtab_bitwise_128_tiles_of_k512(case):
    """avt_set_wgrad_tiles(0): the K 512 convs on the 4-wave 128 x 128 tile (KG = 1 and 2)."""
    _check(case, tiles=0, policy=(1, 1), poison=True)
    _check(case, tiles=0)


@pytest.mark.parametrize("case", [LONG[0], WIDE[0]], ids=str)
def test_wgrad_pixtab_bitwise_fused(case):
    """The FUSED instantiations (avt_set_wgrad_fused(1): the in-kernel slab reduce): a quarter of the k-tiles per
    split (the 128 x 128 tile pairs them at KG = 2: two splits of two groups; the 256 x 256 tile runs four)."""
    N, H, W, C, K, R, st, pad = case
    nkt = (N * conv_out(H, R, st, pad) * conv_out(W, R, st, pad) + 31) // 32
    _check(case, policy=(0, (nkt + 3) // 4), fused=True, poison=True)
