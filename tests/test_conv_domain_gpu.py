"""The 2-D conv entry points over their accepted domain (include/avt.h), not only ResNet-18's: channel counts
off the powers of two (32 .. 2048), K = 192 / 320 / 384, non-square and even taps, every pad the header admits, the
Bottleneck trio -- exactconv.DOMAIN_2D / DOMAIN_DGRAD / DOMAIN_WGRAD, on exactly summable operands, compared for
EQUALITY with the fp64 reference under every distinct plan of test_conv_exact_gpu.py's knob sweeps (its test bodies
run here on these cases: outputs and the BN accumulator pre-filled with NaN, dw with 0.25; no tolerance other than the
accumulator's M2 column).  And one step outside each documented edge (exactconv.OUTSIDE): refused before any launch,
with a message that names the entry point, every output buffer still holding its pre-fill bit for bit.

EXPECTED_REFUSALS is empty: every in-domain case runs and compares."""
import ctypes

import pytest
import torch

import exactconv as ec
import test_conv_exact_gpu as tce
from avt_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
P, S = ec.P, ec.S
EXPECTED_REFUSALS = {}  # (entry point, case) -> message regex; needs the header narrowed and DESIGN 6r to say why

FWD = list(ec.DOMAIN_2D)
DGRAD = list(ec.DOMAIN_DGRAD)
WGRAD = list(ec.DOMAIN_WGRAD)
# 3x3 / stride 1 / pad 1 on the 128 x 128 halo tile: the forced split counts (divisors of the 64-channel chunk count)
SPLITK = {(3, 13, 13, 192, 128, 3, 3, 1, 1): (3, 8), (2, 7, 7, 320, 384, 3, 3, 1, 1): (5, 8),
          (1, 4, 4, 1024, 1024, 3, 3, 1, 1): (3, 8)}
SPLITK_DGRAD = {(3, 13, 13, 128, 192, 3, 3, 1, 1): (2, 3)}
_FAMILIES = {}


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    ec.KEEP.clear()


@pytest.mark.parametrize("case", FWD, ids=str)
def test_fwd_domain(case):
    """avt_conv2d_fwd with and without its BN accumulator under every distinct plan; avt_conv2d_fwd_bias (bias, bias +
    residual + ReLU) where the case has at most 9 taps -- more is the header's refusal (OUTSIDE has it)."""
    c = ec.get_case(case)
    tce.test_fwd_every_plan(case, record=False)
    _FAMILIES[case] = {p[0] for p, _ in tce._fwd_plans(case, ec.FWD_SWEEP, 0)}
    if c.R * c.S <= 9:
        tce.test_fwd_bias_every_plan(case)


def test_off_grid_families_are_reached():
    """Taken together the off-grid forwards launch the halo, tap-gather and register-staged families (the c64 and stem
    forms are ResNet-only by definition; the Bottleneck 64 -> 64 3x3 is the c64 shape)."""
    fams = set()
    for case in FWD:
        c = ec.get_case(case)
        fams |= {p[0] for p, _ in ec.fwd_plans(c, c.C, ec.FWD_SWEEP, 0)}
    assert fams >= {1, 3, 4}, fams
    if len(_FAMILIES) == len(FWD):
        assert set().union(*_FAMILIES.values()) >= {1, 3, 4}, _FAMILIES


@pytest.mark.parametrize("case,ks", [(c, k) for c, kss in SPLITK.items() for k in kss], ids=str)
def test_splitk_domain(case, ks):
    """avt_conv2d_fwd_ws / avt_conv2d_dgrad_ws on 3, 5 and 16 chunks of 64 channels: the forced split is the largest
    divisor of the chunk count <= ks, and the partials sum to the unsplit answer exactly."""
    c = ec.get_case(case)
    with ec.Knobs([("avt_set_halo_splitk", ks, 0)]):
        split = ec.fwd_plan(c, c.C, 3)[8]
    assert split == max(d for d in range(1, ks + 1) if (c.C // 64) % d == 0) and split > 1, (case, ks, split)
    tce.test_splitk_equals_unsplit(case, ks)


@pytest.mark.parametrize("case", DGRAD, ids=str)
def test_dgrad_domain(case):
    """avt_conv2d_dgrad plain, + add, in place, avt_conv2d_dgrad_mask, and the three BN epilogues of
    avt_conv2d_dgrad_bn, each under every distinct plan / setting of the dgrad sweep."""
    tce.test_dgrad_every_plan(case)
    for mode in ("relu_fma", "mask_y", "two_bn"):
        tce.test_dgrad_bn_epilogue(case, mode)


@pytest.mark.parametrize("case,ks", [(c, k) for c, kss in SPLITK_DGRAD.items() for k in kss], ids=str)
def test_dgrad_ws_domain(case, ks):
    """avt_conv2d_dgrad_ws (plain, add, masked add) with K = 192 = 3 chunks: splits 1 (ks 2) and 3."""
    c = ec.get_case(case)
    c.figures("dx")
    o = tce._ops(case)
    keep = ec.mask_from_bits(c.bits, c.x.shape)
    dxs = {"plain": ec.bf16_rne(c.ref("dx")), "add": ec.rne2(c.ref("dx"), c.add),
           "mask": ec.rne2(c.ref("dx"), torch.where(keep, c.add, torch.zeros_like(c.add)))}
    with ec.Knobs([("avt_set_halo_splitk", ks, 0)]):
        part, nf, cnt, nc = tce._splitk_ws(c, True)
        assert (nc > 0) == (ks >= 3), (case, ks, nc)
        for mode, want in dxs.items():
            dx = ec.nan_tensor(c.N, c.H, c.W, c.C)
            rc = lib().avt_conv2d_dgrad_ws(P(o["dy"]), P(o["wt"]), P(dx), P(o["add"]) if mode != "plain" else None,
                                           P(o["bits"]) if mode == "mask" else None, c.N, c.H, c.W, c.C, c.K, 3, 3, 1, 1,
                                           P(part), ctypes.c_longlong(nf), P(cnt), nc, S())
            assert rc == 0, lib().avt_last_error()
            torch.cuda.synchronize()
            ec.assert_rounded(dx, want, f"dgrad_ws {mode} {case} ks={ks} ({nc} tickets)")
        assert int(cnt.abs().max()) == 0
    print(f"dgrad_ws {case} ks={ks}: {nc} tickets")


@pytest.mark.parametrize("case", WGRAD, ids=str)
def test_wgrad_domain(case):
    """Every form test_wgrad_every_form runs (workspace, NULL workspace, atomics, gather table, tickets, deferred +
    avt_wgrad_reduce_batch) at C in 8 .. 192 and K in 64 / 192 / 320; the two SPLIT_WGRAD shapes split (asserted from
    the workspace size)."""
    c = ec.get_case(case)
    if case in ec.SPLIT_WGRAD:
        with ec.Knobs([ec.GATHER]):
            p = ec.wgrad_plan(c, c.Cw, 1)
            slab = p[15] + (p[16] << 31)
            Ng = c.R * c.S * c.Cw
            Ng = (Ng + 127) // 128 * 128 if Ng > 128 else (Ng + 63) // 64 * 64
            assert p[11] >= 2 and slab == p[11] * c.K * Ng * 4, (case, p)
    tce.test_wgrad_every_form(case, record=False)


# ---------------------------------------------------------------------------------------------------------------------
# one step outside
# ---------------------------------------------------------------------------------------------------------------------
def _filled(n, dtype, value):
    return torch.full((max(n, 1),), value, device=DEV, dtype=dtype)


OUT2D = [o for o in ec.OUTSIDE if "3d" not in o[0]]
# the name a refusal carries: the entry point's own, or -- for a check that sits in the implementation the entry points
# of a family share (avt_conv2d_dgrad / _mask / _bn / _ws; avt_conv2d_wgrad / _tk / _defer) -- the family's
NAMED = {"avt_conv2d_fwd": "conv2d_fwd", "avt_conv2d_fwd_bias": "conv2d_fwd_bias", "avt_conv2d_dgrad": "conv2d_dgrad",
         "avt_conv2d_dgrad_mask": "conv2d_dgrad_mask", "avt_conv2d_wgrad": "conv2d_wgrad"}


@pytest.mark.parametrize("entry,case,why", OUT2D, ids=lambda v: str(v).replace(" ", "_")[:40])
def test_outside_is_refused_untouched(entry, case, why):
    """Each call fails one AVT_REQUIRE of csrc/conv_gemm.hip that sits in front of the planner (read there: K % 64,
    C % 32 / % 64 / % 8, the tap bounds, the stride, pad < R, the aliasing rules): a non-zero code, a message naming the
    entry point, and the outputs (and the split-K-free workspace) exactly as pre-filled."""
    N, H, W, C, K, R, Sx, st, pad = case
    Pq, Qq = max(ec.conv_out(H, R, st, pad), 1), max(ec.conv_out(W, Sx, st, pad), 1)
    bf, f32 = torch.bfloat16, torch.float32
    x = _filled(N * H * W * C, bf, 1.0)
    dy = _filled(N * Pq * Qq * K, bf, 1.0)
    w = _filled(K * R * Sx * C, bf, 1.0)
    L = lib()
    if entry == "avt_conv2d_fwd":
        outs = [_filled(N * Pq * Qq * K, bf, 7.0), _filled(4096, torch.float64, 7.0)]
        rc = L.avt_conv2d_fwd(P(x), P(w), P(outs[0]), P(outs[1]), N, H, W, C, K, R, Sx, st, pad, R * Sx * C, S())
    elif entry == "avt_conv2d_fwd_bias":
        outs = [_filled(N * Pq * Qq * K, bf, 7.0)]
        res = outs[0] if "aliasing" in why else None
        rc = L.avt_conv2d_fwd_bias(P(x), P(w), P(outs[0]), N, H, W, C, K, R, Sx, st, pad, R * Sx * C,
                                   P(_filled(K, f32, 1.0)), P(res), 1, S())
    elif entry == "avt_conv2d_dgrad":
        outs = [_filled(N * H * W * C, bf, 7.0)]
        rc = L.avt_conv2d_dgrad(P(dy), P(w), P(outs[0]), None, N, H, W, C, K, R, Sx, st, pad, S())
    elif entry == "avt_conv2d_dgrad_mask":
        outs = [_filled(N * H * W * C, bf, 7.0)]
        rc = L.avt_conv2d_dgrad_mask(P(dy), P(w), P(outs[0]), P(outs[0]), P(_filled(N * H * W * C // 8, torch.uint8, 255)),
                                     N, H, W, C, K, R, Sx, st, pad, S())
    else:
        assert entry == "avt_conv2d_wgrad", entry
        outs = [_filled(K * R * Sx * C, f32, ec.PREFILL), _filled(1 << 16, f32, 7.0)]
        rc = L.avt_conv2d_wgrad(P(x), P(dy), P(outs[0]), N, H, W, C, C, K, R, Sx, st, pad, P(outs[1]),
                                ctypes.c_size_t(outs[1].numel() * 4), S())
    msg = L.avt_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and msg.startswith(NAMED[entry] + ":"), (entry, case, why, rc, msg)
    for o in outs:
        assert torch.equal(o, torch.full_like(o, ec.PREFILL if o.dtype == f32 and o is outs[0] else 7.0)), (entry, why)
    print(f"{entry} {case} ({why}): refused: {msg}")
