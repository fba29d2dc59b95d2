"""The Conv3d entry points over their accepted domain (include/avt.h), not only 3x3x3 / pad 1: (KT, R, S) in
(3,3,3), (1,3,3), (3,1,1), (1,1,1) at stride 2, (2,2,2), (5,3,3) = 45 taps and a non-square (1,3,1); pad_t in 0 / 1 / 2;
C in 32 / 96 / 192 with K in 64 / 128 / 192 (dgrad: C in 64 / 128 / 192, K in 32 / 96 / 192), the three-patch halo form
on 3 chunks of 64 channels included -- exactconv.DOMAIN_3D / DOMAIN_3D_DGRAD on
exactly summable operands, compared for EQUALITY with the fp64 reference under every distinct plan of
test_conv3d_exact_gpu.py's sweep (its test bodies run here on these cases).  And one step outside each documented edge
(exactconv.OUTSIDE): refused before any launch, the outputs untouched.

EXPECTED_REFUSALS is empty: every in-domain case runs and compares."""
import ctypes

import pytest
import torch

import exactconv as ec
import test_conv3d_exact_gpu as t3
from avt_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
P, S = ec.P, ec.S
EXPECTED_REFUSALS = {}
FWD = list(ec.DOMAIN_3D)
DGRAD = list(ec.DOMAIN_3D_DGRAD)
WGRAD = [c for c in FWD if ec.wgrad3d_ok(c)]
_FAMILIES = {}


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    ec.KEEP.clear()


@pytest.mark.parametrize("case", FWD, ids=str)
def test_conv3d_fwd_domain(case):
    """avt_conv3d_fwd with its BN accumulator and avt_conv3d_fwd_bias (bias; bias + residual + ReLU) under every
    distinct plan of the sweep."""
    t3.test_conv3d_fwd_every_plan(case, record=False)
    c = ec.get_case(case)
    _FAMILIES[case] = {p[0] for p, _ in ec.fwd_plans(c, c.C, ec.SWEEP_3D, 0)}


def test_conv3d_off_grid_families():
    """Both Conv3d families run off the grid: the three-patch halo form (family 2) on 3 chunks of 64 channels -- C = 192
    with its 256 x 64 (K = 64) and 256 x 128 (K = 128) tiles, forward and as the forward form of a stride-1 dgrad with
    K = 192 -- and the tap gather's Conv3d form (family 3) on everything else, which the three-patch form's geometry
    (3x3x3 / stride 1 / pad 1, C % 64 == 0: halo3d_eligible) leaves to it."""
    by_case = {}
    for case in FWD:
        c = ec.get_case(case)
        by_case[case] = {p[0] for p, _ in ec.fwd_plans(c, c.C, ec.SWEEP_3D, 0)}
        same = (c.KT, c.R, c.S, c.st, c.pad_t, c.pad) == (3, 3, 3, 1, 1, 1) and c.C % 64 == 0
        assert by_case[case] == ({2, 3} if same and c.K in (64, 128) else {3}), (case, by_case[case])
    patch = [c for c, f in by_case.items() if 2 in f]
    assert {(c[4], c[5]) for c in patch} >= {(192, 64), (192, 128)}, patch
    dg = {case: {p[0] for p, _ in ec.fwd_plans(ec.get_case(case), case[4], ec.SWEEP_3D, 0, dgrad=True)}
          for case in DGRAD if case[9] == 1}
    assert {(c[4], c[5]) for c, f in dg.items() if 2 in f} >= {(64, 192), (128, 192)}, dg
    if len(_FAMILIES) == len(FWD):  # the whole file ran: what was launched
        assert set().union(*_FAMILIES.values()) >= {2, 3}, _FAMILIES


@pytest.mark.parametrize("case", DGRAD, ids=str)
def test_conv3d_dgrad_domain(case):
    """avt_conv3d_dgrad plain, + add, in place: stride 1 on every distinct plan of the forward form, stride 2 on the
    parity classes (with unequal tap counts per axis where R != S)."""
    t3.test_conv3d_dgrad_exact(case)


@pytest.mark.parametrize("case", WGRAD, ids=str)
def test_conv3d_wgrad_domain(case):
    """avt_conv3d_wgrad at temporal 'same' padding (its documented domain): K = 192 takes the 64-row tile, 27 x 96 and
    45 x 32 columns are no multiple of 128."""
    t3.test_conv3d_wgrad_exact(case)


def _filled(n, dtype, value):
    return torch.full((max(n, 1),), value, device=DEV, dtype=dtype)


OUT3D = [o for o in ec.OUTSIDE if "3d" in o[0]]


@pytest.mark.parametrize("entry,case,why", OUT3D, ids=lambda v: str(v).replace(" ", "_")[:40])
def test_outside_is_refused_untouched(entry, case, why):
    """Each call fails one AVT_REQUIRE in front of the planner (conv_gemm.hip conv3d_fwd_impl / avt_conv3d_fwd_bias /
    avt_conv3d_dgrad, conv3d_bwd.hip wgrad3d_args_ok): a non-zero code, a message naming the entry point, outputs and
    workspace exactly as pre-filled."""
    N, T, H, W, C, K, KT, R, Sx, st, pad_t, pad = case
    To = max(T + 2 * pad_t - KT + 1, 1)
    Pq, Qq = max(ec.conv_out(H, R, st, pad), 1), max(ec.conv_out(W, Sx, st, pad), 1)
    bf, f32 = torch.bfloat16, torch.float32
    taps = KT * R * Sx
    x = _filled(N * T * H * W * C, bf, 1.0)
    dy = _filled(N * To * Pq * Qq * K, bf, 1.0)
    w = _filled(K * taps * C, bf, 1.0)
    g = (N, T, H, W, C, K, KT, R, Sx, st, pad_t, pad)
    L = lib()
    if entry == "avt_conv3d_fwd":
        outs = [_filled(dy.numel(), bf, 7.0), _filled(4096, torch.float64, 7.0)]
        rc = L.avt_conv3d_fwd(P(x), P(w), P(outs[0]), P(outs[1]), *g, S())
    elif entry == "avt_conv3d_fwd_bias":
        outs = [_filled(dy.numel(), bf, 7.0)]
        rc = L.avt_conv3d_fwd_bias(P(x), P(w), P(outs[0]), *g, P(_filled(K, f32, 1.0)), P(outs[0]), 1, S())
    elif entry == "avt_conv3d_dgrad":
        outs = [_filled(x.numel(), bf, 7.0)]
        rc = L.avt_conv3d_dgrad(P(dy), P(w), P(outs[0]), None, *g, S())
    else:
        assert entry == "avt_conv3d_wgrad", entry
        outs = [_filled(K * taps * C, f32, 7.0), _filled(1 << 20, f32, 7.0)]
        rc = L.avt_conv3d_wgrad(P(x), P(dy), P(outs[0]), *g, P(outs[1]), ctypes.c_size_t(outs[1].numel() * 4), S())
    msg = L.avt_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and msg.startswith(entry[4:] + ":"), (entry, case, why, rc, msg)
    for o in outs:
        assert torch.equal(o, torch.full_like(o, 7.0)), (entry, why)
    print(f"{entry} {case} ({why}): refused: {msg}")
