"""The planners over the accepted conv domain (include/avt.h), through their host queries avt_conv_fwd_plan
and avt_conv_wgrad_plan: no GPU, no launch (without a device the planners assume 256 CUs, the MI355X's count).

  * every case of exactconv.DOMAIN_2D / DOMAIN_DGRAD / DOMAIN_3D / DOMAIN_3D_DGRAD / DOMAIN_WGRAD gets a plan -- with an
    instantiation behind it, for the wgrads -- under every setting of the GPU files' sweeps;
  * every OUTSIDE shape the two queries can express is refused with a message;
  * taken together the off-grid cases reach the branches no ResNet-18 shape does (the k32 fallback of a 64-deep k-tile
    at C % 64 == 32, a GEMM N that is neither 64 nor a multiple of 128, wgrad column counts off the 128-column tile)
    and every forward family but the ResNet-only stem and c64 forms: halo, Conv3d three-patch halo, tap gather,
    register-staged;
  * the share of in-domain cases that run and compare is computed per entry point (EXPECTED_REFUSALS of the GPU files
    is empty: the share is 1).
The table of distinct plan tuples per case is printed (profiles/conv_domain.txt keeps a copy)."""
import ctypes

import pytest

import exactconv as ec
from avt_amd import _lib

FAMILY, WM, WN, TM, TN, NST, KP = range(7)          # avt_conv_fwd_plan
W_FAMILY, W_TN, W_FOUND = 0, 4, 23                  # avt_conv_wgrad_plan
C64, HALO, HALO3D, GATHER, REG, STEM = range(6)
FWD = list(ec.DOMAIN_2D)
DGRAD = list(ec.DOMAIN_DGRAD)
WGRAD = list(ec.DOMAIN_WGRAD)
FWD3 = list(ec.DOMAIN_3D)
DGRAD3 = list(ec.DOMAIN_3D_DGRAD)
EXPECTED_REFUSALS = {}  # as in the GPU files


@pytest.fixture(scope="module", autouse=True)
def _built():
    import os

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()


def _geom(case):
    """A Case's geometry without its draws."""
    class G:
        pass

    g = G()
    if len(case) == 12:
        g.N, g.T, g.H, g.W, g.C, g.K, g.KT, g.R, g.S, g.st, g.pad_t, g.pad = case
    else:
        g.N, g.H, g.W, g.C, g.K, g.R, g.S, g.st, g.pad = case
        g.T, g.KT, g.pad_t = 1, 1, 0
    g.Cw = g.C
    g.To = g.T + 2 * g.pad_t - g.KT + 1
    g.P, g.Q = ec.conv_out(g.H, g.R, g.st, g.pad), ec.conv_out(g.W, g.S, g.st, g.pad)
    return g


def _fwd_table(case, sweep, epi, dgrad=False):
    g = _geom(case)
    return ec.fwd_plans(g, g.C, sweep, epi, dgrad)  # raises if any setting of the sweep is refused


def _wgrad_table(case):
    g = _geom(case)
    seen = {}
    for mode, setting in ec.WGRAD_SWEEP:
        if any(n == "avt_set_stem_wgrad" for n, *_ in setting):
            continue
        ws_mode = {"null": 0, "tk": 2, "defer": 3}.get(mode, 1)
        with ec.Knobs(setting):
            p = ec.wgrad_plan(g, g.C, ws_mode)
        assert p[W_FOUND] == 1, (case, mode, setting, p)  # the launcher's table has the instantiation
        seen.setdefault(p, (mode, setting))
    return seen


def test_every_domain_case_plans_under_every_setting():
    """No setting of a sweep leaves an in-domain case without a plan; the table is printed."""
    ran = {}
    for name, cases, sweep, epi, dgrad in (
            ("conv2d_fwd", FWD, ec.FWD_SWEEP, 0, False),
            ("conv2d_fwd_bias", [c for c in FWD if c[5] * c[6] <= 9], ec.BIAS_SWEEP, 1, False),
            ("conv2d_fwd_ws", FWD, ec.FWD_SWEEP, 3, False),
            ("conv2d_dgrad (stride 1)", [c for c in DGRAD if c[7] == 1], ec.DGRAD_SWEEP[:len(ec.FWD_SWEEP)], 0, True),
            ("conv3d_fwd", FWD3, ec.SWEEP_3D, 0, False), ("conv3d_fwd_bias", FWD3, ec.SWEEP_3D, 2, False),
            ("conv3d_dgrad (stride 1)", [c for c in DGRAD3 if c[9] == 1], ec.SWEEP_3D, 0, True)):
        n = 0
        for case in cases:
            if (name, case) in EXPECTED_REFUSALS:
                continue
            plans = _fwd_table(case, sweep, epi, dgrad)
            assert plans
            n += 1
            print(f"{name} {case}: {len(plans)} plans: " + " ".join(str(p[:9]).replace(" ", "") for p, _ in plans))
        ran[name] = (n, len(cases))
    n = 0
    for case in WGRAD:
        table = _wgrad_table(case)
        n += 1
        print(f"conv2d_wgrad {case}: {len(table)} plans: "
              + " ".join(str(p[:5] + p[7:9] + p[11:15]).replace(" ", "") for p in table))
    ran["conv2d_wgrad"] = (n, len(WGRAD))
    for name, (n, total) in ran.items():  # the test cannot pass by refusing its way out
        assert 4 * n >= 3 * total, (name, n, total)
    print("share of in-domain cases that run:", {k: f"{a}/{b}" for k, (a, b) in ran.items()})


def test_off_grid_branches_are_reached():
    plans = {case: {p for p, _ in _fwd_table(case, ec.FWD_SWEEP, 0)} for case in FWD}
    # a 64-deep k-tile asked for (nt128 configs 1, 2, 4, 5; nt64 4 .. 8) at C % 64 == 32 falls back to the k32 tile:
    # no plan of such a case has kp 64, and the fallback's own tile (2, 2, 2, wn*tn/2, 3 stages, k32) is there
    odd = [c for c in FWD if c[3] % 64 == 32]
    assert odd
    for case in odd:
        g = [p for p in plans[case] if p[FAMILY] == GATHER]
        assert g and all(p[KP] == 32 for p in g), (case, g)
        assert any(p[1:7] == (2, 2, 2, 2 if case[4] % 128 == 0 else 1, 3, 32) for p in g), (case, g)
    even = [c for c in FWD if c[3] % 64 == 0 and not (c[5] == c[6] == 3 and c[7] == 1 and c[8] == 1)]
    assert any(p[KP] == 64 for c in even for p in plans[c] if p[FAMILY] == GATHER)  # (where it applies it is taken)
    # a GEMM N that is neither 64 nor a multiple of 128 takes the 64-wide tiles
    for case in [c for c in FWD if c[4] != 64 and c[4] % 128]:
        assert all(p[WN] * p[TN] * 32 == 64 for p in plans[case] if p[FAMILY] in (GATHER, REG)), (case, plans[case])
    assert {c[4] for c in FWD if c[4] != 64 and c[4] % 128} >= {192, 320}
    # every family but the ResNet-only stem and c64 forms (the Bottleneck 64 -> 64 3x3 is the c64 shape itself)
    fams = set().union(*({p[FAMILY] for p in ps} for ps in plans.values()))
    assert fams >= {HALO, GATHER, REG}, fams
    off = set().union(*({p[FAMILY] for p in plans[c]} for c in FWD if (c[3], c[4]) != (64, 64)))
    assert C64 not in off and STEM not in fams
    # Conv3d: the three-patch halo form on 3 chunks of 64 channels (C = 192, both of its tiles) and the tap gather
    f3 = {c: {p[FAMILY] for p, _ in _fwd_table(c, ec.SWEEP_3D, 0)} for c in FWD3}
    assert set().union(*f3.values()) == {HALO3D, GATHER}, f3
    assert {(c[4], c[5]) for c, f in f3.items() if HALO3D in f} >= {(192, 64), (192, 128)}
    patch = [p for c in FWD3 for p, _ in _fwd_table(c, ec.SWEEP_3D, 0) if p[FAMILY] == HALO3D]
    assert {p[1:5] for p in patch} >= {(8, 1, 1, 2), (4, 2, 2, 2)}, patch  # 256 x 64 and 256 x 128
    d3 = {c: {p[FAMILY] for p, _ in _fwd_table(c, ec.SWEEP_3D, 0, True)} for c in DGRAD3 if c[9] == 1}
    assert {(c[4], c[5]) for c, f in d3.items() if HALO3D in f} >= {(64, 192), (128, 192)}, d3
    # wgrad: column counts off the 128-column tile
    ncols = {c: c[5] * c[6] * c[3] for c in WGRAD}
    big = [c for c in WGRAD if ncols[c] % 128 and ncols[c] > 128]
    small = [c for c in WGRAD if ncols[c] < 64]
    assert big and small
    for case in big:
        assert all(p[W_TN] == 2 for p in _wgrad_table(case) if p[W_FAMILY] == 3), case  # BN 128, Ng rounded up
    for case in small:
        assert all(p[W_TN] == 1 for p in _wgrad_table(case) if p[W_FAMILY] == 3), case  # BN 64
    # the halo arms (nine taps, one filter row) at K = 192, C = 192 and the tap gather
    assert {1, 2, 3} <= {p[W_FAMILY] for c in WGRAD for p in _wgrad_table(c)}


def _refused(name, *args):
    rc = getattr(_lib.lib(), name)(*args)
    msg = _lib.lib().avt_last_error().decode()
    assert rc != 0 and msg.strip(), (name, args, rc, msg)  # (the wgrad query answers in the entry points' name)
    return msg


def test_outside_shapes_are_refused_by_the_queries():
    """What avt_conv_fwd_plan / avt_conv_wgrad_plan can express of exactconv.OUTSIDE: the forward entries' channel, tap
    and stride edges, the wgrad's.  (The dgrad's own edges, the aliasing rules and the Conv3d wgrad's temporal padding
    have no planner query: test_conv_domain_gpu.py / test_conv3d_domain_gpu.py make those calls.)"""
    out = (ctypes.c_int * 32)()
    n = 0
    for entry, case, why in ec.OUTSIDE:
        if "aliasing" in why or "dgrad" in entry or entry == "avt_conv3d_wgrad":
            continue
        if entry == "avt_conv2d_wgrad":
            N, H, W, C, K, R, S, st, pad = case
            msg = _refused("avt_conv_wgrad_plan", N, H, W, C, C, K, R, S, st, pad, 1, out)
        else:
            g = _geom(case)
            epi = 0 if entry.endswith("fwd") else 1 if entry == "avt_conv2d_fwd_bias" else 2
            if entry == "avt_conv2d_fwd_bias" and "taps" in why:
                continue  # the 9-tap bound is the entry point's: the planner sends a longer list to the Conv3d form
            msg = _refused("avt_conv_fwd_plan", g.N, g.T, g.H, g.W, g.C, g.K, g.KT, g.R, g.S, g.st, g.pad_t, g.pad, epi, out)
        print(f"{entry} {case} ({why}): {msg}")
        n += 1
    assert n >= 12, n
