"""The 2-D wgrad planner (plan_wgrad in csrc/conv_gemm.hip) through its host query avt_conv_wgrad_plan: no GPU, no launch
(without a device the planner assumes 256 CUs).

Recorded plans: tests/golden/wgrad_plans.json holds what the commit BEFORE the one plan launched for every conv of the
two AVENet trunks (B = 128, 64, 32, 1, stems included), the 2-D wgrads of the tube step, and the geometries of
test_conv_exact_gpu.py's wgrad sweep, test_wgrad_pixtab_gpu.py and test_kernels_gpu.py's wgrad tests under their knob
sets -- each with no workspace (ws_mode 0), the workspace the size query gives (1), that and the tickets (2), that and
a defer descriptor (3).  It was written by a build of that commit whose wgrad and reduce launch sites noted their
kernel, template arguments, grid and block instead of launching.

Consistency: the two size queries, the plan and the launcher's table agree over the same grid."""
import ctypes
import json
import os

import pytest

from avt_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_plans.json")
INTS = 24
(FAMILY, WM, WN, TM, TN, RW, PRMAX, NST, KG, PF, TAB, SPLITS, KPS, TILES, PARTIALS, SLAB_LO, SLAB_HI, TICKETS, G, RED_GRID,
 RED_BLOCK, GROUPS, PER_GROUP, FOUND) = range(INTS)
STEM, HALO9, ROW3, GATHER, REG = range(5)
SLAB_REDUCE, SLAB_FUSED, SLAB_DEFER, ATOMICS = range(4)
RESTORE = {"avt_set_wgrad_tiles": (1,), "avt_set_wgrad_halo": (-1,), "avt_set_wgrad_row3": (-1, -1, -1),
           "avt_set_wgrad_nst": (4, 3), "avt_set_stem_wgrad": (1,), "avt_set_wgrad_policy": (0, 4),
           "avt_set_wgrad_slab_max": (1 << 30, 16), "avt_set_wgrad_slots_pct": (-1,), "avt_set_wgrad_fused": (-1, -1),
           "avt_set_conv_variant": (1,), "avt_set_wgrad_pixtab": (-1,)}


class Knobs:
    def __init__(self, knobs):
        self.knobs = knobs

    def __enter__(self):
        for name, *args in self.knobs:
            _lib.call(name, *args)

    def __exit__(self, *exc):
        for name, *_ in self.knobs:
            _lib.call(name, *RESTORE[name])


def plan(shape, ws_mode):
    """avt_conv_wgrad_plan of shape = (N, H, W, Cp, Creal, K, R, S, stride, pad) under the knobs as they stand."""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    out = (ctypes.c_int * INTS)()
    _lib.call("avt_conv_wgrad_plan", *shape, ws_mode, out)
    return list(out)


def slab_bytes(p):
    return p[SLAB_LO] + (p[SLAB_HI] << 31)


_GOLDEN = {}


def _golden():
    """(knob sets, entries [group, knob set index, shape, ws_mode, plan] grouped by knob set): read once."""
    if not _GOLDEN:
        with open(GOLDEN) as f:
            g = json.load(f)
        entries = [[group, ks, shape, mode, plans[which[mode]]]
                   for group, ks, items in g["records"] for shape, plans, which in items for mode in range(4)]
        by = {}
        for e in entries:
            by.setdefault(e[1], []).append(e)
        _GOLDEN.update(knobsets=g["knobsets"], by=by, entries=entries, commit=g["recorded_from"])
    return _GOLDEN


def test_golden_covers_every_form():
    """The golden cannot shrink to the easy cases: the recorder wrote 5636 entries."""
    g = _golden()
    plans = [e[4] for e in g["entries"]]
    assert len(plans) >= 5636 and g["commit"]
    assert {e[0] for e in g["entries"]} >= {f"{t}_b{b}" for t in ("vision", "audio") for b in (128, 64, 32, 1)} | {
        "tube", "exact", "pixtab", "kernels"}
    assert {e[3] for e in g["entries"]} == {0, 1, 2, 3}
    assert {p[FAMILY] for p in plans} == {STEM, HALO9, ROW3, GATHER, REG}
    assert {p[PARTIALS] for p in plans} == {SLAB_REDUCE, SLAB_FUSED, SLAB_DEFER, ATOMICS}
    assert {p[KG] for p in plans if p[FAMILY] == GATHER} == {1, 2}
    assert {p[KG] for p in plans if p[FAMILY] == ROW3} == {1, 2, 4}
    assert {p[PF] for p in plans if p[FAMILY] == ROW3 and p[KG] == 2 and p[WM] == 1} == {0, 1}
    assert {p[NST] for p in plans if p[FAMILY] == GATHER} == {3, 4, 5, 6, 8}
    assert {(4, 2, 2, 4), (4, 2, 2, 2), (2, 2, 2, 2), (2, 2, 2, 1), (2, 2, 1, 2), (2, 2, 1, 1)} <= {
        tuple(p[WM:TN + 1]) for p in plans if p[FAMILY] == GATHER}
    assert {p[TAB] for p in plans if p[FAMILY] == GATHER} == {0, 1}
    assert any(p[G] > 1 for p in plans) and any(p[GROUPS] > 1 for p in plans)


def test_query_reproduces_the_recorded_plans():
    g = _golden()
    bad = []
    for ks, entries in g["by"].items():
        with Knobs(g["knobsets"][ks]):
            for group, _, shape, ws_mode, want in entries:
                got = plan(shape, ws_mode)
                if got != want:
                    bad.append((group, g["knobsets"][ks], shape, ws_mode, "recorded", want, "now", got))
    assert not bad, (len(bad), bad[:10])


def test_queries_plan_and_launcher_agree():
    """avt_conv2d_wgrad_workspace is the workspace plan's slab, avt_conv2d_wgrad_tickets the ticket plan's tickets; no
    workspace, no slab; a slab only as large as the workspace; every plan has its instantiation."""
    g = _golden()
    bad, n = [], 0
    for ks, entries in g["by"].items():
        with Knobs(g["knobsets"][ks]):
            for shape in sorted({tuple(e[2]) for e in entries}):
                ws = int(_lib.query("avt_conv2d_wgrad_workspace", *shape))
                tk = int(_lib.query("avt_conv2d_wgrad_tickets", *shape))
                p = [plan(shape, m) for m in range(4)]
                n += 1
                ok = (slab_bytes(p[0]) == 0 and p[0][PARTIALS] == ATOMICS and p[0][TICKETS] == 0
                      and all(slab_bytes(q) == ws for q in p[1:]) and p[2][TICKETS] == tk
                      and p[1][TICKETS] == p[3][TICKETS] == 0 and all(q[FOUND] == 1 for q in p)
                      and (p[2][PARTIALS] == SLAB_FUSED) == (tk > 0) and p[1][PARTIALS] != SLAB_DEFER
                      and all((q[PARTIALS] == ATOMICS) == (slab_bytes(q) == 0) for q in p)
                      and all(q[SPLITS] >= 1 and q[TILES] >= 1 for q in p))
                if not ok:
                    bad.append((g["knobsets"][ks], shape, ws, tk, p))
    assert n > 500 and not bad, (len(bad), bad[:5])


def test_ring_depth_launched_and_planned():
    """avt_set_wgrad_nst's 5 and 7 launch the 4- and 6-stage instantiations, and plan their splits as 5 and 7 do: the
    4-stage ring alone pairs its blocks into two k groups."""
    shape = (32, 28, 28, 128, 128, 128, 3, 3, 1, 1)
    with Knobs([("avt_set_wgrad_halo", 0)]):
        base = plan(shape, 1)
        assert base[NST] == 4 and base[KG] == 2
        for nst, launched in ((5, 4), (6, 6), (7, 6), (8, 8)):
            with Knobs([("avt_set_wgrad_nst", nst, 3)]):
                p = plan(shape, 1)
            assert (p[FAMILY], p[NST], p[KG], p[FOUND]) == (GATHER, launched, 1, 1), (nst, p)
            assert p[TAB] == (1 if launched == 4 else 0)


def test_query_refusals():
    out = (ctypes.c_int * INTS)()
    good = (2, 9, 11, 64, 64, 128, 3, 3, 1, 1)
    for bad, msg in (((2, 9, 11, 64, 64, 96, 3, 3, 1, 1), "conv2d_wgrad: K=96 must be a multiple of 64"),
                     ((2, 9, 11, 12, 12, 64, 3, 3, 1, 1), "conv2d_wgrad: C=12 unsupported"),
                     ((2, 9, 11, 4, 5, 64, 7, 7, 2, 3), "conv2d_wgrad: Creal > Cp"),
                     ((2, 9, 11, 64, 48, 64, 3, 3, 1, 1), "conv2d_wgrad: channel padding only for the stems"),
                     ((2, 9, 11, 64, 64, 64, 3, 3, 3, 1), "stride"),
                     ((2, 1, 1, 64, 64, 64, 3, 3, 1, 0), "empty"),
                     ((0, 9, 11, 64, 64, 64, 3, 3, 1, 1), "empty")):
        with pytest.raises(RuntimeError, match=msg):
            _lib.call("avt_conv_wgrad_plan", *bad, 1, out)
    for mode in (-1, 4):
        with pytest.raises(RuntimeError, match="ws_mode"):
            _lib.call("avt_conv_wgrad_plan", *good, mode, out)
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.call("avt_conv_wgrad_plan", *good, 0, None)
