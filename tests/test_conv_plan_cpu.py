"""The forward conv planner (plan_nt in csrc/conv_gemm.hip) through its host query avt_conv_fwd_plan: no GPU, no launch
(without a device the planner assumes 256 CUs).

Recorded plans: tests/golden/conv_plans.json holds what the commit BEFORE the planners were merged launched for every
conv of the two AVENet trunks (B = 128, 32, 1), of R3D-18 (8 clips and 1 clip of 16 x 224^2) and for the shapes of the
two bias-epilogue test files under their knobs -- through avt_conv2d_fwd / avt_conv3d_fwd (epi 0), avt_conv2d_fwd_ws
with the workspace avt_conv2d_splitk_plan sizes (3), avt_conv2d_fwd_bias (1) and avt_conv3d_fwd_bias (2).  It was
written by a build of that commit whose launch sites noted their template arguments instead of launching.

Agreement: a bias epilogue runs on the main loop the plain forward of the shape runs."""
import ctypes
import itertools
import json
import os

import pytest

from avt_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plans.json")
FAMILY, WM, WN, TM, TN, NST, KP, OPT, KSPLIT, EPI = range(10)
C64, HALO, HALO3D, GATHER, REG, STEM = range(6)
RESTORE = {"avt_set_halo8": -1, "avt_set_small_tiles": -2, "avt_set_halo": 1, "avt_set_c64": 1, "avt_set_halo3d": -1,
           "avt_set_nt128_config": -1}


class Knobs:
    def __init__(self, knobs):
        self.knobs = knobs

    def __enter__(self):
        for k, v in self.knobs.items():
            _lib.call(k, v)

    def __exit__(self, *exc):
        for k in self.knobs:
            _lib.call(k, RESTORE[k])


def plan(shape, epi):
    """avt_conv_fwd_plan of shape = (N, T, H, W, Cp, K, KT, R, S, stride, pad_t, pad) under the knobs as they stand."""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    out = (ctypes.c_int * 10)()
    _lib.call("avt_conv_fwd_plan", *shape, epi, out)
    return list(out)


def _entries():
    with open(GOLDEN) as f:
        return json.load(f)["entries"]


def test_query_reproduces_the_recorded_plans():
    entries = _entries()
    groups = {e["group"] for e in entries}
    assert len(entries) >= 600 and len(groups) == 10, (len(entries), sorted(groups))
    assert {e["plan"][FAMILY] for e in entries} == {C64, HALO, HALO3D, GATHER, STEM}
    assert any(e["plan"][KSPLIT] > 1 for e in entries)
    bad = []
    for e in entries:
        with Knobs(e["knobs"]):
            got = plan(e["shape"], e["epi"])
        if got != e["plan"]:
            bad.append((e["group"], e["name"], e["knobs"], e["shape"], e["epi"], "recorded", e["plan"], "now", got))
    assert not bad, bad[:10]


# the knob settings of tests/test_conv_bias_epi_gpu.py's FORMS and tests/test_conv3d_bias_epi_gpu.py's CASES; {} first
KNOB_SETS = [
    {},
    {"avt_set_halo8": 0, "avt_set_small_tiles": 0},
    {"avt_set_halo8": 1, "avt_set_small_tiles": 0},
    {"avt_set_halo": 2, "avt_set_c64": 0, "avt_set_small_tiles": 0},
    {"avt_set_small_tiles": -1},
    {"avt_set_small_tiles": 0},
    {"avt_set_halo": 0, "avt_set_small_tiles": 0},
    {"avt_set_halo": 0, "avt_set_small_tiles": -1},
    {"avt_set_c64": 0, "avt_set_small_tiles": 0},
    {"avt_set_halo3d": 2},
    {"avt_set_halo3d": 0},
]


def _grid():
    """Small shapes on both sides of every width bound (19, 39, 51, 79), K = 64 / 128 / 256, GEMM rows on both sides
    of 65536 (and one clip: the small-tile side), 2-D and Conv3d, stride 1 and 2."""
    for W, K, (T, KT), stride in itertools.product((19, 20, 39, 40, 51, 52, 79, 80), (64, 128, 256), ((1, 1), (4, 3)),
                                                   (1, 2)):
        H = 8
        rows = T * (H // stride) * ((W - 1) // stride + 1)  # output rows per clip (3x3 / pad 1)
        below = 65535 // rows
        for N in (1, below, below + 1):
            yield (N, T, H, W, K, K, KT, 3, 3, stride, KT // 2, 1)


def test_grid_covers_both_sides_of_the_row_bound():
    shapes = list(_grid())
    ms = [s[0] * s[1] * ((s[2] - 1) // s[9] + 1) * ((s[3] - 1) // s[9] + 1) for s in shapes]  # N * T * OH * OW
    for i in range(0, len(shapes), 3):  # (one clip, the last batch below 65536 rows, the first from it)
        assert ms[i] < ms[i + 1] < 65536 <= ms[i + 2], (shapes[i + 1], ms[i + 1], ms[i + 2])


@pytest.mark.parametrize("knobs", KNOB_SETS, ids=lambda k: ",".join(f"{n[8:]}={v}" for n, v in k.items()) or "default")
def test_bias_plan_is_the_plain_plan(knobs):
    """Family, tile and k-tile depth / patch rows of the bias plan are the plain forward's, for both bias entry points,
    unless the plain call took split-K or a two-taps-per-barrier form (plain only); at default knobs the stages too."""
    bad, n = [], 0
    with Knobs(knobs):
        for shape in _grid():
            two_d = shape[1] == 1 and shape[6] == 1
            for plain_epi in (0, 3):
                want = plan(shape, plain_epi)
                assert want[EPI] == 0
                if want[KSPLIT] > 1 or want[OPT] in (3, 7):
                    continue
                for epi in ((1, 2) if two_d else (2,)):
                    got = plan(shape, epi)
                    n += 1
                    assert got[EPI] == (1 if two_d else 2) and got[KSPLIT] == 1
                    same = [FAMILY, WM, WN, TM, TN, KP] + ([NST] if not knobs else [])
                    if [got[i] for i in same] != [want[i] for i in same]:
                        bad.append((shape, "plain", plain_epi, want, "bias", epi, got))
    assert n > 500 and not bad, bad[:10]


def test_bias_plan_ignores_the_tile_overrides():
    """The canonical rule: a tile override moves the plain forward to another tile and leaves the bias epilogue on the
    default one (a zero bias then equals the plain forward at default knobs: tests/test_conv_bias_epi_gpu.py)."""
    shape = (1, 1, 7, 7, 256, 256, 1, 3, 3, 1, 0, 1)
    base = {"avt_set_halo": 0, "avt_set_small_tiles": 0}
    with Knobs(base):
        plain_default = plan(shape, 0)
    with Knobs(dict(base, avt_set_nt128_config=3)):
        plain, b2, b3 = plan(shape, 0), plan(shape, 1), plan(shape, 2)
    assert plain_default[:KSPLIT] == [GATHER, 2, 2, 2, 2, 2, 64, 0]   # 128 x 128, k64, 2 stages
    assert plain[:KSPLIT] == [GATHER, 2, 2, 4, 2, 3, 32, 0]           # config 3: 256 x 128, k32, 3 stages
    assert b2[:KSPLIT] == b3[:KSPLIT] == plain_default[:KSPLIT] and b2[EPI] == b3[EPI] == 1


def test_query_refusals():
    out = (ctypes.c_int * 10)()
    good = (1, 1, 7, 7, 256, 256, 1, 3, 3, 1, 0, 1)
    for bad, msg in (((1, 1, 7, 7, 256, 96, 1, 3, 3, 1, 0, 1), "multiple of 64"),
                     ((1, 1, 7, 7, 48, 64, 1, 3, 3, 1, 0, 1), "unsupported"),
                     ((1, 1, 7, 7, 256, 256, 1, 3, 3, 3, 0, 1), "stride"),
                     ((1, 1, 1, 1, 256, 256, 1, 3, 3, 1, 0, 0), "empty output"),
                     ((1 << 16, 4, 1 << 10, 11, 64, 128, 3, 3, 3, 2, 1, 1), "2 GiB")):
        with pytest.raises(RuntimeError, match=msg):
            _lib.call("avt_conv_fwd_plan", *bad, 0, out)
    with pytest.raises(RuntimeError, match="epi"):
        _lib.call("avt_conv_fwd_plan", *good, 4, out)
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.call("avt_conv_fwd_plan", *good, 0, None)
    with pytest.raises(RuntimeError, match="unsupported"):  # a stem has no bias epilogue
        _lib.call("avt_conv_fwd_plan", 1, 1, 64, 64, 4, 64, 1, 7, 7, 2, 0, 3, 1, out)
