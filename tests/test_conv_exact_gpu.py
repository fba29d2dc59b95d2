"""The 2-D conv family pinned term by term: every kernel form and every A/B knob of avt_conv2d_fwd / _fwd_bias / _fwd_ws,
avt_conv2d_dgrad / _dgrad_mask / _dgrad_ws / _dgrad_bn, avt_conv_stem_dgrad and avt_conv2d_wgrad / _wgrad_tk /
_wgrad_defer on operands whose sums are exact in fp32 in ANY order (tests/exactconv.py), compared for EQUALITY with the
fp64 torch reference.  One dropped, duplicated or misplaced term moves an output by a whole unit; there is no noise
to tolerate, so there is no tolerance here other than the BN accumulator's M2 column (its fp32 mean is not exact:
test_conv_fwd_and_bn_partials' rtol).  tests/test_exactconv_cpu.py sizes the draws and checks the instrument.

Knob sweeps are deduplicated through avt_conv_fwd_plan: a setting whose plan tuple the case has already run is not
launched again.  Each test prints the number of distinct plans it ran and the share of outputs above 255."""
import ctypes

import pytest
import torch

import exactconv as ec
from avt_amd._lib import DgradBnEpi, call, query

pytestmark = pytest.mark.gpu
DEV = "cuda"
P, S, Knobs, _tag = ec.P, ec.S, ec.Knobs, ec.tag


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    ec.KEEP.clear()


FWD_SWEEP, BIAS_SWEEP, DGRAD_SWEEP = ec.FWD_SWEEP, ec.BIAS_SWEEP, ec.DGRAD_SWEEP  # shared with test_conv_domain_gpu.py

CASES = ec.cases_2d()
STEMS = ec.STEM_CASES
_RAN = {}   # case -> the kernel families its forward test launched
_PATHS = {}  # wgrad mode -> the cases on which its own path was taken (tickets issued, two slabs batched)
_WGRAD_RAN = set()
_OPS = {}


def _cp(c):
    return c.C if c.C % 8 == 0 else (4 if c.C == 3 else 1)


def _pad_c(t, cp):
    if t.shape[-1] == cp:
        return t
    return torch.cat([t, torch.zeros(t.shape[:-1] + (cp - t.shape[-1],))], -1)


def _ops(case):
    """Device operands of a case, made once: bf16 activations (stems: zero-padded to Cp channels), the packed forward
    and dgrad weight images."""
    if case not in _OPS:
        c = ec.get_case(case)
        cp = _cp(c)
        rs = c.R * c.S
        kg = rs * cp if cp % 8 == 0 else (rs * cp + 31) // 32 * 32
        w = c.w.to(DEV)
        wf = torch.empty(c.K, kg, device=DEV, dtype=torch.bfloat16)
        wt = torch.empty(c.C, rs * c.K, device=DEV, dtype=torch.bfloat16) if cp % 8 == 0 else None
        call("avt_pack_conv_weight", P(w), c.K, c.R, c.S, c.C, cp, kg, P(wf), P(wt), S())
        torch.cuda.synchronize()
        bf = lambda t: t.to(torch.bfloat16).to(DEV)
        _OPS[case] = dict(cp=cp, kg=kg, wf=wf, wt=wt, x=bf(_pad_c(c.x, cp)), xg=bf(_pad_c(c.xg, cp)), dy=bf(c.dy),
                          dyg=bf(c.dyg), add=bf(c.add), res=bf(c.res), bias=c.bias.to(DEV), bits=c.bits.to(DEV))
    return _OPS[case]


_plan, _nan = ec.fwd_plan, ec.nan_tensor


def _geo(c, cp):
    return (c.N, c.H, c.W, cp, c.K, c.R, c.S, c.st, c.pad)


def _fwd_plans(case, sweep, epi):
    """[(plan, setting)] of the settings whose plan tuple differs from every earlier one (host queries only)."""
    c = ec.get_case(case)
    return ec.fwd_plans(c, _cp(c), sweep, epi)


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + STEMS, ids=str)
def test_fwd_every_plan(case, record=True):
    """avt_conv2d_fwd with and without the BN accumulator, once per distinct plan of the knob sweep: y == bf16_rne(fp64
    conv) everywhere, the accumulator's column sums == the reference's exactly."""
    c = ec.get_case(case)
    fig = c.figures("y")
    o = _ops(case)
    ref = c.ref("y")
    if case in STEMS:
        assert fig["above255"] == 0  # the stem kernel takes the statistics of the stored bf16 tensor: the same integers
    plans = _fwd_plans(case, FWD_SWEEP, 0)
    for plan, setting in plans:
        with Knobs(setting):
            for with_acc in (True, False):
                y = _nan(c.N, c.P, c.Q, c.K)
                acc = None
                if with_acc:
                    acc = _nan(int(query("avt_bn_acc_doubles", c.N * c.P * c.Q, c.K)), dtype=torch.float64)
                call("avt_conv2d_fwd", P(o["x"]), P(o["wf"]), P(y), P(acc), *_geo(c, o["cp"]), o["kg"], S())
                torch.cuda.synchronize()
                what = f"fwd {case} [{_tag(setting)}] plan {plan} acc={with_acc}"
                ec.assert_bf16(y, ref, what)
                if with_acc:
                    ec.assert_fwd_acc(acc, ref, what)
    fams = {p[0] for p, _ in plans}
    if record:  # (test_conv_domain_gpu.py runs this body on its own cases and keeps its own record)
        _RAN[case] = fams
    print(f"fwd {case}: {len(plans)} distinct plans, families {sorted(fams)}, above 255: {fig['above255']:.2e}")


def test_every_2d_family_is_reached():
    """Families 0 (c64), 1 (halo), 3 (tap gather), 4 (register-staged) and 5 (stem) of avt_conv_fwd_plan each run on at
    least one case of test_fwd_every_plan (family 2, the Conv3d three-patch form: test_conv3d_exact_gpu.py) -- a planner
    change cannot silently empty a branch."""
    fams = set()
    for case in CASES + STEMS:
        fams |= {p[0] for p, _ in _fwd_plans(case, FWD_SWEEP, 0)}
    assert fams >= {0, 1, 3, 4, 5}, fams
    if len(_RAN) == len(CASES + STEMS):  # the whole file ran: what was launched, not only what would be
        assert set().union(*_RAN.values()) >= {0, 1, 3, 4, 5}, _RAN


@pytest.mark.parametrize("case", CASES, ids=str)
def test_fwd_bias_every_plan(case):
    """avt_conv2d_fwd_bias with an integer bias, without and with residual + ReLU.  The bias joins the fp32 accumulator
    before the first rounding; the residual joins the rounded value (one rounding in the layer-1 kernel: there both
    orders must be the identity)."""
    c = ec.get_case(case)
    fig = c.figures("y")
    o = _ops(case)
    v = ec.bf16_rne(c.ref("y") + c.bias.double())
    want = {False: v, True: ec.bf16_rne(v + c.res.double()).clamp_min(0)}
    plans = _fwd_plans(case, BIAS_SWEEP, 1)
    for plan, setting in plans:
        if plan[0] == 0:
            assert fig["one_rounding_safe"], case
        with Knobs(setting):
            for full in (False, True):
                y = _nan(c.N, c.P, c.Q, c.K)
                call("avt_conv2d_fwd_bias", P(o["x"]), P(o["wf"]), P(y), *_geo(c, o["cp"]), o["kg"], P(o["bias"]),
                     P(o["res"]) if full else None, int(full), S())
                torch.cuda.synchronize()
                ec.assert_rounded(y, want[full], f"fwd_bias {case} [{_tag(setting)}] plan {plan} res+relu={full}")
    print(f"fwd_bias {case}: {len(plans)} distinct plans, above 255: {fig['above255']:.2e}")


SPLITK = [c for c in CASES if c[5] == 3 and c[6] == 1 and c[3] % 64 == 0 and c[4] % 128 == 0 and c[0] <= 8]


def _splitk_ws(c, dgrad):
    nf, nc = ctypes.c_longlong(0), ctypes.c_int(0)
    call("avt_conv2d_splitk_plan", c.N, c.H, c.W, c.C, c.K, 3, 3, 1, 1, int(dgrad), ctypes.byref(nf), ctypes.byref(nc))
    part = torch.empty(max(nf.value, 1), device=DEV)
    cnt = torch.zeros(max(nc.value, 1), device=DEV, dtype=torch.int32)
    return part, nf.value, cnt, nc.value


@pytest.mark.parametrize("ks", [2, 4, 8])
@pytest.mark.parametrize("case", SPLITK, ids=str)
def test_splitk_equals_unsplit(case, ks):
    """avt_conv2d_fwd_ws / avt_conv2d_dgrad_ws under avt_set_halo_splitk(ks, 0): the split partials sum to the unsplit
    answer exactly (forward with its BN accumulator; dgrad plain, + add, + masked add); the tickets are left zero."""
    c = ec.get_case(case)
    c.figures("y"), c.figures("dx")
    o = _ops(case)
    keep = ec.mask_from_bits(c.bits, c.x.shape)
    dxs = {"plain": ec.bf16_rne(c.ref("dx")), "add": ec.rne2(c.ref("dx"), c.add),
           "mask": ec.rne2(c.ref("dx"), torch.where(keep, c.add, torch.zeros_like(c.add)))}
    with Knobs([("avt_set_halo_splitk", ks, 0)]):
        split = _plan(c, c.C, 3)[8]
        part, nf, cnt, nc = _splitk_ws(c, False)
        y = _nan(c.N, c.P, c.Q, c.K)
        acc = _nan(int(query("avt_bn_acc_doubles", c.N * c.P * c.Q, c.K)), dtype=torch.float64)
        call("avt_conv2d_fwd_ws", P(o["x"]), P(o["wf"]), P(y), P(acc), *_geo(c, c.C), o["kg"], P(part), nf, P(cnt), nc,
             S())
        torch.cuda.synchronize()
        what = f"fwd_ws {case} ks={ks} (plan split {split}, {nc} tickets)"
        ec.assert_bf16(y, c.ref("y"), what)
        ec.assert_fwd_acc(acc, c.ref("y"), what)
        assert int(cnt.abs().max()) == 0, what
        part, nf, cnt, nc = _splitk_ws(c, True)
        for mode, want in dxs.items():
            dx = _nan(c.N, c.H, c.W, c.C)
            call("avt_conv2d_dgrad_ws", P(o["dy"]), P(o["wt"]), P(dx), P(o["add"]) if mode != "plain" else None,
                 P(o["bits"]) if mode == "mask" else None, *_geo(c, c.C), P(part), nf, P(cnt), nc, S())
            torch.cuda.synchronize()
            ec.assert_rounded(dx, want, f"dgrad_ws {mode} {case} ks={ks} ({nc} tickets)")
        assert int(cnt.abs().max()) == 0
    if c.C >= 256 and c.C % 128 == 0 and c.W <= 19:  # (a dgrad of C % 128 != 0 has no 128-wide halo tile to split)
        assert split > 1 and nc > 0, (case, ks, split, nc)  # the layer3/4 shapes do split
    print(f"splitk {case} ks={ks}: forward split {split}, dgrad tickets {nc}")


# ---------------------------------------------------------------------------------------------------------------------
# dgrad
# ---------------------------------------------------------------------------------------------------------------------
def _dgrad_settings(case):
    """The sweep deduplicated by the plan of the stride-1 dgrad's forward form; a strided dgrad (parity classes, no
    plan query) runs the settings that reach it."""
    c = ec.get_case(case)
    if c.st == 1:
        seen, out = set(), []
        for setting in DGRAD_SWEEP:
            if any(n == "avt_set_s2_dgrad_one" or n == "avt_set_stem_kernel" for n, *_ in setting):
                continue
            with Knobs(setting):
                plan = _plan(c, c.C, 0, dgrad=True)
            if plan not in seen or c.R != c.S:  # (the query takes one pad: at R != S its tuple is no key, all run)
                seen.add(plan)
                out.append((plan, setting))
        return out
    names = {"avt_set_conv_variant", "avt_set_small_tiles", "avt_set_s2_dgrad_one", "avt_set_halo",
             "avt_set_nt128_config" if c.C % 128 == 0 else "avt_set_nt64_config"}
    return [(None, s) for s in DGRAD_SWEEP if all(n in names for n, *_ in s)]


@pytest.mark.parametrize("case", CASES, ids=str)
def test_dgrad_every_plan(case):
    """avt_conv2d_dgrad plain, + add, + add aliasing dx, and avt_conv2d_dgrad_mask with random bits: each equals the
    fp64 conv2d_input (the add joining the rounded result) exactly, under every distinct plan of the sweep."""
    c = ec.get_case(case)
    fig = c.figures("dx")
    o = _ops(case)
    keep = ec.mask_from_bits(c.bits, c.x.shape)
    plain, added = ec.bf16_rne(c.ref("dx")), ec.rne2(c.ref("dx"), c.add)
    masked = ec.rne2(c.ref("dx"), torch.where(keep, c.add, torch.zeros_like(c.add)))
    settings = _dgrad_settings(case)
    g = (c.N, c.H, c.W, c.C, c.K, c.R, c.S, c.st, c.pad)
    for plan, setting in settings:
        with Knobs(setting):
            dx, dxa, dxm = _nan(*c.x.shape), _nan(*c.x.shape), _nan(*c.x.shape)
            dxi = o["add"].clone()
            call("avt_conv2d_dgrad", P(o["dy"]), P(o["wt"]), P(dx), None, *g, S())
            call("avt_conv2d_dgrad", P(o["dy"]), P(o["wt"]), P(dxa), P(o["add"]), *g, S())
            call("avt_conv2d_dgrad", P(o["dy"]), P(o["wt"]), P(dxi), P(dxi), *g, S())
            call("avt_conv2d_dgrad_mask", P(o["dy"]), P(o["wt"]), P(dxm), P(o["add"]), P(o["bits"]), *g, S())
            torch.cuda.synchronize()
            what = f"{case} [{_tag(setting)}] plan {plan}"
            ec.assert_rounded(dx, plain, "dgrad " + what)
            ec.assert_rounded(dxa, added, "dgrad + add " + what)
            ec.assert_rounded(dxi, added, "dgrad in place " + what)
            ec.assert_rounded(dxm, masked, "dgrad_mask " + what)
    print(f"dgrad {case}: {len(settings)} distinct plans / settings, above 255: {fig['above255']:.2e}")


NO_SMALL = [("avt_set_c64", 0), ("avt_set_small_tiles", 0)]


def _dgrad_bn_settings(case):
    """DGRAD_SWEEP for a dgrad that carries the BN-backward epilogue, deduplicated the same way.  plan_nt gives such a
    call neither the layer-1 kernel nor a 64-row tile, so its plan is the plain dgrad's under avt_set_c64(0) and
    avt_set_small_tiles(0): that tuple is the key.  The register-staged variant has no such epilogue (it refuses:
    test_dgrad_bn_epilogue_needs_lds_dma_kernels); a strided dgrad has no plan query and runs the settings that
    reach it, every tile config of its width included."""
    c = ec.get_case(case)
    sweep = [s for s in DGRAD_SWEEP if not any(n in ("avt_set_conv_variant", "avt_set_stem_kernel") for n, *_ in s)]
    if c.st != 1:
        names = {"avt_set_small_tiles", "avt_set_s2_dgrad_one", "avt_set_halo",
                 "avt_set_nt128_config" if c.C % 128 == 0 else "avt_set_nt64_config"}
        return [(None, s) for s in sweep if all(n in names for n, *_ in s)]
    seen, out = set(), []
    for setting in sweep:
        if any(n == "avt_set_s2_dgrad_one" for n, *_ in setting):
            continue
        with Knobs(setting):
            with Knobs(NO_SMALL):
                plan = _plan(c, c.C, 0, dgrad=True)
        if plan not in seen or c.R != c.S:
            seen.add(plan)
            out.append((plan, setting))
    return out


def _bn_operands(case):
    c = ec.get_case(case)
    xc, xc2 = ec.ints(c.x.shape, -3, 3, case, "xc"), ec.ints(c.x.shape, -3, 3, case, "xc2")
    y = ec.ints(c.x.shape, -2, 2, case, "y")
    return xc, xc2, y, ec.exact_bn_stats(c.C, (case, 1)), ec.exact_bn_stats(c.C, (case, 2))


@pytest.mark.parametrize("mode", ["relu_fma", "mask_y", "two_bn"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_dgrad_bn_epilogue(case, mode):
    """avt_conv2d_dgrad_bn with statistics chosen so that everything stays exact (scale in {+-1/2, +-1, +-2}, shift in
    halves, integer mean, invstd in {1/2, 1, 2}; xc, xc2, y small integers): g' is the masked integers, and both
    accumulator columns equal the reference totals exactly -- for acc and, with two BNs, acc2.  Under every distinct
    plan of the dgrad sweep (_dgrad_bn_settings): each tile instantiates its own epilogue and its own reduction
    partition (4-wave and 8-wave, 128- and 256-row, 64- and 128-wide)."""
    c = ec.get_case(case)
    c.figures("dx")
    o = _ops(case)
    xc, xc2, y, st, st2 = _bn_operands(case)
    two = mode == "two_bn"
    g = ec.bf16_rne(c.ref("dx")) if two else ec.rne2(c.ref("dx"), c.add)
    refs = ec.dgrad_bn_ref(g, xc, st, y if mode == "mask_y" else None, xc2 if two else None, st2 if two else None)
    bf = lambda t: t.to(torch.bfloat16).to(DEV)
    xcd, xc2d, yd, std, st2d = bf(xc), bf(xc2), bf(y), st.to(DEV), st2.to(DEV)
    rows = c.N * c.H * c.W
    settings = _dgrad_bn_settings(case)
    for plan, setting in settings:
        with Knobs(setting):
            acc = torch.full((int(query("avt_bn_bwd_workspace", rows, c.C)),), 255, device=DEV, dtype=torch.uint8)
            acc2 = torch.full_like(acc, 255)
            e = DgradBnEpi()
            e.xc, e.stats, e.acc = P(xcd).value, P(std).value, P(acc).value
            e.y = P(yd).value if mode == "mask_y" else None
            if two:
                e.xc2, e.stats2, e.acc2 = P(xc2d).value, P(st2d).value, P(acc2).value
            dx = _nan(*c.x.shape)
            call("avt_conv2d_dgrad_bn", P(o["dy"]), P(o["wt"]), P(dx), None if two else P(o["add"]), c.N, c.H, c.W, c.C,
                 c.K, c.R, c.S, c.st, c.pad, ctypes.byref(e), S())
            torch.cuda.synchronize()
            what = f"dgrad_bn {mode} {case} [{_tag(setting)}] plan {plan}"
            ec.assert_rounded(dx, refs[0], what)
            a = ec.bwd_acc_sums(acc, c.C)
            for col, want in ((0, refs[1]), (1, refs[2])):
                rep = ec.mismatches(a[:, col], want, channels_last=False)
                assert not rep, f"{what}: acc column {col}\n{rep}"
            if two:
                b = ec.bwd_acc_sums(acc2, c.C)
                for col, want in ((0, refs[1]), (1, refs[3])):
                    rep = ec.mismatches(b[:, col], want, channels_last=False)
                    assert not rep, f"{what}: acc2 column {col}\n{rep}"
    print(f"dgrad_bn {mode} {case}: {len(settings)} distinct plans / settings")


@pytest.mark.parametrize("case", [(2, 9, 11, 64, 128, 3, 2, 1), (2, 15, 13, 64, 128, 3, 2, 1)], ids=str)
def test_dgrad_bn_skip00_then_append(case):
    """A first block's input gradient: the 3x3/s2 dgrad stores its (even, even) pixels plain (skip_class00), the in-place
    1x1/s2 downsample dgrad adds to them and appends its slots (append_slots): the union is the masked sum of both
    dgrads and the slot sums cover every pixel once -- exactly, under the default plan and every tile config of the
    sweep that reaches a strided dgrad."""
    c = ec.get_case(case)
    c.figures("dx")
    o = _ops(case)
    xc, _, y, st, _ = _bn_operands(case)
    dyd = ec.signs(c.dy.shape, 2.0 / 3, case, "dyd")
    wd = ec.signs((c.K, 1, 1, c.C), 2.0 / 3, case, "wd")
    convd = torch.nn.grad.conv2d_input((c.N, c.C, c.H, c.W), wd.double().permute(0, 3, 1, 2),
                                       dyd.double().permute(0, 3, 1, 2), stride=2, padding=0).permute(0, 2, 3, 1)
    assert float(convd.abs().max()) <= 255
    g = ec.rne2(convd, ec.bf16_rne(c.ref("dx")))
    gm, s1, s2 = ec.dgrad_bn_ref(g, xc, st, y)
    wtd = torch.empty(c.C, c.K, device=DEV, dtype=torch.bfloat16)
    wfd = torch.empty(c.K, c.C, device=DEV, dtype=torch.bfloat16)
    call("avt_pack_conv_weight", P(wd.to(DEV)), c.K, 1, 1, c.C, c.C, c.C, P(wfd), P(wtd), S())
    bf = lambda t: t.to(torch.bfloat16).to(DEV)
    xcd, yd, std, dydd = bf(xc), bf(y), st.to(DEV), bf(dyd)
    settings = _dgrad_bn_settings(case)  # the default and, with the halo off, every tile config of the 64-wide GEMM
    assert len(settings) >= 10, settings
    for _, setting in settings:
        with Knobs(setting):
            acc = torch.full((int(query("avt_bn_bwd_workspace", c.N * c.H * c.W, c.C)),), 255, device=DEV, dtype=torch.uint8)
            e = DgradBnEpi()
            e.xc, e.y, e.stats, e.acc = P(xcd).value, P(yd).value, P(std).value, P(acc).value
            e.skip_class00 = 1
            dx = _nan(*c.x.shape)
            call("avt_conv2d_dgrad_bn", P(o["dy"]), P(o["wt"]), P(dx), None, c.N, c.H, c.W, c.C, c.K, 3, 3, 2, 1, ctypes.byref(e),
                 S())
            e.skip_class00, e.append_slots = 0, 1
            call("avt_conv2d_dgrad_bn", P(dydd), P(wtd), P(dx), P(dx), c.N, c.H, c.W, c.C, c.K, 1, 1, 2, 0, ctypes.byref(e), S())
            torch.cuda.synchronize()
            ec.assert_rounded(dx, gm, f"skip00 + append {case} [{_tag(setting)}]")
            a = ec.bwd_acc_sums(acc, c.C)
            for col, want in ((0, s1), (1, s2)):
                rep = ec.mismatches(a[:, col], want, channels_last=False)
                assert not rep, f"skip00 + append {case} [{_tag(setting)}]: acc column {col}\n{rep}"
    print(f"skip00 + append {case}: {len(settings)} settings")


@pytest.mark.parametrize("case", STEMS, ids=str)
def test_stem_dgrad(case):
    """avt_conv_stem_dgrad (fp32 NCHW out, fp32 weights): integer sums, so the fp64 conv2d_input exactly."""
    c = ec.get_case(case)
    fig = c.figures("dx")
    assert fig["max_abs"] + ec.PREFILL < ec.FP32_OUT_MAX
    gx = _nan(c.N, c.C, c.H, c.W, dtype=torch.float32)
    call("avt_conv_stem_dgrad", P(c.dy.to(torch.bfloat16).to(DEV)), P(c.w.contiguous().to(DEV)), P(gx), c.N, c.H, c.W,
         c.C, S())
    torch.cuda.synchronize()
    ec.assert_fp32(gx, c.ref("dx").permute(0, 3, 1, 2).contiguous(), f"stem dgrad {case}", channels_last=False)


# ---------------------------------------------------------------------------------------------------------------------
# wgrad
# ---------------------------------------------------------------------------------------------------------------------
MANY, GATHER, WGRAD_SWEEP, _run_wgrad = ec.MANY, ec.GATHER, ec.WGRAD_SWEEP, ec.run_wgrad


@pytest.mark.parametrize("case", CASES + STEMS, ids=str)
def test_wgrad_every_form(case, record=True):
    """avt_conv2d_wgrad under every tile, halo form, ring depth, gather-table, split policy and slot share, with a full
    and a NULL workspace (the documented fp32-atomic path), past avt_set_wgrad_slab_max's splits (atomics again), the
    in-kernel reduce of avt_conv2d_wgrad_tk and avt_conv2d_wgrad_defer + avt_wgrad_reduce_batch over two slabs: each
    equals the fp64 conv2d_weight + 0.25 exactly."""
    c = ec.get_case(case)
    fig = c.figures("dw")
    o = _ops(case)
    stem = case in STEMS
    want = c.ref("dw") + ec.PREFILL
    ran = 0
    for mode, setting in WGRAD_SWEEP:
        names = {n for n, *_ in setting}
        if ("avt_set_stem_wgrad" in names) != stem and "avt_set_stem_wgrad" in names:
            continue  # the stem knob reaches the stems only
        if stem and (mode in ("pixtab", "tk", "defer", "split4", "atomic") or "avt_set_wgrad_policy" in names):
            continue  # 49 taps have no gather table; the stems keep their own kernel, its slab and its plan
        with Knobs(setting):
            what = f"wgrad {case} {mode} [{_tag(setting)}]"
            dws, info = _run_wgrad(c, o, mode, what)
            if record and (info in ("2 slabs batched",) or (mode == "tk" and not info.startswith("0 "))):
                _PATHS.setdefault(mode, set()).add(case)
            for dw in dws:
                ec.assert_fp32(dw, want, f"{what} ({info}); index (k, r, s, c)", channels_last=False)
        ran += 1
    if record:
        _WGRAD_RAN.add(case)
    print(f"wgrad {case}: {ran} forms, max |dw| {fig['max_abs']:.0f}")


PATH_CASE = (32, 14, 14, 256, 256, 3, 1, 1)  # test_kernels_gpu's FUSED_EXPECTED: split, and within the fused bound


def test_wgrad_paths_are_taken():
    """The wgrad modes above compare results; this pins that their own paths run, so that a planner change cannot turn
    them into the ordinary slab reduce unnoticed: avt_conv2d_wgrad_tk issues tickets (the in-kernel reduce engages),
    avt_conv2d_wgrad_defer leaves two slabs that one avt_wgrad_reduce_batch sums, and the tap-gather kernel reads its
    registered gather table (an all-invalid table changes the result; the real one gives the exact answer)."""
    case = PATH_CASE
    c = ec.get_case(case)
    c.figures("dw")
    o = _ops(case)
    want = c.ref("dw") + ec.PREFILL
    with Knobs([("avt_set_wgrad_fused", 1, -1), ("avt_set_wgrad_slots_pct", 100)]):
        dws, info = _run_wgrad(c, o, "tk", "tk")
        assert not info.startswith("0 "), info
        ec.assert_fp32(dws[0], want, f"wgrad_tk {case} ({info})", channels_last=False)
    with Knobs([("avt_set_wgrad_slots_pct", 100)]):
        dws, info = _run_wgrad(c, o, "defer", "defer")
        assert info == "2 slabs batched", info
        for dw in dws:
            ec.assert_fp32(dw, want, f"wgrad_defer {case} ({info})", channels_last=False)
    g = (c.N, c.H, c.W, c.C, c.C, c.K, c.R, c.R, c.st, c.pad)
    geo = (c.N, c.H, c.W, c.C, c.R, c.R, c.st, c.pad)
    # one block per tile: k ranges far longer than the ring, whose steps past the prologue gather from the table
    with Knobs([GATHER, ("avt_set_wgrad_pixtab", 1), ("avt_set_wgrad_policy", 1, 1)]):
        wsb = int(query("avt_conv2d_wgrad_workspace", *g))
        ws = _nan(max(wsb // 4, 4), dtype=torch.float32)
        tab = torch.full((int(query("avt_wgrad_pixtab_bytes", c.N, c.H, c.W, c.R, c.R, c.st, c.pad)) // 4,), -1,
                         device=DEV, dtype=torch.int32)
        call("avt_wgrad_pixtab_build", P(tab), *geo, S())
        zero = torch.zeros_like(tab)
        outs = []
        try:
            for t in (tab, zero):
                call("avt_wgrad_pixtab_register", P(t), *geo)
                dw = torch.full((c.K, c.R, c.R, c.C), ec.PREFILL, device=DEV)
                call("avt_conv2d_wgrad", P(o["xg"]), P(o["dyg"]), P(dw), *g, P(ws), wsb, S())
                torch.cuda.synchronize()
                outs.append(dw)
        finally:
            call("avt_wgrad_pixtab_register", None, *geo)
    ec.assert_fp32(outs[0], want, f"wgrad with its gather table {case}", channels_last=False)
    assert not torch.equal(outs[1], outs[0]), "the launch did not read its gather table"
    if len(_WGRAD_RAN) == len(CASES + STEMS):  # the whole file ran: the sweep itself reached both paths
        assert _PATHS.get("tk") and _PATHS.get("defer"), _PATHS
