"""Exactly summable conv operands, their fp64 references and an equality comparator (a helper module, like fwdlink.py
and gradcheck.py): the instrument of test_exactconv_cpu.py, test_conv_exact_gpu.py and test_conv3d_exact_gpu.py.

The principle.  bf16 holds the integers up to 256 exactly; an MFMA product of two of them is exact; every fp32 partial
sum of integers stays exact while the sum of the |products| is below 2^24 -- in whatever order tiles, taps, chunks,
rings, split-K partials, slabs or atomics add them; and f2bf is round-to-nearest-even (avt_common.h).  A conv of such
operands therefore has ONE right answer, bf16_rne(the fp64 conv), and every kernel form and every A/B knob must give
it bit for bit: one dropped, duplicated or misplaced term changes an output by at least one unit, and a unit shows.

Draws (seeded): activations in {0, 1}, weights and output gradients in {-1, 0, 1}; for weight gradients x in {0..3}
and dy in {-3..3}; residual / add in {-3..3}, bias in {-4..4}; a weight gradient accumulates into 0.25.

Conditions (asserted by `figures()` before anything is compared -- conditions of the test, not tolerances):
  * sum of |products| per output < 2^24 (so every partial sum any kernel forms is exact), and the per-channel sums
    of |output| over all rows < 2^24 (the BN partials of the epilogues);
  * at most 1 % of a bf16 output's elements have |ref| > 255 (below that the output is the integer itself; above it
    the comparison is still bf16_rne(ref), only coarser);
  * at least 25 % of the (output, in-image term) pairs have a non-zero product;
  * every |fp32 output| + 0.25 < 2^21.

Roundings of the two-operand epilogues, as the kernels define them (conv_epi.h, conv_c64.h): a dgrad's `add` joins the
ROUNDED conv result and the sum is rounded again, in every form -- `rne2()`; a bias joins the fp32 accumulator before
the first rounding and the residual the rounded value, except in the layer-1 (c64) kernel, which rounds once
 -- so a 2-D bias case with a residual must keep |conv + bias| + |residual| <= 256 everywhere, where both
orders are the identity (`figures()["one_rounding_safe"]`)."""
import zlib

import torch
import torch.nn.functional as F

EXACT = float(2 ** 24)
FP32_OUT_MAX = float(2 ** 21)
PREFILL = 0.25


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def _gen(key, salt):
    return torch.Generator().manual_seed(zlib.crc32(repr((key, salt)).encode()))


def ints(shape, lo, hi, key, salt):
    """Uniform integers lo..hi as fp32."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(key, salt)).float()


def acts(shape, p, key, salt):
    """{0, 1}, one with probability p: post-ReLU-like."""
    return (torch.rand(tuple(shape), generator=_gen(key, salt)) < p).float()


def signs(shape, p, key, salt):
    """{-1, 0, 1}: non-zero with probability p, either sign equally likely."""
    g = _gen(key, salt)
    nz = (torch.rand(tuple(shape), generator=g) < p).float()
    return nz * (torch.randint(0, 2, tuple(shape), generator=g).float() * 2 - 1)


def bf16_rne(t):
    """The bf16 value (as fp64) nearest to t, ties to even: integers below 2^24 pass through fp32 unchanged."""
    return t.float().to(torch.bfloat16).double()


def rne2(conv, add):
    """bf16(bf16(conv) + add): a dgrad's `add` joins the rounded result (conv_epi.h epi_store, conv_c64.h ADD 1/2)."""
    return bf16_rne(bf16_rne(conv) + add.double())


def mask_from_bits(bits, shape):
    """avt_bn_apply_mask's layout: bit e of byte j is channel 8j + e."""
    return ((bits.long().reshape(-1, 1) >> torch.arange(8)) & 1).bool().reshape(shape)


class Case:
    """Operands and lazily computed, cached fp64 references of one conv geometry.

    2-D: case = (N, H, W, C, K, R, stride, pad) (square taps) or (N, H, W, C, K, R, S, stride, pad); activations NHWC,
         weights OHWI.
    3-D: case = (N, T, H, W, C, K, stride) (3x3x3, pad 1) or (N, T, H, W, C, K, KT, R, S, stride, pad_t, pad), temporal
         stride 1; activations NTHWC, weights OIDHW.
    A wgrad-only case (exactconv.DOMAIN_WGRAD) carries the weight gradient's channel count in its C slot (the wgrad
    entry points take C % 8 == 0, the others C % 32 == 0); Cw is that count.
    px / pw / pdy: the densities of the draws (per case: the 27 x 512 sums may take sparser weights).
    The draws are seeded by the case tuple as given: the two short forms keep theirs (tests/golden/exactconv_draws.json)."""
    exact = True

    def __init__(self, case, px=0.5, pw=2.0 / 3, pdy=2.0 / 3):
        self.case = tuple(case)
        self.d3 = len(case) in (7, 12)
        if len(case) == 7:
            N, T, H, W, C, K, st = case
            KT = R = S = 3
            pad_t = pad = 1
        elif len(case) == 12:
            N, T, H, W, C, K, KT, R, S, st, pad_t, pad = case
        elif len(case) == 9:
            N, H, W, C, K, R, S, st, pad = case
            T, KT, pad_t = 1, 1, 0
        else:
            N, H, W, C, K, R, st, pad = case
            T, KT, pad_t, S = 1, 1, 0, R
        self.N, self.T, self.H, self.W, self.C, self.K, self.R, self.st, self.pad = N, T, H, W, C, K, R, st, pad
        self.S, self.KT, self.pad_t, self.Cw = S, KT, pad_t, C
        self.To = T + 2 * pad_t - KT + 1
        self.P, self.Q = conv_out(H, R, st, pad), conv_out(W, S, st, pad)
        assert self.To >= 1 and self.P >= 1 and self.Q >= 1, case
        sp_in = (N, T, H, W) if self.d3 else (N, H, W)
        sp_out = (N, self.To, self.P, self.Q) if self.d3 else (N, self.P, self.Q)
        key = self.case
        self.x = acts(sp_in + (C,), px, key, "x")
        self.w = signs((K, C, KT, R, S) if self.d3 else (K, R, S, C), pw, key, "w")
        self.dy = signs(sp_out + (K,), pdy, key, "dy")
        self.add = ints(sp_in + (C,), -3, 3, key, "add")
        self.res = ints(sp_out + (K,), -3, 3, key, "res")
        self.bias = ints((K,), -4, 4, key, "bias")
        self.xg = ints(sp_in + (self.Cw,), 0, 3, key, "xg")
        self.dyg = ints(sp_out + (K,), -3, 3, key, "dyg")
        n_in = self.x.numel()
        self.bits = torch.randint(0, 256, (n_in // 8,), generator=_gen(key, "bits"), dtype=torch.uint8)
        self._ref, self._fig = {}, {}

    # channel-first views (what torch's conv functions take) --------------------------------------------------------
    def _cf(self, t):
        return t.permute(0, 4, 1, 2, 3) if self.d3 else t.permute(0, 3, 1, 2)

    def _cl(self, t):
        return (t.permute(0, 2, 3, 4, 1) if self.d3 else t.permute(0, 2, 3, 1)).contiguous()

    def _w_oi(self, w):
        return w if self.d3 else w.permute(0, 3, 1, 2)

    def _kw(self):
        if self.d3:
            return dict(stride=(1, self.st, self.st), padding=(self.pad_t, self.pad, self.pad))
        return dict(stride=self.st, padding=self.pad)

    def conv(self, x, w, dtype=torch.float64):
        f = F.conv3d if self.d3 else F.conv2d
        return self._cl(f(self._cf(x).to(dtype), self._w_oi(w).to(dtype), **self._kw()))

    def conv_input(self, dy, w, dtype=torch.float64):
        f = torch.nn.grad.conv3d_input if self.d3 else torch.nn.grad.conv2d_input
        shape = tuple(self._cf(self.x).shape)
        return self._cl(f(shape, self._w_oi(w).to(dtype), self._cf(dy).to(dtype), **self._kw()))

    def conv_weight(self, x, dy, dtype=torch.float64):
        """In the weight's own layout (OHWI for 2-D, OIDHW for 3-D)."""
        f = torch.nn.grad.conv3d_weight if self.d3 else torch.nn.grad.conv2d_weight
        shape = tuple(self._w_oi(self.w).shape)
        dw = f(self._cf(x).to(dtype), shape, self._cf(dy).to(dtype), **self._kw())
        return dw if self.d3 else dw.permute(0, 2, 3, 1).contiguous()

    # references --------------------------------------------------------------------------------------------------
    def ref(self, kind, dtype=torch.float64):
        """kind: "y" = conv(x, w), "dx" = conv_input(dy, w), "dw" = conv_weight(xg, dyg); fp64, computed once."""
        k = (kind, dtype)
        if k not in self._ref:
            if kind == "y":
                r = self.conv(self.x, self.w, dtype)
            elif kind == "dx":
                r = self.conv_input(self.dy, self.w, dtype)
            else:
                r = self.conv_weight(self.xg, self.dyg, dtype)
            self._ref[k] = r
        return self._ref[k]

    def _terms_in_image(self):
        """(output, term) pairs whose term lies inside the image (padding contributes no term), per (k, c) pair."""
        one = torch.ones(1, 1, *((self.T, self.H, self.W) if self.d3 else (self.H, self.W)))
        kern = torch.ones(1, 1, *((self.KT, self.R, self.S) if self.d3 else (self.R, self.S)))
        f = F.conv3d if self.d3 else F.conv2d
        return float(f(one, kern, **self._kw()).sum()) * self.N

    def figures(self, kind):
        """Check the module docstring's conditions for this case's `kind` and return the measured figures."""
        if kind in self._fig:
            return self._fig[kind]
        ref = self.ref(kind)
        # the counts are integers below 2^24: an fp32 conv of the 0/1 indicators is exact and fast
        if kind == "y":
            nz = self.conv((self.x != 0).float(), (self.w != 0).float(), torch.float32).double()
            amax = 1.0
        elif kind == "dx":
            nz = self.conv_input((self.dy != 0).float(), (self.w != 0).float(), torch.float32).double()
            amax = 1.0
        else:
            nz = self.conv_weight((self.xg != 0).float(), (self.dyg != 0).float(), torch.float32).double()
            amax = 9.0
        pairs = self._terms_in_image() * (self.Cw if kind == "dw" else self.C) * self.K
        fig = dict(max_abs=float(ref.abs().max()), abs_sum=float(nz.max()) * amax, nonzero=float(nz.sum()) / pairs,
                   above255=float((ref.abs() > 255).double().mean()))
        assert fig["abs_sum"] < EXACT, (self.case, kind, fig)
        assert fig["nonzero"] >= 0.25, (self.case, kind, fig)
        if kind == "dw":
            assert fig["max_abs"] + PREFILL < FP32_OUT_MAX, (self.case, kind, fig)
        else:
            assert fig["above255"] <= 0.01, (self.case, kind, fig)
            ch = ref.shape[-1]
            fig["col_abs_sum"] = float(ref.abs().reshape(-1, ch).sum(0).max())
            assert fig["col_abs_sum"] < EXACT, (self.case, kind, fig)
        if kind == "y":
            fig["one_rounding_safe"] = float((ref + self.bias.double()).abs().max() + self.res.abs().max()) <= 256
        self._fig[kind] = fig
        return fig


class RandnCase(Case):
    """The same geometry with the per-kernel files' kind of draw (ReLU'd normal activations, scaled normal weights,
    normal gradients, all rounded to bf16): NOT exactly summable.  Only test_exactconv_cpu.py uses it, to record what
    the old relative-error criterion makes of each injected fault on the operands it was used with."""
    exact = False

    def __init__(self, case):
        super().__init__(case)
        g = _gen(self.case, "randn")
        bf = lambda t: t.to(torch.bfloat16).float()
        rn = lambda ref: torch.randn(ref.shape, generator=g)
        self.x, self.xg = bf(rn(self.x).relu()), bf(rn(self.xg).relu())
        self.w = bf(rn(self.w) * (2.0 / (self.K * self.w[0].numel() / self.C)) ** 0.5)
        self.dy, self.dyg, self.add = bf(rn(self.dy)), bf(rn(self.dyg)), bf(rn(self.add))


_CASES = {}


def get_case(case, **density):
    """The Case of a geometry, built once per process and left unchanged."""
    k = (tuple(case), tuple(sorted(density.items())))
    if k not in _CASES:
        _CASES[k] = Case(case, **density)
    return _CASES[k]


# ---------------------------------------------------------------------------------------------------------------------
# what the two GPU files share: raw pointers, the stream, knob settings that are always put back
# ---------------------------------------------------------------------------------------------------------------------
KEEP = []  # device temporaries passed to the C ABI stay alive until the test ends (each GPU file clears it per test)


def P(t):
    import ctypes

    if t is None:
        return None
    KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr())


def S():
    import ctypes

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# knob -> the arguments that put it back (the existing tests' restores)
RESTORE = {
    "avt_set_conv_variant": (1,), "avt_set_halo": (1,), "avt_set_halo8": (-1,), "avt_set_halo8_form": (-1,),
    "avt_set_halo8_nst": (-1,), "avt_set_halo_stages": (2, 3), "avt_set_halo_tps2": (-1,), "avt_set_c64": (1,),
    "avt_set_small_tiles": (-2,), "avt_set_stem_kernel": (1,), "avt_set_nt128_config": (-1,),
    "avt_set_nt64_config": (-1,), "avt_set_s2_dgrad_one": (1,), "avt_set_halo_splitk": (0, 0),
    "avt_set_wgrad_tiles": (1,), "avt_set_wgrad_halo": (-1,), "avt_set_wgrad_row3": (-1, -1, -1),
    "avt_set_wgrad_nst": (4, 3), "avt_set_stem_wgrad": (1,), "avt_set_wgrad_pixtab": (-1,),
    "avt_set_wgrad_policy": (0, 4), "avt_set_wgrad_slots_pct": (-1,), "avt_set_wgrad_slab_max": (1 << 30, 16),
    "avt_set_wgrad_fused": (-1, -1), "avt_set_halo3d": (-1,), "avt_set_video_stem_dgrad": (-1,),
}


class Knobs:
    """Set (knob, args...) tuples on entry and put every one back on exit -- also those already set when a later one
    is refused."""

    def __init__(self, setting):
        self.setting = list(setting)

    def __enter__(self):
        from avt_amd._lib import call

        done = []
        try:
            for name, *args in self.setting:
                call(name, *args)
                done.append(name)
        except Exception:
            for name in reversed(done):
                call(name, *RESTORE[name])
            raise

    def __exit__(self, *exc):
        from avt_amd._lib import call

        for name, *_ in reversed(self.setting):
            call(name, *RESTORE[name])


def tag(setting):
    return ",".join(f"{n[8:]}={'/'.join(map(str, a))}" for n, *a in setting) or "default"


# The knob sweeps of the GPU files.  Forward / dgrad: every knob moved alone from its default, the ring / wave-layout
# knobs also on the tile they belong to, and with the halo off every tile config of the tap-gather kernel.
FWD_SWEEP = (
    [[], [("avt_set_conv_variant", 0)], [("avt_set_halo", 0)], [("avt_set_halo", 2)], [("avt_set_halo8", 0)],
     [("avt_set_halo8", 1)], [("avt_set_halo8_form", 1)], [("avt_set_halo8_nst", 3)], [("avt_set_halo8_nst", 4)],
     [("avt_set_halo_tps2", 1)], [("avt_set_c64", 0)], [("avt_set_small_tiles", 0)], [("avt_set_small_tiles", -1)],
     [("avt_set_stem_kernel", 0)]]
    + [[("avt_set_halo_stages", a, b)] for a, b in ((2, 2), (3, 3), (4, 4), (5, 5), (2, 4), (2, 5))]
    + [[("avt_set_halo8", 0), ("avt_set_halo_stages", a, a)] for a in (2, 4, 5)]
    + [[("avt_set_small_tiles", -1), ("avt_set_halo_stages", a, a)] for a in (2, 5)]
    + [[("avt_set_halo", 2), k] for k in (("avt_set_halo8_form", 1), ("avt_set_halo8_nst", 4), ("avt_set_halo_tps2", 1),
                                           ("avt_set_c64", 0))]
    + [[("avt_set_halo", 0), ("avt_set_nt128_config", c)] for c in range(7)]
    + [[("avt_set_halo", 0), ("avt_set_nt64_config", c)] for c in range(9)]
)
BIAS_SWEEP = [[], [("avt_set_halo", 0)], [("avt_set_halo", 2)], [("avt_set_halo8", 0)], [("avt_set_halo8", 1)],
              [("avt_set_c64", 0)], [("avt_set_small_tiles", 0)], [("avt_set_small_tiles", -1)],
              [("avt_set_halo", 0), ("avt_set_small_tiles", -1)], [("avt_set_halo", 2), ("avt_set_c64", 0)]]
DGRAD_SWEEP = FWD_SWEEP + [[("avt_set_s2_dgrad_one", 0)], [("avt_set_s2_dgrad_one", 1)],
                           [("avt_set_s2_dgrad_one", 0), ("avt_set_small_tiles", -1)]]
# Conv3d: avt_set_halo3d 0/1/2, the two-taps-per-barrier knob, and the tile configs the Conv3d planner picks from
# (test_conv3d_tile_configs: nt64 0/1/2, nt128 1/6) on the tap-gather form
SWEEP_3D = ([[], [("avt_set_halo3d", 0)], [("avt_set_halo3d", 1)], [("avt_set_halo3d", 2)], [("avt_set_halo_tps2", 0)],
             [("avt_set_halo_tps2", 1)], [("avt_set_halo3d", 2), ("avt_set_halo_tps2", 1)]]
            + [[("avt_set_halo3d", 0), ("avt_set_nt64_config", v)] for v in (0, 1, 2)]
            + [[("avt_set_halo3d", 0), ("avt_set_nt128_config", v)] for v in (1, 6)])
MANY = ("avt_set_wgrad_policy", 1 << 20, 1)  # more blocks asked for than there are k-tiles: every split one k-tile (or pair)
GATHER = ("avt_set_wgrad_halo", 0)
WGRAD_SWEEP = (
    [("ws", []), ("ws", [("avt_set_wgrad_tiles", 0)]), ("ws", [("avt_set_wgrad_tiles", 1)])]
    + [("ws", [("avt_set_wgrad_halo", h)]) for h in (0, 1, 2, 3)]
    + [("ws", [("avt_set_wgrad_halo", 2), ("avt_set_wgrad_row3", kg, -1, pf)]) for kg in (1, 2, 4) for pf in (0, 1)]
    + [("ws", [GATHER, ("avt_set_wgrad_nst", a, b)]) for a, b in ((4, 3), (6, 4), (8, 5))]
    + [("ws", [("avt_set_stem_wgrad", 0)]), ("ws", [("avt_set_stem_wgrad", 1)])]
    + [("ws", [GATHER, ("avt_set_wgrad_pixtab", 0)]), ("pixtab", [GATHER, ("avt_set_wgrad_pixtab", 1)]),
       ("pixtab", [GATHER, ("avt_set_wgrad_pixtab", 1), MANY])]
    + [("split4", [GATHER, MANY]), ("split4", [GATHER, MANY, ("avt_set_wgrad_tiles", 0)])]
    + [("ws", [("avt_set_wgrad_slots_pct", 65)]), ("ws", [("avt_set_wgrad_slots_pct", 100)])]
    + [("null", []), ("null", [GATHER]), ("null", [GATHER, MANY]), ("null", [("avt_set_stem_wgrad", 0)])]
    + [("atomic", [GATHER, MANY, ("avt_set_wgrad_slab_max", 2, 16)])]
    + [("tk", [("avt_set_wgrad_fused", 1, -1), ("avt_set_wgrad_slots_pct", 100)]),
       ("tk", [GATHER, ("avt_set_wgrad_fused", 1, -1), ("avt_set_wgrad_policy", 0, 2)])]
    + [("defer", [("avt_set_wgrad_slots_pct", 100)]), ("defer", [GATHER, ("avt_set_wgrad_policy", 0, 2)])]
)
FWD_PLAN_INTS, WGRAD_PLAN_INTS = 10, 24


def fwd_plan(c, cp, epi, dgrad=False):
    """avt_conv_fwd_plan (a host query: no device) under the knobs as they stand; a stride-1 dgrad is the forward of dy
    with C and K swapped and pad' = taps - 1 - pad.  The query takes one pad: for R != S it is asked with R's, so the
    tuple is exact for square taps only (the callers that deduplicate settings by it run every setting at R != S)."""
    import ctypes

    from avt_amd._lib import call

    out = (ctypes.c_int * FWD_PLAN_INTS)()
    if dgrad:
        call("avt_conv_fwd_plan", c.N, c.To, c.P, c.Q, c.K, c.C, c.KT, c.R, c.S, 1, c.KT - 1 - c.pad_t, c.R - 1 - c.pad,
             epi, out)
    else:
        call("avt_conv_fwd_plan", c.N, c.T, c.H, c.W, cp, c.K, c.KT, c.R, c.S, c.st, c.pad_t, c.pad, epi, out)
    return tuple(out)


def fwd_plans(c, cp, sweep, epi, dgrad=False):
    """[(plan, setting)] of the settings whose plan tuple differs from every earlier one (host queries only)."""
    seen, out = set(), []
    for setting in sweep:
        with Knobs(setting):
            plan = fwd_plan(c, cp, epi, dgrad)
        if plan not in seen:
            seen.add(plan)
            out.append((plan, setting))
    return out


def wgrad_plan(c, cp, ws_mode):
    """avt_conv_wgrad_plan (a host query) of a 2-D case under the knobs as they stand."""
    import ctypes

    from avt_amd._lib import call

    out = (ctypes.c_int * WGRAD_PLAN_INTS)()
    call("avt_conv_wgrad_plan", c.N, c.H, c.W, cp, c.Cw, c.K, c.R, c.S, c.st, c.pad, ws_mode, out)
    return tuple(out)


def nan_tensor(*shape, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), device="cuda", dtype=dtype)


def run_wgrad(c, o, mode, what):
    """One 2-D wgrad under the knobs as they stand, into dw pre-filled with 0.25; returns ([dw, ...], info) (defer:
    two).  o: the device operands (cp, xg, dyg)."""
    import ctypes

    from avt_amd._lib import SlabReduceDesc, call, query

    cp = o["cp"]
    g = (c.N, c.H, c.W, cp, c.Cw, c.K, c.R, c.S, c.st, c.pad)
    wsb = int(query("avt_conv2d_wgrad_workspace", *g))  # after the knobs: the plan sizes it
    ws = nan_tensor(max(wsb // 4, 4), dtype=torch.float32)    # any contents
    dw = torch.full((c.K, c.R, c.S, c.Cw), PREFILL, device="cuda")
    npix = c.N * c.P * c.Q
    if mode == "split4" and npix >= 8 * 32:
        assert wsb >= 4 * c.K * c.R * c.S * c.Cw * 4, (what, wsb)  # at least 4 splits through the slab
    if mode == "atomic" and npix >= 8 * 32:
        assert wsb == 0, (what, wsb)  # beyond avt_set_wgrad_slab_max's splits the plan has no slab: fp32 atomics
    if mode in ("ws", "split4", "atomic"):
        call("avt_conv2d_wgrad", P(o["xg"]), P(o["dyg"]), P(dw), *g, P(ws), wsb, S())
    elif mode == "null":
        call("avt_conv2d_wgrad", P(o["xg"]), P(o["dyg"]), P(dw), *g, None, 0, S())
    elif mode == "pixtab":
        geo = (c.N, c.H, c.W, cp, c.R, c.S, c.st, c.pad)
        nb = int(query("avt_wgrad_pixtab_bytes", c.N, c.H, c.W, c.R, c.S, c.st, c.pad))
        assert nb > 0, what
        tab = torch.full((nb // 4,), -1, device="cuda", dtype=torch.int32)
        call("avt_wgrad_pixtab_build", P(tab), *geo, S())
        torch.cuda.synchronize()
        try:
            call("avt_wgrad_pixtab_register", P(tab), *geo)
            call("avt_conv2d_wgrad", P(o["xg"]), P(o["dyg"]), P(dw), *g, P(ws), wsb, S())
            torch.cuda.synchronize()
        finally:
            call("avt_wgrad_pixtab_register", None, *geo)
    elif mode == "tk":
        nt = int(query("avt_conv2d_wgrad_tickets", *g))
        tk = torch.zeros(max(nt, 1), device="cuda", dtype=torch.int32)
        call("avt_conv2d_wgrad_tk", P(o["xg"]), P(o["dyg"]), P(dw), *g, P(ws), wsb, P(tk) if nt else None, nt, S())
        torch.cuda.synchronize()
        assert int(tk.abs().sum()) == 0, what + ": tickets not left zero"
        return [dw], f"{nt} tickets"
    else:  # defer: two slabs, one avt_wgrad_reduce_batch launch
        dws, descs = [dw, dw.clone()], []
        for d in dws:
            w2 = nan_tensor(max(wsb // 4, 4), dtype=torch.float32)
            desc = SlabReduceDesc()
            call("avt_conv2d_wgrad_defer", P(o["xg"]), P(o["dyg"]), P(d), *g, P(w2), wsb, ctypes.byref(desc), S())
            if desc.splits > 0:
                descs.append(desc)
        if descs:
            arr = (SlabReduceDesc * len(descs))(*descs)
            call("avt_wgrad_reduce_batch", arr, len(descs), S())
        torch.cuda.synchronize()
        return dws, f"{len(descs)} slabs batched"
    torch.cuda.synchronize()
    return [dw], f"{wsb} slab bytes"


# ---------------------------------------------------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------------------------------------------------
def _edges(idx, shape, channels_last=True):
    """What an index lies on: image borders, clip ends, 32/64/128/256-row tile edges of the flattened row index, and
    8/32/64-channel chunk edges -- so the cause is readable from the log."""
    tags = []
    if channels_last:
        *sp, c = idx
        dims = shape[:-1]
        names = ("n", "t", "h", "w") if len(dims) == 4 else ("n", "h", "w")
        for nm, v, d in zip(names, sp, dims):
            if nm != "n" and v == 0:
                tags.append(f"{nm}=0")
            if nm != "n" and v == d - 1:
                tags.append(f"{nm}=last")
        row = 0
        for v, d in zip(sp, dims):
            row = row * d + v
        for tile in (32, 64, 128, 256):
            if row % tile == 0:
                tags.append(f"row%{tile}=0")
            if row % tile == tile - 1:
                tags.append(f"row%{tile}=last")
        tags.append(f"row={row}")
        for ch in (8, 32, 64):
            if c % ch == 0:
                tags.append(f"c%{ch}=0")
            if c % ch == ch - 1:
                tags.append(f"c%{ch}=last")
    return ",".join(tags)


def mismatches(got, want, ref=None, channels_last=True, limit=8):
    """'' if got == want as values everywhere with no NaN in got (-0 equals +0); else a report: the count and the
    first few indices with the values and the edges they lie on."""
    got = got.detach().cpu().double()
    want = want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = ~(got == want)  # a NaN is unequal to everything
    n = int(bad.sum())
    if n == 0:
        return ""
    lines = [f"{n} of {bad.numel()} elements differ ({int(torch.isnan(got).sum())} NaN); first {min(n, limit)}:"]
    for idx in bad.nonzero()[:limit].tolist():
        t = tuple(idx)
        r = f" ref {ref[t].item():.2f}" if ref is not None else ""
        lines.append(f"  {t}: got {got[t].item()} want {want[t].item()}{r} [{_edges(t, tuple(got.shape), channels_last)}]")
    return "\n".join(lines)


def assert_bf16(got, ref, what=""):
    """A bf16 output (NaN pre-filled by the caller) must equal bf16_rne(ref) everywhere."""
    assert got.dtype == torch.bfloat16, got.dtype
    rep = mismatches(got, bf16_rne(ref), ref)
    assert not rep, f"{what}\n{rep}"


def assert_rounded(got, want, what=""):
    """A bf16 output against values that are already the expected roundings (rne2, masked integers)."""
    assert got.dtype == torch.bfloat16, got.dtype
    rep = mismatches(got, want)
    assert not rep, f"{what}\n{rep}"


def assert_fp32(got, ref, what="", channels_last=True):
    """An fp32 output must equal the fp64 reference exactly."""
    assert got.dtype == torch.float32, got.dtype
    rep = mismatches(got, ref, ref, channels_last)
    assert not rep, f"{what}\n{rep}"


def fwd_acc_sums(acc, K):
    """[K][3] fp64 sums over the slots the header records (include/avt.h: 8 header doubles, then [slot][K][3]); every
    recorded slot must be finite."""
    a = acc.detach().cpu()
    n = int(a[0].item()) + int(a[1].item())
    assert 0 < n and 8 + n * K * 3 <= a.numel(), (n, a.numel())
    slots = a[8:8 + n * K * 3].view(n, K, 3)
    assert torch.isfinite(slots).all(), "a recorded BN slot is not finite"
    return slots.sum(0)


def assert_fwd_acc(acc, ref, what=""):
    """The forward's BN accumulator: column 0 == the reference's column sums exactly (integers, summed in fp64 over the
    slots); M2 to test_conv_fwd_and_bn_partials' rtol 1e-4 (its fp32 mean is not exact)."""
    K = ref.shape[-1]
    rows = ref.reshape(-1, K)
    a = fwd_acc_sums(acc, K)
    rep = mismatches(a[:, 0], rows.sum(0), channels_last=False)
    assert not rep, f"{what}: BN column sums\n{rep}"
    n = rows.shape[0]
    m2 = a[:, 1] + a[:, 2] - a[:, 0] ** 2 / n
    torch.testing.assert_close(m2, ((rows - rows.mean(0)) ** 2).sum(0), rtol=1e-4, atol=0)


def bwd_acc_sums(ws, C):
    """[C][2] fp64 sums of a BN-backward workspace's recorded slots (8 header doubles, C doubles, [slot][C][2])."""
    a = ws.detach().cpu()
    a = a.view(torch.float64) if a.dtype == torch.uint8 else a
    n = int(a[0].item()) + int(a[1].item())
    base = 8 + C
    assert 0 < n and base + n * C * 2 <= a.numel(), (n, a.numel())
    slots = a[base:base + n * C * 2].view(n, C, 2)
    assert torch.isfinite(slots).all(), "a recorded BN-backward slot is not finite"
    return slots.sum(0)


def exact_bn_stats(C, key):
    """[4][C] fp32 (scale, shift, mean, invstd) that keep the dgrad's BN-backward epilogue exact: scale in {+-1/2, +-1,
    +-2}, shift in halves, mean integer, invstd in {1/2, 1, 2}."""
    g = _gen(key, "stats")
    sc = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)] * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
    sh = torch.randint(-4, 5, (C,), generator=g).float() / 2
    mean = torch.randint(-2, 3, (C,), generator=g).float()
    inv = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    return torch.stack([sc, sh, mean, inv]).float()


def dgrad_bn_ref(g, xc, stats, y=None, xc2=None, stats2=None):
    """The fused BN-backward epilogue from the (already rounded) gradient g: g' = g * mask, sum g', sum g' * xhat (and
    the second BN's sum g' * xhat2), fp64; asserts that the fp32 sums the kernel forms are exact."""
    g, xc = g.double(), xc.double()
    sc, sh, mean, inv = (stats[i].double() for i in range(4))
    mask = (y.double() > 0) if y is not None else (xc * sc + sh > 0)
    gm = torch.where(mask, g, torch.zeros_like(g))
    C = g.shape[-1]
    t1 = gm * ((xc - mean) * inv)
    assert float(t1.abs().reshape(-1, C).sum(0).max()) < EXACT
    out = [gm, gm.reshape(-1, C).sum(0), t1.reshape(-1, C).sum(0)]
    if xc2 is not None:
        t2 = gm * ((xc2.double() - stats2[2].double()) * stats2[3].double())
        assert float(t2.abs().reshape(-1, C).sum(0).max()) < EXACT
        out.append(t2.reshape(-1, C).sum(0))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the two GPU files (sized on the CPU by test_exactconv_cpu.py: nobody tunes densities on the GPU box)
# ---------------------------------------------------------------------------------------------------------------------
STRIDED_CASES = [(2, 9, 11, 64, 128, 3, 2, 1), (2, 15, 13, 64, 128, 3, 2, 1), (3, 7, 5, 128, 256, 1, 2, 0)]
C64_CASES = [(3, 56, 56, 64, 64, 3, 1, 1), (2, 65, 75, 64, 64, 3, 1, 1), (1, 7, 95, 64, 64, 3, 1, 1)]
# N, H, W, Cin, K, R, stride, pad (the device tensors carry Cp = 4 channels for Cin = 3, the fourth zero)
STEM_CASES = [(2, 20, 22, 3, 64, 7, 2, 3), (2, 21, 17, 1, 64, 7, 2, 3), (2, 9, 8, 3, 64, 7, 2, 3)]
VIDEO_STEM_SHAPES = [(2, 4, 32, 32), (1, 3, 17, 9)]  # clips, T, H, W of a 3-channel video


def _dedup(cases):
    out = []
    for c in cases:
        if tuple(c) not in out:
            out.append(tuple(c))
    return out


def cases_2d():
    """CONV_CASES and the FUSED_WGRAD_CASES extras of test_kernels_gpu.py, the strided and the c64 shapes."""
    from test_kernels_gpu import CONV_CASES, FUSED_WGRAD_CASES

    return _dedup(list(CONV_CASES) + list(FUSED_WGRAD_CASES) + STRIDED_CASES + C64_CASES)


def cases_3d():
    """CASES of test_r3d_backward_gpu.py: the patch-form switches, the clip ends inside tiles, P*Q in {31, 32, 33} and
    the empty parity classes."""
    from test_r3d_backward_gpu import CASES

    return [tuple(c) for c in CASES]


class VideoStem:
    """The R3D stem Conv3d(3, 64, 7x7x7, stride (1, 2, 2), pad 3) on an integer video: operands, fp64 references and the
    module's conditions (1029 terms per output; the weight gradient from x in {0..3}, dy in {-3..3})."""

    def __init__(self, shape):
        b, T, H, W = shape
        self.shape = tuple(shape)
        self.P, self.Q = conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3)
        key = ("video_stem",) + self.shape
        self.video = acts((b, 3, T, H, W), 0.5, key, "x")          # NCDHW, the video's own layout
        self.w = signs((64, 3, 7, 7, 7), 2.0 / 3, key, "w")       # OIDHW
        self.dy = signs((b, T, self.P, self.Q, 64), 2.0 / 3, key, "dy")
        self.videog = ints((b, 3, T, H, W), 0, 3, key, "xg")
        self.dyg = ints((b, T, self.P, self.Q, 64), -3, 3, key, "dyg")
        kw = dict(stride=(1, 2, 2), padding=3)
        cf = lambda t: t.permute(0, 4, 1, 2, 3)
        self.y = F.conv3d(self.video.double(), self.w.double(), **kw).permute(0, 2, 3, 4, 1).contiguous()
        self.dx = torch.nn.grad.conv3d_input(tuple(self.video.shape), self.w.double(), cf(self.dy).double(), **kw)
        self.dw = torch.nn.grad.conv3d_weight(self.videog.double(), tuple(self.w.shape), cf(self.dyg).double(), **kw)
        nz_y = F.conv3d((self.video != 0).float(), (self.w != 0).float(), **kw)
        nz_dx = torch.nn.grad.conv3d_input(tuple(self.video.shape), (self.w != 0).float(), cf((self.dy != 0).float()), **kw)
        nz_dw = torch.nn.grad.conv3d_weight((self.videog != 0).float(), tuple(self.w.shape), cf((self.dyg != 0).float()), **kw)
        pairs = float(F.conv3d(torch.ones(1, 1, T, H, W), torch.ones(1, 1, 7, 7, 7), **kw).sum()) * b * 3 * 64
        self.fig = {}
        for kind, ref, nz, amax in (("y", self.y, nz_y, 1.0), ("dx", self.dx, nz_dx, 1.0), ("dw", self.dw, nz_dw, 9.0)):
            fig = dict(max_abs=float(ref.abs().max()), abs_sum=float(nz.max()) * amax, nonzero=float(nz.sum()) / pairs,
                       above255=float((ref.abs() > 255).double().mean()))
            assert fig["abs_sum"] < EXACT and fig["nonzero"] >= 0.25, (shape, kind, fig)
            if kind == "y":
                assert fig["above255"] <= 0.01, (shape, kind, fig)
                assert float(ref.abs().reshape(-1, 64).sum(0).max()) < EXACT
            else:  # fp32 outputs
                assert fig["max_abs"] + PREFILL < FP32_OUT_MAX, (shape, kind, fig)
            self.fig[kind] = fig


_STEMS = {}


def get_video_stem(shape):
    if tuple(shape) not in _STEMS:
        _STEMS[tuple(shape)] = VideoStem(shape)
    return _STEMS[tuple(shape)]


# ---------------------------------------------------------------------------------------------------------------------
# The accepted domain of include/avt.h off the ResNet-18 grid (test_conv_domain_cpu.py, test_conv_domain_gpu.py,
# test_conv3d_domain_gpu.py).  The smallest shapes at which each path exists -- N <= 3, H, W <= 13,
# T <= 5 -- with odd and even sizes, M off the multiples of 64, P*Q < 32; the knob sweeps force the big tiles at
# small M.  Sized on the CPU by test_exactconv_cpu.py: every case passes figures()'s conditions at the default densities
# (the shapes are small: 9 x 1024 and 45 x 192 terms stay below the 1 % above-255 cap), so none carries its own.
# ---------------------------------------------------------------------------------------------------------------------
# forward, bias epilogue (at most 9 taps: more is a documented refusal of avt_conv2d_fwd_bias), split-K
# (N, H, W, C, K, R, S, stride, pad)
DOMAIN_2D = [
    (2, 9, 11, 32, 64, 3, 3, 1, 1),      # C % 64 == 32: the k32 fallback; M = 198
    (1, 5, 6, 96, 192, 3, 3, 1, 1),      # P*Q = 30; Ng = 192
    (2, 8, 8, 160, 320, 1, 1, 1, 0),     # M = 128
    (3, 7, 9, 192, 384, 1, 3, 1, 1),     # R != S; pad > (R-1)/2 along h
    (2, 10, 7, 320, 64, 3, 1, 2, 1),     # R != S at stride 2; pad > (S-1)/2 along w
    (2, 12, 13, 96, 64, 2, 2, 2, 0),     # even taps
    (1, 9, 9, 32, 192, 5, 5, 1, 2),      # 25 taps
    (2, 6, 13, 32, 64, 1, 7, 1, 0),
    (1, 11, 12, 32, 64, 7, 7, 2, 3),     # 49 taps at C = 32: the long tap list
    (2, 6, 5, 192, 192, 3, 3, 1, 0),     # pad 0 under 3x3
    (2, 6, 7, 64, 320, 3, 3, 1, 2),      # pad 2 > (R-1)/2
    (3, 13, 13, 192, 128, 3, 3, 1, 1),   # the halo forms on 3 chunks of 64 channels (split-K: 3 | 3)
    (2, 7, 7, 320, 384, 3, 3, 1, 1),     # the halo forms on 5 chunks, 3 column tiles (split-K: 5 | 5)
    (2, 8, 8, 1024, 64, 1, 1, 1, 0),
    (1, 7, 7, 2048, 192, 1, 1, 2, 0),
    (2, 4, 4, 32, 2048, 1, 1, 1, 0),
    (1, 5, 5, 160, 1024, 1, 1, 1, 0),
    (1, 3, 3, 2048, 2048, 1, 1, 1, 0),
    (1, 4, 4, 1024, 1024, 3, 3, 1, 1),   # P*Q = 16: 9 x 1024 terms
    # the Bottleneck trio, each at stride 1 and 2
    (2, 8, 9, 256, 64, 1, 1, 1, 0), (2, 8, 9, 256, 64, 1, 1, 2, 0),
    (2, 8, 9, 64, 64, 3, 3, 1, 1), (2, 8, 9, 64, 64, 3, 3, 2, 1),
    (2, 8, 9, 64, 256, 1, 1, 1, 0), (2, 8, 9, 64, 256, 1, 1, 2, 0),
]
# dgrad: plain, add, in place, mask, the three BN epilogues, _ws.  C % 64 == 0, K % 32 == 0, at most 32 taps
DOMAIN_DGRAD = [
    (2, 9, 11, 64, 32, 3, 3, 1, 1),
    (1, 5, 6, 192, 96, 3, 3, 1, 1),      # P*Q = 30; Ng = 192; IC % 64 == 32
    (2, 8, 7, 320, 160, 1, 1, 1, 0),
    (2, 7, 9, 192, 192, 1, 3, 1, 0),     # R != S at stride 1 (pad < min(R, S): pad 0)
    (2, 8, 9, 64, 160, 2, 3, 1, 1),      # R != S with a pad on both axes
    (2, 10, 7, 64, 96, 3, 2, 2, 1),      # stride 2, R != S: the parity classes' tap counts differ per axis
    (2, 9, 8, 192, 160, 1, 3, 2, 0),     # stride 2, R != S, pad 0: classes without a tap
    (2, 12, 13, 64, 32, 2, 2, 2, 0),
    (1, 6, 6, 1024, 192, 1, 1, 1, 0),
    (2, 4, 4, 64, 2048, 1, 1, 1, 0),
    (2, 9, 10, 64, 32, 5, 5, 2, 2),      # 25 taps at stride 2: parity classes of 9, 6, 6 and 4 taps
    (2, 6, 7, 192, 96, 3, 3, 2, 1),
    (2, 6, 5, 320, 32, 3, 3, 1, 0),      # pad 0 under 3x3
    (3, 13, 13, 128, 192, 3, 3, 1, 1),   # the halo forms of the dgrad (and its split-K) on 3 chunks
]
# wgrad: every form of test_wgrad_every_form.  The tuple's C slot is Cw, the weight gradient's channel count
DOMAIN_WGRAD = [
    (2, 9, 11, 8, 64, 1, 1, 1, 0),       # 8 columns: ncols < 64
    (2, 9, 11, 8, 64, 3, 3, 1, 1),       # 72 columns
    (3, 7, 9, 16, 192, 1, 3, 1, 1),      # 48 columns
    (2, 8, 8, 24, 64, 3, 3, 1, 1),       # 216 columns: % 128 != 0, > 128
    (2, 13, 12, 24, 320, 3, 3, 2, 1),
    (1, 5, 6, 40, 192, 5, 5, 1, 2),      # 1000 columns; P*Q = 30
    (3, 13, 13, 40, 64, 3, 3, 1, 1),     # 507 pixels: splits
    (2, 10, 7, 96, 320, 1, 1, 2, 0),
    (3, 12, 13, 96, 192, 3, 3, 1, 1),    # 468 pixels: splits
    (2, 6, 6, 160, 64, 1, 3, 1, 0),
    (2, 7, 7, 160, 320, 3, 3, 1, 0),
    (2, 9, 8, 192, 192, 3, 3, 1, 1),     # C % 64 == 0: the halo arms' shape test at K = 192
    (1, 4, 5, 192, 64, 5, 5, 2, 2),
]
SPLIT_WGRAD = [(3, 13, 13, 40, 64, 3, 3, 1, 1), (3, 12, 13, 96, 192, 3, 3, 1, 1)]  # >= 2 splits from the workspace size
# (N, T, H, W, C, K, KT, R, S, stride, pad_t, pad): avt_conv3d_fwd / _fwd_bias, and avt_conv3d_wgrad where the padding is
# temporal 'same' (wgrad3d_ok); the dgrad has its own list (C % 64 == 0, K % 32 == 0, square taps at stride 1)
DOMAIN_3D = [
    (2, 3, 6, 5, 32, 64, 3, 3, 3, 1, 1, 1),
    (1, 4, 7, 6, 96, 192, 3, 3, 3, 1, 1, 1),    # 27 x 96 terms; Ng = 192
    (1, 3, 5, 6, 192, 64, 3, 3, 3, 2, 1, 1),
    (1, 3, 6, 7, 192, 64, 3, 3, 3, 1, 1, 1),     # the three-patch halo form on 3 chunks of 64 channels, 256 x 64 tile
    (2, 3, 6, 7, 192, 128, 3, 3, 3, 1, 1, 1),    # ... and its 256 x 128 tile
    (2, 5, 6, 7, 32, 192, 3, 3, 3, 1, 0, 1),    # pad_t 0: T' = 3
    (2, 3, 7, 6, 96, 64, 3, 3, 3, 1, 2, 0),     # pad_t 2 > (KT-1)/2: T' = 5; spatial pad 0
    (2, 4, 8, 7, 96, 64, 1, 3, 3, 1, 0, 1),
    (1, 5, 6, 6, 32, 192, 3, 1, 1, 1, 1, 0),
    (2, 3, 9, 8, 192, 64, 1, 1, 1, 2, 0, 0),
    (2, 4, 6, 7, 96, 192, 2, 2, 2, 1, 0, 0),
    (2, 4, 6, 7, 32, 64, 2, 2, 2, 2, 1, 1),
    (1, 5, 6, 5, 32, 64, 5, 3, 3, 1, 2, 1),     # 45 taps: the long tap list
    (1, 4, 5, 6, 192, 192, 5, 3, 3, 2, 2, 1),   # 45 x 192 terms
    (2, 3, 5, 7, 64, 128, 1, 3, 1, 2, 0, 1),    # R != S (no stride-1 dgrad: square taps only)
]
DOMAIN_3D_DGRAD = [  # C in {64, 192}, K in {32, 96}
    (2, 3, 6, 5, 64, 32, 3, 3, 3, 1, 1, 1),
    (1, 4, 7, 6, 192, 96, 3, 3, 3, 1, 1, 1),
    (1, 3, 5, 6, 192, 32, 3, 3, 3, 2, 1, 1),
    (1, 3, 6, 7, 64, 192, 3, 3, 3, 1, 1, 1),     # the forward form of this dgrad is the three-patch kernel: IC = 192
    (2, 3, 6, 7, 128, 192, 3, 3, 3, 1, 1, 1),    # ... on its 256 x 128 tile
    (2, 5, 6, 7, 64, 96, 3, 3, 3, 1, 0, 1),     # pad_t 0
    (2, 3, 7, 6, 64, 96, 3, 3, 3, 1, 2, 0),     # pad_t 2, spatial pad 0
    (2, 4, 8, 7, 192, 32, 1, 3, 3, 1, 0, 1),
    (1, 5, 6, 6, 64, 96, 3, 1, 1, 1, 1, 0),
    (2, 3, 9, 8, 192, 96, 1, 1, 1, 2, 0, 0),    # three of the four classes without a tap
    (2, 4, 6, 7, 64, 32, 2, 2, 2, 1, 0, 0),
    (2, 4, 6, 7, 64, 96, 2, 2, 2, 2, 1, 1),
    (1, 5, 6, 5, 64, 32, 5, 3, 3, 1, 2, 1),     # 45 taps
    (2, 3, 5, 7, 64, 96, 1, 3, 1, 2, 0, 0),     # R != S at stride 2
]


def wgrad3d_ok(case):
    """avt_conv3d_wgrad's documented domain within DOMAIN_3D: temporal 'same' padding."""
    N, T, H, W, C, K, KT, R, S, st, pad_t, pad = case
    return 2 * pad_t == KT - 1


# One step across each documented edge: (entry point, case, why).  The case tuples are complete geometries (nothing is
# drawn for them: the GPU files pass pre-filled buffers of the right sizes and expect them back untouched).
OUTSIDE = [
    ("avt_conv2d_fwd", (2, 6, 6, 48, 64, 3, 3, 1, 1), "C = 48: a multiple of 8, not of 32"),
    ("avt_conv2d_fwd", (2, 6, 6, 32, 96, 3, 3, 1, 1), "K = 96"),
    ("avt_conv2d_fwd", (2, 6, 6, 32, 32, 3, 3, 1, 1), "K = 32"),
    ("avt_conv2d_fwd", (1, 12, 12, 32, 64, 5, 10, 1, 2), "50 taps"),
    ("avt_conv2d_fwd", (2, 9, 9, 32, 64, 3, 3, 3, 1), "stride 3"),
    ("avt_conv2d_fwd_bias", (2, 6, 6, 48, 64, 3, 3, 1, 1), "C = 48"),
    ("avt_conv2d_fwd_bias", (2, 6, 6, 32, 96, 3, 3, 1, 1), "K = 96"),
    ("avt_conv2d_fwd_bias", (2, 8, 8, 32, 64, 2, 5, 1, 0), "10 taps: the bias epilogue's narrow form ends at 9"),
    ("avt_conv2d_fwd_bias", (2, 6, 6, 32, 64, 3, 3, 1, 1), "an aliasing residual"),
    ("avt_conv2d_dgrad", (2, 6, 6, 32, 64, 3, 3, 1, 1), "C = 32"),
    ("avt_conv2d_dgrad", (2, 6, 6, 64, 48, 3, 3, 1, 1), "K = 48"),
    ("avt_conv2d_dgrad", (2, 6, 6, 64, 32, 3, 3, 1, 3), "pad >= R"),
    ("avt_conv2d_dgrad", (2, 9, 9, 64, 32, 3, 3, 3, 1), "stride 3"),
    ("avt_conv2d_dgrad", (1, 12, 12, 64, 32, 3, 11, 1, 1), "33 taps"),
    ("avt_conv2d_dgrad", (1, 9, 9, 64, 32, 5, 5, 1, 2), "25 taps in one launch: the 2-D argument block holds 9"),
    ("avt_conv2d_dgrad_mask", (2, 6, 6, 64, 32, 3, 3, 1, 1), "add aliasing dx"),
    ("avt_conv2d_wgrad", (2, 6, 6, 12, 64, 3, 3, 1, 1), "C = 12"),
    ("avt_conv2d_wgrad", (2, 6, 6, 16, 96, 3, 3, 1, 1), "K = 96"),
    ("avt_conv2d_wgrad", (2, 9, 9, 16, 64, 3, 3, 3, 1), "stride 3"),
    ("avt_conv3d_fwd", (1, 3, 6, 6, 48, 64, 3, 3, 3, 1, 1, 1), "C = 48"),
    ("avt_conv3d_fwd", (1, 3, 6, 6, 32, 96, 3, 3, 3, 1, 1, 1), "K = 96"),
    ("avt_conv3d_fwd", (1, 5, 12, 6, 32, 64, 5, 10, 1, 1, 2, 0), "50 taps"),
    ("avt_conv3d_fwd", (1, 3, 9, 9, 32, 64, 3, 3, 3, 3, 1, 1), "stride 3"),
    ("avt_conv3d_fwd_bias", (1, 3, 6, 6, 32, 64, 3, 3, 3, 1, 1, 1), "an aliasing residual"),
    ("avt_conv3d_dgrad", (1, 3, 6, 6, 32, 64, 3, 3, 3, 1, 1, 1), "C = 32"),
    ("avt_conv3d_dgrad", (1, 3, 6, 6, 64, 32, 3, 3, 3, 1, 1, 3), "pad >= R"),
    ("avt_conv3d_dgrad", (1, 3, 6, 6, 64, 32, 3, 3, 1, 1, 1, 0), "R != S at stride 1: square spatial taps only"),
    ("avt_conv3d_wgrad", (1, 3, 6, 6, 32, 64, 3, 3, 3, 1, 0, 1), "pad_t 0 under KT 3: not temporal 'same' padding"),
    ("avt_conv3d_wgrad", (1, 3, 6, 6, 24, 64, 3, 3, 3, 1, 1, 1), "C = 24"),
]
