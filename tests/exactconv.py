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

    2-D: case = (N, H, W, C, K, R, stride, pad); activations NHWC, weights OHWI.
    3-D: case = (N, T, H, W, C, K, stride) (3x3x3, temporal stride 1, pad 1); activations NTHWC, weights OIDHW.
    px / pw / pdy: the densities of the draws (per case: the 27 x 512 sums may take sparser weights)."""
    exact = True

    def __init__(self, case, px=0.5, pw=2.0 / 3, pdy=2.0 / 3):
        self.case = tuple(case)
        self.d3 = len(case) == 7
        if self.d3:
            N, T, H, W, C, K, st = case
            R, pad = 3, 1
        else:
            N, H, W, C, K, R, st, pad = case
            T = 1
        self.N, self.T, self.H, self.W, self.C, self.K, self.R, self.st, self.pad = N, T, H, W, C, K, R, st, pad
        self.P, self.Q = conv_out(H, R, st, pad), conv_out(W, R, st, pad)
        sp_in = (N, T, H, W) if self.d3 else (N, H, W)
        sp_out = (N, T, self.P, self.Q) if self.d3 else (N, self.P, self.Q)
        key = self.case
        self.x = acts(sp_in + (C,), px, key, "x")
        self.w = signs((K, C, 3, 3, 3) if self.d3 else (K, R, R, C), pw, key, "w")
        self.dy = signs(sp_out + (K,), pdy, key, "dy")
        self.add = ints(sp_in + (C,), -3, 3, key, "add")
        self.res = ints(sp_out + (K,), -3, 3, key, "res")
        self.bias = ints((K,), -4, 4, key, "bias")
        self.xg = ints(sp_in + (C,), 0, 3, key, "xg")
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
            return dict(stride=(1, self.st, self.st), padding=1)
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
        kern = torch.ones(1, 1, *((3, 3, 3) if self.d3 else (self.R, self.R)))
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
        pairs = self._terms_in_image() * self.C * self.K
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
