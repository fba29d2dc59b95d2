"""The input layout kernels of csrc/misc.hip -- the first launch of every step -- at their edges:
avt_nchw_to_nhwc_bf16 (nchw_to_nhwc_kernel and the vectorised nchw_to_nhwc4_kernel<4> / <1>), avt_ncthw_to_nhwc_bf16
and avt_nhwc_bf16_to_nchw.

The reference is x.to(torch.bfloat16), permuted, with pad channels of +0, and the comparison is bitwise (int16 views),
the sign of zero included.  Every destination lies inside a larger buffer filled with one bit pattern (0x5A5A for
bf16, a NaN for fp32), at least 256 bytes of it on either side; after a call the guards must still hold the pattern
and the interior must equal a reference that holds none of it, so a skipped element shows as well as a stray one.

  * both sides of every switch of nhwc4_ok: H W a multiple of 4 or not, x and y 16-byte aligned or not, (C, Cp) in
    and outside {(., 4), (1, 1)}; C > Cp is a refusal;
  * the 8192-block x 256-thread grid cap of each form, where the grid-stride loop wraps (inputs and references built
    on the device, to stay quick).  The 2^31-element switch to the generic form needs more than 12 GB and is left out;
  * bf16 round-to-nearest-even ties (even and odd kept mantissa, both signs), overflow to inf, inf, signed zero, NaN
    (its payload is not compared) and values around the smallest bf16 normal, fp32 denormals among them;
  * a destination that is not 8-byte aligned at Cp = 4 (the generic form stores 8 bytes at once) is refused by both
    entry points before any launch."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from avt_amd._lib import call, lib, query  # noqa: E402

DEV = "cuda"
SENTINEL = 0x5A5A      # bits of every bf16 destination element and guard before a call
NAN_BITS = 0x7FC00000  # the same for an fp32 destination
GUARD_BYTES = 256
_KEEP = []  # device temporaries passed to the C-ABI stay alive until the test ends


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _KEEP.clear()


def P(t):
    if t is None:
        return None
    if isinstance(t, Guarded):
        t = t.t
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """n elements (bf16 as int16 bits, or fp32) inside a buffer of the sentinel: GUARD_BYTES of it in front, `skew`
    more elements to move the interior off its alignment, and GUARD_BYTES behind."""

    def __init__(self, n, dtype=torch.bfloat16, skew=0):
        self.idt, self.fill = (torch.int16, SENTINEL) if dtype == torch.bfloat16 else (torch.int32, NAN_BITS)
        size = 2 if dtype == torch.bfloat16 else 4
        self.n, self.lo = n, GUARD_BYTES // size + skew
        self.buf = torch.full((self.lo + n + GUARD_BYTES // size,), self.fill, device=DEV, dtype=self.idt)
        self.t = self.buf[self.lo:self.lo + n].view(dtype)
        assert self.buf.data_ptr() % 16 == 0
        _KEEP.append(self.buf)

    def bits(self):
        return self.buf[self.lo:self.lo + self.n]

    def guards_intact(self):
        return bool((self.buf[:self.lo] == self.fill).all()) and bool((self.buf[self.lo + self.n:] == self.fill).all())

    def untouched(self):
        return self.guards_intact() and bool((self.bits() == self.fill).all())

    def holds(self, ref):
        """guards intact, the interior bit-identical to ref, and ref free of the sentinel (so nothing was skipped)"""
        rb = ref.contiguous().view(self.idt).reshape(-1).to(DEV)
        assert not bool((rb == self.fill).any())
        return self.guards_intact() and torch.equal(self.bits(), rb)


def _skewed(x, floats):
    """a device copy of x that starts `floats` floats past a 16-byte boundary"""
    buf = torch.empty(x.numel() + floats, device=DEV, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    v = buf[floats:].view(x.shape)
    v.copy_(x)
    _KEEP.append(buf)
    return v


def _nhwc_ref(x, Cp):
    """x [N, C, H, W] fp32 (any device) -> [N, H, W, Cp] bf16, pad channels +0"""
    N, C, H, W = x.shape
    ref = torch.zeros(N, H, W, Cp, dtype=torch.bfloat16, device=x.device)
    ref[..., :C] = x.permute(0, 2, 3, 1).to(torch.bfloat16)
    return ref


def _fold_ref(x, Cp):
    """x [N, C, T, H, W] -> 'b c t h w -> (b t) h w c' in bf16, pad channels +0"""
    N, C, T, H, W = x.shape
    ref = torch.zeros(N * T, H, W, Cp, dtype=torch.bfloat16, device=x.device)
    ref[..., :C] = x.permute(0, 2, 3, 4, 1).reshape(N * T, H, W, C).to(torch.bfloat16)
    return ref


def _to_nhwc(x, Cp, x_skew=0, y_skew=0):
    """avt_nchw_to_nhwc_bf16 of x (CPU or device) into a guarded destination; y_skew in bf16 elements"""
    N, C, H, W = x.shape
    xd = _skewed(x, x_skew) if x_skew else x.to(DEV).contiguous()
    y = Guarded(N * H * W * Cp, skew=y_skew)
    assert xd.data_ptr() % 16 == (4 * x_skew) % 16 and y.t.data_ptr() % 16 == (2 * y_skew) % 16
    call("avt_nchw_to_nhwc_bf16", P(xd), P(y), N, C, H, W, Cp, S())
    torch.cuda.synchronize()
    return y


# H x W: 4, 8, 12 pixels take the vectorised form where (C, Cp) and the alignment allow it; 1, 3, 5, 6, 7 never do
SIZES = [(1, 4), (2, 4), (3, 4), (1, 1), (1, 3), (5, 1), (2, 3), (7, 1)]
# x one float off its 16 bytes / y 8 bytes off its 16: both put a vectorisable shape on the generic form, whose own
# 8-byte store at Cp = 4 stays legal
PLACEMENTS = {"aligned": (0, 0), "x+4B": (1, 0), "y+8B": (0, 4)}


@pytest.mark.parametrize("place", list(PLACEMENTS))
@pytest.mark.parametrize("C,Cp", [(3, 4), (1, 4), (4, 4), (1, 1)])
def test_nchw_to_nhwc_switches(C, Cp, place):
    x_skew, y_skew = PLACEMENTS[place]
    g = torch.Generator().manual_seed(8000 + 10 * C + Cp)
    for H, W in SIZES:
        x = torch.randn(3, C, H, W, generator=g)
        y = _to_nhwc(x, Cp, x_skew, y_skew)
        assert y.holds(_nhwc_ref(x, Cp)), (C, Cp, H, W, place)


@pytest.mark.parametrize("C,Cp", [(8, 8), (5, 8), (2, 3)])
def test_nchw_to_nhwc_generic_widths(C, Cp):
    """Cp outside {1, 4}: the generic kernel's per-channel loop, pad lanes +0."""
    g = torch.Generator().manual_seed(8100 + 10 * C + Cp)
    for H, W in SIZES:
        x = torch.randn(3, C, H, W, generator=g)
        y = _to_nhwc(x, Cp)
        assert y.holds(_nhwc_ref(x, Cp)), (C, Cp, H, W)


# ------------------------------------------------------------------------------------------------- grid caps
CAP = 8192 * 256  # threads of a capped grid


def _device_randn(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, device=DEV, generator=g)


@pytest.mark.parametrize("form,N,C,H,W,Cp", [
    ("generic", 3, 1, 699, 1001, 1),   # 2 099 097 pixels, H W odd: one pixel per thread
    ("nhwc4<1>", 1, 1, 2049, 4096, 1),  # 8 392 704 pixels: four per thread
    ("nhwc4<4>", 1, 3, 2049, 4096, 4),
])
def test_nchw_to_nhwc_above_grid_cap(form, N, C, H, W, Cp):
    per_thread = 1 if form == "generic" else 4
    assert (H * W % 4 == 0) == (per_thread == 4) and CAP < N * H * W // per_thread < CAP + CAP // 256
    x = _device_randn((N, C, H, W), 8200 + Cp)
    y = _to_nhwc(x, Cp)
    assert y.holds(_nhwc_ref(x, Cp))


def test_ncthw_to_nhwc_above_grid_cap():
    N, C, T, H, W, Cp = 1, 3, 2, 1025, 1025, 4
    assert CAP < N * T * H * W < CAP + CAP // 256
    x = _device_randn((N, C, T, H, W), 8210)
    y = Guarded(N * T * H * W * Cp)
    call("avt_ncthw_to_nhwc_bf16", P(x), P(y), N, C, T, H, W, Cp, S())
    torch.cuda.synchronize()
    assert y.holds(_fold_ref(x, Cp))


def test_nhwc_to_nchw_above_grid_cap():
    N, C, HW = 2, 8, 131075
    assert CAP < N * C * HW < CAP + CAP // 256
    x = _device_randn((N, HW, C), 8220).to(torch.bfloat16)
    y = Guarded(N * C * HW, dtype=torch.float32)
    call("avt_nhwc_bf16_to_nchw", P(x), P(y), N, C, HW, S())
    torch.cuda.synchronize()
    assert y.holds(x.float().permute(0, 2, 1))


# ---------------------------------------------------------------------------------------------- special values
def _u(bits):
    return bits - (1 << 32) if bits & 0x80000000 else bits


# fp32 bit patterns with the bf16 bits they must become (None: any NaN)
NORMAL_SPECIALS = [
    (0x3F808000, 0x3F80), (0xBF808000, 0xBF80),  # a tie, the kept mantissa even: down
    (0x3F818000, 0x3F82), (0xBF818000, 0xBF82),  # a tie, the kept mantissa odd: up
    (0x3F808001, 0x3F81), (0x3F817FFF, 0x3F81), (0xBF808001, 0xBF81),  # one ulp to either side of a tie
    (0x3FFF8000, 0x4000), (0x3FFFFFFF, 0x4000),  # a carry out of the mantissa
    (0x7F7FFFFF, 0x7F80), (0xFF7FFFFF, 0xFF80), (0x7F7F8000, 0x7F80),  # the largest finite fp32s overflow to inf
    (0x7F7F7FFF, 0x7F7F),  # the largest that stays finite
    (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),  # inf
    (0x00000000, 0x0000), (0x80000000, 0x8000),  # signed zero
    (0x7FC00000, None), (0xFFC00000, None), (0x7F800001, None), (0x7FFFFFFF, None),  # NaN, payload in the low bits too
    (0x00800000, 0x0080), (0x80800000, 0x8080),  # the smallest normal
    (0x00808000, 0x0080), (0x00818000, 0x0082), (0x00808001, 0x0081),  # ties just above it
]
# fp32 denormals: below the smallest bf16 normal, rounding up to it, and down to zero.  The convert instruction of
# gfx950 decides these; it is held to torch's round-to-nearest-even here (DESIGN.md has the measured result).
DENORMAL_SPECIALS = [
    (0x007FFFFF, 0x0080), (0x807FFFFF, 0x8080), (0x007F8000, 0x0080), (0x007F7FFF, 0x007F), (0x007F0000, 0x007F),
    (0x00400000, 0x0040), (0x00010000, 0x0001), (0x00018000, 0x0002), (0x00008000, 0x0000), (0x00008001, 0x0001),
    (0x00000001, 0x0000), (0x80000001, 0x8000), (0x80018000, 0x8002),
]


def _with_specials(shape, seed):
    """randn with every special value written at 8 random places; returns (x, positions by class)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    flat = x.view(-1).view(torch.int32)
    specials = NORMAL_SPECIALS + DENORMAL_SPECIALS
    where = torch.randperm(flat.numel(), generator=g)[:8 * len(specials)].reshape(len(specials), 8)
    for (bits, _), idx in zip(specials, where):
        flat[idx] = _u(bits)
    return x, where


def test_special_value_table_is_torch():
    """The expected bits above are what torch's own fp32 -> bf16 conversion gives (the reference of this file)."""
    for bits, want in NORMAL_SPECIALS + DENORMAL_SPECIALS:
        got = torch.tensor([_u(bits)], dtype=torch.int32).view(torch.float32).to(torch.bfloat16)
        if want is None:
            assert torch.isnan(got).all(), hex(bits)
        else:
            assert got.view(torch.int16).item() & 0xFFFF == want, (hex(bits), hex(got.view(torch.int16).item()))


def _check_specials(y, ref, tag):
    """y (Guarded) against ref [.., Cp] bf16 from torch: guards, then class by class -- NaN stays NaN, everything
    else bitwise, fp32 denormals reported on their own."""
    assert y.guards_intact(), tag
    got = y.bits().cpu()
    rb = ref.contiguous().view(torch.int16).reshape(-1)
    nan = torch.isnan(ref.reshape(-1))
    assert nan.any() and not (rb == SENTINEL).any()
    assert torch.isnan(got.view(torch.bfloat16)[nan]).all(), (tag, "a NaN did not stay NaN")
    bad = (got != rb) & ~nan
    if bad.any():
        i = bad.nonzero().reshape(-1)[:8]
        raise AssertionError((tag, "bf16 bits differ from torch's", [hex(v & 0xFFFF) for v in got[i].tolist()],
                              [hex(v & 0xFFFF) for v in rb[i].tolist()]))


@pytest.mark.parametrize("form,C,H,W,Cp,x_skew", [
    ("nhwc4<4>", 3, 8, 12, 4, 0), ("nhwc4<1>", 1, 16, 24, 1, 0), ("generic Cp=4", 3, 9, 11, 4, 0),
    ("generic Cp=4, x off", 3, 8, 12, 4, 1), ("generic Cp=8", 5, 9, 11, 8, 0), ("generic Cp=1", 1, 9, 33, 1, 0),
])
def test_nchw_to_nhwc_special_values(form, C, H, W, Cp, x_skew):
    x, _ = _with_specials((2, C, H, W), 8300 + Cp + C)
    y = _to_nhwc(x, Cp, x_skew)
    _check_specials(y, _nhwc_ref(x, Cp), form)


def test_denormals_follow_torch():
    """The pinned part: an fp32 denormal converts as in torch (round to nearest even into the bf16 denormals, up to
    the smallest normal, or down to a zero of its sign) -- nothing is flushed.  Every form, each value alone."""
    vals = torch.tensor([_u(b) for b, _ in DENORMAL_SPECIALS], dtype=torch.int32).view(torch.float32)
    want = torch.tensor([w - (1 << 16) if w & 0x8000 else w for _, w in DENORMAL_SPECIALS], dtype=torch.int16)
    n = vals.numel()
    pad = (-n) % 4
    x = torch.cat([vals, torch.zeros(pad)]).reshape(1, 1, 1, n + pad)
    for Cp, x_skew in [(1, 0), (1, 1), (4, 0), (4, 1)]:  # nhwc4<1>, generic, nhwc4<4>, generic
        y = _to_nhwc(x, Cp, x_skew)
        got = y.bits().cpu().reshape(n + pad, Cp)[:n, 0]
        print(f"denormals Cp={Cp} x_skew={x_skew}: " + " ".join(f"{v & 0xFFFF:04x}" for v in got.tolist()))
        assert torch.equal(got, want), (Cp, x_skew)
        assert y.holds(_nhwc_ref(x, Cp))


# -------------------------------------------------------------------------------------- avt_ncthw_to_nhwc_bf16
NCTHW_CASES = [(2, 3, 1, 4, 4, 4), (2, 1, 1, 3, 3, 4), (2, 3, 2, 9, 11, 4), (1, 1, 2, 2, 4, 4), (1, 3, 16, 5, 5, 4),
               (2, 1, 16, 4, 6, 4), (2, 2, 3, 3, 3, 3), (1, 1, 2, 3, 4, 1)]


@pytest.mark.parametrize("N,C,T,H,W,Cp", NCTHW_CASES)
def test_ncthw_to_nhwc(N, C, T, H, W, Cp):
    """T = 1, 2 and 16, C = 1 and 3 at Cp = 4, odd and even H W; special values scattered through the input.  T = 1
    is avt_nchw_to_nhwc_bf16, bit for bit (there on the vectorised form where H W allows it)."""
    if N * C * T * H * W >= 16 * len(NORMAL_SPECIALS + DENORMAL_SPECIALS):
        x, _ = _with_specials((N, C, T, H, W), 8400 + T + C)
    else:
        x = torch.randn(N, C, T, H, W, generator=torch.Generator().manual_seed(8400 + T + C))
    y = Guarded(N * T * H * W * Cp)
    call("avt_ncthw_to_nhwc_bf16", P(x.to(DEV)), P(y), N, C, T, H, W, Cp, S())
    torch.cuda.synchronize()
    ref = _fold_ref(x, Cp)
    if torch.isnan(ref).any():
        _check_specials(y, ref, (N, C, T, H, W, Cp))
    else:
        assert y.holds(ref)
    if T == 1:
        y2 = _to_nhwc(x[:, :, 0], Cp)
        assert y2.guards_intact() and torch.equal(y2.bits(), y.bits())


# ---------------------------------------------------------------------------------------------------- refusals
def _refused(name, needle, args, y):
    rc = getattr(lib(), name)(*args)
    msg = query("avt_last_error").decode(errors="replace")
    torch.cuda.synchronize()
    assert rc != 0, (name, needle)
    assert needle in msg, (name, needle, msg)
    assert y.untouched(), (name, needle)


@pytest.mark.parametrize("skew", [1, 2, 3])
def test_misaligned_destination_refused(skew):
    """y 2, 4 or 6 bytes off an 8-byte boundary at Cp = 4: both entry points refuse before any launch (the generic
    form's 8-byte store would be misaligned), and C > Cp / NULL are refused as before."""
    x = torch.ones(2 * 3 * 8, device=DEV)
    y = Guarded(2 * 8 * 4, skew=skew)
    assert y.t.data_ptr() % 8 == 2 * skew
    _refused("avt_nchw_to_nhwc_bf16", "bad arguments", [P(x), P(y), 2, 5, 2, 4, 4, S()], y)
    _refused("avt_nchw_to_nhwc_bf16", "nchw_to_nhwc_bf16: y must be 8-byte aligned", [P(x), P(y), 2, 3, 2, 4, 4, S()], y)
    _refused("avt_nchw_to_nhwc_bf16", "bad arguments", [None, P(y), 2, 3, 2, 4, 4, S()], y)
    _refused("avt_ncthw_to_nhwc_bf16", "ncthw_to_nhwc_bf16: y must be 8-byte aligned",
             [P(x), P(y), 2, 3, 1, 2, 4, 4, S()], y)
    _refused("avt_ncthw_to_nhwc_bf16", "bad arguments", [P(x), None, 2, 3, 1, 2, 4, 4, S()], y)
    _refused("avt_ncthw_to_nhwc_bf16", "ncthw_to_nhwc_bf16: y must be 8-byte aligned",
             [P(x), P(y), 1, 3, 2, 2, 4, 4, S()], y)
