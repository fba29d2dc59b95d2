"""The BatchNorm kernels of bn.hip at the paths the first-generation tests never run, element by element against the
fp64 references and bounds of tests/bncheck.py (tests/test_bn_bounds_cpu.py shows that those bounds bite).

What each backward case reaches, from the launch arithmetic of bn.hip (rstep = 256 / (C / 8) rows per block step,
rows_per_block = ceil(rows / 512) rounded up to rstep, the four-row unrolled loop runs once rows_per_block >= 4 rstep;
the apply kernels take a second grid-stride trip once rows C / 8 > 4096 * 256 = 1,048,576 vectors):
  (16391, 512)  rstep 4, rows_per_block 36: two unrolled iterations + one tail row per thread, 456 blocks with a
                partial last one (11 rows); 1,049,024 vectors: second grid-stride trip of the apply kernels
  (66001, 64)   rstep 32, rows_per_block 160 = 5 rstep: one unrolled iteration + a tail; last block 81 rows
  (12301, 256)  rstep 8, rows_per_block 32: exactly one unrolled iteration, no tail; last block 13 rows
  (1601, 2048)  rstep 1, rows_per_block 4: unrolled, the C <= 2048 limit, all of red[2048 * NS]; last block 1 row
  (777, 8)      rstep 256, rows_per_block 256: tail loop, the last block's threads 9 .. 255 have no rows
  (1, 64)       a single row (xhat = 0, gc = 0)
  (198, 64)     an old shape under the new bound
Longest fp32 chain: 9 rows per thread + 256 partials, under the 272 of bncheck's sum bound.
Forward only: (43701, 192) is bn_apply_kernel<false> (C / 8 = 24, no power of two) with 1,048,824 vectors -- a second
trip whose stride 1,048,576 is no multiple of 24 -- and (50, 24) the same kernel at C / 8 = 3.

Every workspace and accumulator is 0xFF- or NaN-filled, every output holds a sentinel before the call."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bncheck as bc

pytestmark = pytest.mark.gpu

from avt_amd._lib import BnBwdTarget, call, query  # noqa: E402

DEV = "cuda"
_KEEP = []


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _KEEP.clear()


def P(t):
    if t is None:
        return None
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr())


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def D(t):
    d = t.to(DEV)
    _KEEP.append(d)
    return d


BWD_CASES = [(16391, 512), (66001, 64), (12301, 256), (1601, 2048), (777, 8), (1, 64), (198, 64)]
TWICE = {(16391, 512), (66001, 64)}  # run from two differently filled workspaces: bitwise equal
FWD_CASES = BWD_CASES + [(43701, 192), (50, 24)]
SENTINEL = 777.0


@functools.lru_cache(maxsize=None)
def case(rows, C):
    return bc.make_case(rows, C)


def ws_filled(rows, C, byte):
    return torch.full((int(query("avt_bn_bwd_workspace", rows, C)),), byte, device=DEV, dtype=torch.uint8)


def ws_k(ws, C):
    """The fp32 k1, k2 a backward entry leaves behind the workspace's 8-double header (avt_common.h)."""
    k = ws[64:64 + 8 * C].cpu().view(torch.float32)
    return k[:C], k[C:]


def unpack_bits(bits, rows, C):
    """[rows][C] bool from the [rows][C/8] mask bytes (bit e of a byte: channel 8 * block + e)."""
    b = bits.cpu().view(rows, C // 8, 1).to(torch.int32)
    return ((b >> torch.arange(8, dtype=torch.int32)) & 1).bool().reshape(rows, C)


def sentinel_like(t):
    return torch.full_like(t, SENTINEL)


def check_target(tag, k, gy, mask, x, st, gamma, gc, dgamma, dbeta, start, ws):
    """gc element-wise, dgamma / dbeta (added to `start`) by the sum bound, the workspace's k1 / k2."""
    ref = bc.bwd_eval(gy, mask, x, st, gamma)
    yard = bc.bwd_eval(gy, mask, x, st, gamma, torch.float32)
    bc.assert_visible(ref, k.rows, tag)
    a, a_yard = bc.a_bwd(ref, yard)
    print(f"{tag}: a_yard {a_yard:.2e}")
    bc.check_elements(tag + " gc", gc, ref.gc, ref.T, a)
    if dgamma is not None:
        bc.check_sums(tag, dgamma, dbeta, ref, start[0], start[1])
    okk, rk = bc.k_ok(*ws_k(ws, k.C), ref, k.rows)
    print(f"{tag}: worst (k1, k2) error / bound {rk:.3f}")
    assert okk.all(), (tag, rk)


def starts(C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C, generator=g), torch.randn(C, generator=g)


def run_plain(entry, k, dev, byte):
    """avt_bn_bwd with y ("y"), without ("nomask"), or avt_bn_relu_bwd ("relu") -> the outputs as a dict."""
    rows, C = k.rows, k.C
    ws = ws_filled(rows, C, byte)
    sg, sb = starts(C, 3)
    dgamma, dbeta = D(sg), D(sb)
    gc, gmask = sentinel_like(dev["c"]), sentinel_like(dev["c"])
    st = dev["st"]
    if entry == "relu":
        call("avt_bn_relu_bwd", P(dev["gy"]), P(dev["c"]), P(st[0]), P(st[1]), P(st[2]), P(st[3]), P(dev["gamma"]),
             P(dgamma), P(dbeta), P(gc), P(ws), rows, C, S())
    else:
        call("avt_bn_bwd", P(dev["gy"]), P(dev["y"] if entry == "y" else None), P(dev["c"]), P(st[2]), P(st[3]),
             P(dev["gamma"]), P(dgamma), P(dbeta), P(gc), P(gmask), P(ws), rows, C, S())
    torch.cuda.synchronize()
    return {"gc": gc, "gmask": gmask, "dgamma": dgamma, "dbeta": dbeta, "ws": ws, "start": (sg, sb)}


def run_mask(two, k, dev, byte, null_sums=False):
    rows, C = k.rows, k.C

    def target(xc, s, gamma, seed):
        t = BnBwdTarget()
        sg, sb = starts(C, seed)
        t.start = (sg, sb)
        t.keep = [D(sg), D(sb), sentinel_like(xc), ws_filled(rows, C, byte)]
        t.xc, t.mean, t.invstd, t.gamma = xc.data_ptr(), s[2].data_ptr(), s[3].data_ptr(), gamma.data_ptr()
        t.dgamma, t.dbeta, t.gc, t.workspace = [x.data_ptr() for x in t.keep]
        if null_sums:
            t.dgamma = t.dbeta = None
        return t

    t1 = target(dev["c"], dev["st"], dev["gamma"], 4)
    t2 = target(dev["cd"], dev["st2"], dev["gamma2"], 5) if two else None
    call("avt_bn_bwd_mask", P(dev["gy2"] if two else dev["gy"]), P(dev["bits2"] if two else dev["bits1"]),
         ctypes.byref(t1), ctypes.byref(t2) if two else None, rows, C, S())
    torch.cuda.synchronize()
    return [t1, t2] if two else [t1]


@functools.lru_cache(maxsize=2)
def device_case(rows, C):
    """The case on the GPU with the forward outputs the backward entries take their masks from."""
    k = case(rows, C)
    dev = {n: getattr(k, n).to(DEV) for n in ("c", "cd", "gy", "gy2", "st", "st2", "gamma", "gamma2")}
    st, st2 = dev["st"], dev["st2"]
    dev["y"] = sentinel_like(dev["c"])
    call("avt_bn_apply", P(dev["c"]), P(st[0]), P(st[1]), None, None, None, P(dev["y"]), rows, C, 1, S())
    for name, res in (("1", (None, None)), ("2", (P(st2[0]), P(st2[1])))):
        out = sentinel_like(dev["c"])
        bits = torch.full((rows * C // 8,), 0xA5, device=DEV, dtype=torch.uint8)
        call("avt_bn_apply_mask", P(dev["c"]), P(st[0]), P(st[1]), P(dev["cd"]), *res, P(out), P(bits), rows, C, S())
        dev["out" + name], dev["bits" + name] = out, bits
    torch.cuda.synchronize()
    return dev


ENTRIES = ["y", "nomask", "relu", "mask1", "mask2"]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                       b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("rows,C", BWD_CASES)
def test_bn_backward_edges(rows, C, entry):
    k, dev = case(rows, C), device_case(rows, C)
    tag = f"({rows}, {C}) {entry}"
    if entry in ("y", "nomask", "relu"):
        o = run_plain(entry, k, dev, 0xFF)
        mask = None if entry == "nomask" else dev["y"].cpu() > 0
        check_target(tag, k, k.gy, mask, k.c, k.st, k.gamma, o["gc"], o["dgamma"], o["dbeta"], o["start"], o["ws"])
        if entry != "relu":  # g' as the kernel masked it, exactly
            gp = k.gy if mask is None else torch.where(mask, k.gy, torch.zeros((), dtype=torch.bfloat16))
            assert torch.equal(o["gmask"].cpu().float(), gp.float())
        if (rows, C) in TWICE:
            o2 = run_plain(entry, k, dev, 0x7F)
            for n in ("gc", "dgamma", "dbeta") + (("gmask",) if entry != "relu" else ()):
                assert _same_bits(o[n], o2[n]), (tag, n)
        return
    two = entry == "mask2"
    bits = dev["bits2" if two else "bits1"]
    mask = unpack_bits(bits, rows, C)
    assert torch.equal(mask, dev["out2" if two else "out1"].cpu() > 0)
    ts = run_mask(two, k, dev, 0xFF)
    gy = k.gy2 if two else k.gy
    ins = [(k.c, k.st, k.gamma)] + ([(k.cd, k.st2, k.gamma2)] if two else [])
    for i, (t, (x, st, gamma)) in enumerate(zip(ts, ins)):
        check_target(f"{tag} bn{i + 1}", k, gy, mask, x, st, gamma, t.keep[2], t.keep[0], t.keep[1], t.start,
                     t.keep[3])
    if (rows, C) in TWICE:
        for t, u in zip(ts, run_mask(two, k, dev, 0x7F)):
            for j in range(3):
                assert _same_bits(t.keep[j], u.keep[j]), (tag, j)
    if (rows, C) == (198, 64):  # NULL dgamma / dbeta: gc as before, bit for bit
        for t, u in zip(ts, run_mask(two, k, dev, 0xFF, null_sums=True)):
            assert _same_bits(t.keep[2], u.keep[2])
            assert torch.equal(u.keep[0].cpu(), u.start[0]) and torch.equal(u.keep[1].cpu(), u.start[1])


RES = ["none", "plain", "scaled"]


@pytest.mark.parametrize("res", RES)
@pytest.mark.parametrize("rows,C", FWD_CASES)
def test_bn_apply_edges(rows, C, res):
    """avt_bn_apply (relu 0 / 1) and avt_bn_apply_mask, with no residual, a plain one and a scaled one."""
    k = case(rows, C)
    st, st2 = D(k.st), D(k.st2)
    cdev, cddev = D(k.c), D(k.cd)
    args = {"none": (None, None, None), "plain": (P(cddev), None, None), "scaled": (P(cddev), P(st2[0]), P(st2[1]))}[res]
    r, T = bc.fwd_ref(k.c, k.st[0], k.st[1], None if res == "none" else k.cd,
                      k.st2[0] if res == "scaled" else None, k.st2[1] if res == "scaled" else None)
    tag = f"({rows}, {C}) res={res}"
    outs = {}
    for relu in (0, 1):
        out = sentinel_like(cdev)
        call("avt_bn_apply", P(cdev), P(st[0]), P(st[1]), *args, P(out), rows, C, relu, S())
        torch.cuda.synchronize()
        bc.check_elements(f"{tag} relu={relu}", out, r.relu() if relu else r, T, bc.A_FWD)
        outs[relu] = out
    out = sentinel_like(cdev)
    bits = torch.full((rows * C // 8,), 0xA5, device=DEV, dtype=torch.uint8)
    if 256 % (C // 8):
        with pytest.raises(RuntimeError):
            call("avt_bn_apply_mask", P(cdev), P(st[0]), P(st[1]), *args, P(out), P(bits), rows, C, S())
        return
    call("avt_bn_apply_mask", P(cdev), P(st[0]), P(st[1]), *args, P(out), P(bits), rows, C, S())
    torch.cuda.synchronize()
    assert _same_bits(out, outs[1])
    assert torch.equal(unpack_bits(bits, rows, C), out.cpu() > 0)


# ------------------------------------------------------------------------------------------ finalize
def ragged_acc(x, C):
    """The accumulator a conv epilogue with 64-row tiles leaves for the rows x [rows][C] (fp64): per tile t its own
    slot (sum_t, M2_t, sum_t^2 / n_t), the last tile short; the slot count split over header[0] and header[1] (the
    finalize reads their sum); everything else NaN."""
    rows = x.shape[0]
    nf = rows // 64
    parts = []
    if nf:
        blk = x[:nf * 64].view(nf, 64, C)
        s = blk.sum(1)
        parts.append(torch.stack([s, ((blk - blk.mean(1, keepdim=True)) ** 2).sum(1), s * s / 64], dim=2))
    if rows % 64:
        blk = x[nf * 64:]
        s = blk.sum(0)
        parts.append(torch.stack([s, ((blk - blk.mean(0)) ** 2).sum(0), s * s / blk.shape[0]], dim=1)[None])
    slots = torch.cat(parts)
    n = slots.shape[0]
    acc = torch.full((int(query("avt_bn_acc_doubles", rows, C)),), float("nan"), dtype=torch.float64)
    acc[0], acc[1] = n // 2, n - n // 2
    acc[8:8 + n * C * 3] = slots.reshape(-1)
    return acc, n


def fin_rows(C, rows, data, seed):
    g = torch.Generator().manual_seed(seed)
    if data == "randn":
        x = torch.randn(rows, C, generator=g) * 1.3 + 0.4
    elif data == "const":  # channel 1 constant: M2 clamps to 0, invstd = rsqrt(eps)
        x = torch.randn(rows, C, generator=g) * 1.3 + 0.4
        x[:, 1] = 2.5
    elif data == "offset":  # large mean, tiny variance (in bf16, whose spacing at 300 is 2: mostly exactly 300)
        x = 300 + 0.05 * torch.randn(rows, C, generator=g)
    else:  # "offset2": large mean, a variance that survives the bf16 rounding
        x = 300 + 3 * torch.randn(rows, C, generator=g)
    return x.to(torch.bfloat16).double()


# (C, rows, data, rep): slot counts 1 (50 rows, 1 row), 17 (1061 rows), 1025 (65541 rows) -- one past a single
# eight-load batch of slot_sums (8 * 16 waves * SPI slots per batch: 1024 at C >= 4)
FIN_CASES = [
    (6, 50, "randn", 1), (6, 1061, "const", 3), (6, 65541, "offset", 16), (6, 65541, "randn", 3),
    (64, 50, "offset", 16), (64, 1061, "randn", 1), (64, 65541, "const", 3), (64, 65541, "offset2", 1),
    (2048, 50, "const", 1), (2048, 50, "randn", 16), (2048, 1061, "offset", 3), (2048, 1061, "offset2", 1),
    (6, 1, "randn", 1), (64, 1, "randn", 3), (64, 1, "offset", 1), (2048, 1, "const", 16),
]


@pytest.mark.parametrize("C,rows,data,rep", FIN_CASES)
def test_bn_finalize_rep_edges(C, rows, data, rep):
    x = fin_rows(C, rows, data, 40 + rep)
    acc, n = ragged_acc(x, C)
    assert n == (rows + 63) // 64
    g = torch.Generator().manual_seed(41)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    rm0, rv0 = 0.5 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    mom, eps = 0.3, 1e-5

    def run(which):
        stats = torch.full((4, C), SENTINEL, device=DEV)
        rm, rv, a = D(rm0), D(rv0), D(acc)
        tail = [P(D(gamma)), P(D(beta)), P(rm), P(rv), ctypes.c_float(mom), ctypes.c_float(eps), P(stats[0]),
                P(stats[1]), P(stats[2]), P(stats[3]), S()]
        if which is None:
            call("avt_bn_finalize", P(a), rows, C, *tail)
        else:
            call("avt_bn_finalize_rep", P(a), rows, which, C, *tail)
        torch.cuda.synchronize()
        return stats.cpu(), rm.cpu(), rv.cpu()

    plain, one, got = run(None), run(1), run(rep)
    for a, b in zip(plain, one):  # avt_bn_finalize is avt_bn_finalize_rep(rep = 1), bit for bit
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # reference: fp64 BatchNorm over the logical batch in which every row occurs rep times
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    inv = (var + eps).rsqrt()
    if rows * rep > 1:
        rm64, rv64 = rm0.double(), rv0.double()
        F.batch_norm(x.repeat_interleave(rep, 0), rm64, rv64, gamma.double(), beta.double(), True, mom, eps)
    else:  # one value per channel, which torch refuses: the formulas, the kernel keeping the biased variance (0)
        rm64, rv64 = (1 - mom) * rm0.double() + mom * mean, (1 - mom) * rv0.double() + mom * var
    stats, rm, rv = got
    atol = bc_ulp32(x.abs().max(0).values)
    for name, have, want in (("mean", stats[2], mean), ("invstd", stats[3], inv), ("scale", stats[0], gamma.double() * inv),
                             ("running_mean", rm, rm64), ("running_var", rv, rv64)):
        err = (have.double() - want).abs()
        bound = 1e-6 * want.abs() + atol
        assert (err <= bound).all(), (name, (err / bound).max().item())
    # shift = beta - mean scale, in fp32 from the kernel's own mean and scale: two roundings
    sh = beta.double() - stats[2].double() * stats[0].double()
    assert ((stats[1].double() - sh).abs() <= 2.0 ** -23 * (beta.double().abs() + (stats[2].double() * stats[0].double()).abs())).all()
    if data == "const":
        assert stats[3][1].item() == pytest.approx(float(np.float32(1) / np.sqrt(np.float32(eps))), rel=1e-6)


def bc_ulp32(x):
    """One fp32 ulp at |x| (fp64 tensor in, fp64 out)."""
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()
