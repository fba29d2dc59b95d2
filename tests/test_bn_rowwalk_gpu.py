"""The row-walking BatchNorm passes of bn.hip (AVT_BN_EW=1, the default) against the grid-stride kernels they replace
(AVT_BN_EW=0): every output BIT FOR BIT, and the new path within the bounds tests/test_bn_edges_gpu.py applies to the
same entry points (tests/bncheck.py: fp64 restatement, element bound 2^-8 |r| + a T, sum bound 2^-15).

The library reads the knob once, so the two paths run in two fresh child processes (this file as a script, started
with subprocess.run, never exec'd into).  A child runs every case, writes the sha256 of every output's bytes and --
on the new path -- the bncheck verdicts of the cases of at most 2^20 elements (the fp64 restatement of the larger
ones costs seconds on the CPU; they are held bit for bit to the grid-stride kernels, which test_bn_edges_gpu.py pins
at such sizes).  The children run with AVT_BN_EW_BPC=1: the row walk's grid is T = one block per CU (the library's
default is more), which keeps the shape at which EVERY block is busy small.

Launch arithmetic (bn.hip: rw_deal): cv = C/8, rstep = 256/cv rows per block step, rows_per_block =
max(U rstep, ceil(rows/T) rounded up to rstep), U = 4 (2 for the two-target mask apply).  Rows per C:
  1, rstep-1, rstep, rstep+1     one block: tail loop only, threads without a row
  U rstep +- 1, U rstep          exactly one unrolled iteration; one short of it; a second block with a single row
  3 U rstep + 1                  four blocks, the last with one row (255 of its threads have nothing to do)
  T U rstep - 1, +0, +1          every block exactly one unrolled iteration and no tail / the last block one short /
                                 rows_per_block grows to (U + 1) rstep: an unrolled iteration and a tail row
  9 T rstep + 5                  two unrolled iterations and a tail in every block but the last
C = 24 (C/8 = 3 does not divide 256) keeps bn_apply_kernel<false> under both settings; the backward entries refuse it.
Inputs: pre-activations straddle zero; rows of exact +0 and -0 in c, a channel with shift +0 and one with -0 (so
fma(c, scale, shift) is exactly +-0 there); the gradient has both signs and is correlated with xhat (bncheck)."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CS = [64, 128, 256, 512]
FALLBACK_C = 24
U = 4
SMALL = 1 << 20  # elements: the cases the new path is also held to bncheck's bounds on


def rows_of(C, T):
    rstep = 2048 // C
    ur = U * rstep
    return sorted({1, rstep - 1, rstep, rstep + 1, ur - 1, ur, ur + 1, 3 * ur + 1, T * ur - 1, T * ur, T * ur + 1,
                   9 * T * rstep + 5})


# ------------------------------------------------------------------------------------------------------ child
def child(out_path, check):
    sys.path.insert(0, REPO)
    import torch

    import avtubes  # noqa: F401
    import bncheck as bc
    from avt_amd._lib import BnBwdTarget, call, query

    dev = "cuda"
    T = torch.cuda.get_device_properties(0).multi_processor_count
    digests, failures, keep = {}, [], []

    def P(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def S():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def put(key, t):
        digests[key] = hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()

    def verdict(tag, fn):
        try:
            fn()
        except AssertionError as e:
            failures.append(f"{tag}: {e}")

    def stats(c, gamma, beta):
        x = c.float()
        mean = x.mean(0)
        inv = (x.var(0, unbiased=False) + bc.EPS).rsqrt()
        scale = gamma * inv
        shift = beta - mean * scale
        shift[0], shift[1] = 0.0, -0.0
        return torch.stack([scale, shift, mean, inv]).contiguous()

    def run_case(rows, C):
        g = torch.Generator(device=dev).manual_seed(rows * 4099 + C)
        rn = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
        c = (rn(rows, C) * 1.3 - 0.2).bfloat16()
        cd = (rn(rows, C) * 0.9 + 0.1).bfloat16()
        c[::7] = 0.0
        c[3::11] = -0.0
        gamma, beta = 1 + 0.02 * rn(C), 0.1 * rn(C)
        gamma2, beta2 = 1 + 0.02 * rn(C), 0.1 * rn(C)
        st, st2 = stats(c, gamma, beta), stats(cd, gamma2, beta2)
        xh = (c.float() - st[2]) * st[3]
        xh2 = (cd.float() - st2[2]) * st2[3]
        gy = (0.5 * rn(rows, C) + 0.6 * xh + 0.4).bfloat16()
        gy2 = (gy.float() + 0.6 * xh2).bfloat16()
        small = check and rows * C <= SMALL
        cpu = {n: v.cpu() for n, v in dict(c=c, cd=cd, st=st, st2=st2, gy=gy, gy2=gy2, gamma=gamma,
                                           gamma2=gamma2).items()} if small else None
        tag0 = f"({rows}, {C})"
        sent = lambda: torch.full_like(c, 777.0)  # noqa: E731

        # ---- forward
        res_args = {"none": (None, None, None), "plain": (P(cd), None, None), "scaled": (P(cd), P(st2[0]), P(st2[1]))}
        masked = {}
        for res, args in res_args.items():
            if small:
                r, Tb = bc.fwd_ref(cpu["c"], cpu["st"][0], cpu["st"][1], None if res == "none" else cpu["cd"],
                                   cpu["st2"][0] if res == "scaled" else None,
                                   cpu["st2"][1] if res == "scaled" else None)
            outs = {}
            for relu in (0, 1):
                out = sent()
                call("avt_bn_apply", P(c), P(st[0]), P(st[1]), *args, P(out), rows, C, relu, S())
                put(f"{tag0} apply res={res} relu={relu}", out)
                outs[relu] = out
                if small:
                    verdict(f"{tag0} apply res={res} relu={relu}",
                            lambda: bc.check_elements("", out, r.relu() if relu else r, Tb, bc.A_FWD))
            if 256 % (C // 8):
                continue
            out = sent()
            bits = torch.full((rows * C // 8,), 0xA5, device=dev, dtype=torch.uint8)
            call("avt_bn_apply_mask", P(c), P(st[0]), P(st[1]), *args, P(out), P(bits), rows, C, S())
            put(f"{tag0} apply_mask res={res} out", out)
            put(f"{tag0} apply_mask res={res} bits", bits)
            masked[res] = (out, bits)
            if small:
                def same():
                    assert torch.equal(out.view(torch.int16), outs[1].view(torch.int16)), "apply_mask != apply(relu)"
                    b = bits.cpu().view(rows, C // 8, 1).to(torch.int32)
                    m = ((b >> torch.arange(8, dtype=torch.int32)) & 1).bool().reshape(rows, C)
                    assert torch.equal(m, out.cpu() > 0), "mask bits != out > 0"
                verdict(f"{tag0} apply_mask res={res}", same)
        if 256 % (C // 8):
            return
        y = outs_y = sent()
        call("avt_bn_apply", P(c), P(st[0]), P(st[1]), None, None, None, P(y), rows, C, 1, S())

        # ---- backward
        def ws_new():
            return torch.full((int(query("avt_bn_bwd_workspace", rows, C)),), 0xFF, device=dev, dtype=torch.uint8)

        def check_bwd(tag, gyc, mask, x, stc, gm, gc, dgamma, dbeta, ws):
            ref = bc.bwd_eval(gyc, mask, x, stc, gm)
            yard = bc.bwd_eval(gyc, mask, x, stc, gm, torch.float32)
            a, _ = bc.a_bwd(ref, yard)
            verdict(tag + " gc", lambda: bc.check_elements("", gc, ref.gc, ref.T, a))
            verdict(tag + " sums", lambda: bc.check_sums("", dgamma, dbeta, ref, torch.zeros(C), torch.zeros(C)))
            k = ws[64:64 + 8 * C].cpu().view(torch.float32)

            def ks():
                ok, rk = bc.k_ok(k[:C], k[C:], ref, rows)
                assert ok.all(), ("k1/k2", rk)
            verdict(tag + " k", ks)

        for entry, use_y, gm_out in (("relu", False, False), ("y+gmask", True, True), ("y", True, False),
                                     ("nomask+gmask", False, True), ("nomask", False, False)):
            ws, gc, gmask = ws_new(), sent(), sent()
            dgamma, dbeta = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            if entry == "relu":
                call("avt_bn_relu_bwd", P(gy), P(c), P(st[0]), P(st[1]), P(st[2]), P(st[3]), P(gamma), P(dgamma),
                     P(dbeta), P(gc), P(ws), rows, C, S())
            else:
                call("avt_bn_bwd", P(gy), P(y if use_y else None), P(c), P(st[2]), P(st[3]), P(gamma), P(dgamma),
                     P(dbeta), P(gc), P(gmask if gm_out else None), P(ws), rows, C, S())
            tag = f"{tag0} bwd {entry}"
            for n, t in (("gc", gc), ("dgamma", dgamma), ("dbeta", dbeta), ("ws", ws)) + \
                    ((("gmask", gmask),) if gm_out else ()):
                put(f"{tag} {n}", t)
            if small:
                mask = None if entry.startswith("nomask") else outs_y.cpu() > 0
                check_bwd(tag, cpu["gy"], mask, cpu["c"], cpu["st"], cpu["gamma"], gc, dgamma, dbeta, ws)
                if gm_out:
                    def gm_exact():
                        gp = cpu["gy"] if mask is None else torch.where(mask, cpu["gy"],
                                                                        torch.zeros((), dtype=torch.bfloat16))
                        assert torch.equal(gmask.cpu().float(), gp.float()), "gmask_out"
                    verdict(tag + " gmask", gm_exact)

        for two in (False, True):
            out, bits = masked["scaled" if two else "none"]
            gin = gy2 if two else gy
            ts = []
            for xc, s, gm in ((c, st, gamma), (cd, st2, gamma2))[:2 if two else 1]:
                t = BnBwdTarget()
                t.keep = [torch.zeros(C, device=dev), torch.zeros(C, device=dev), sent(), ws_new()]
                t.xc, t.mean, t.invstd, t.gamma = xc.data_ptr(), s[2].data_ptr(), s[3].data_ptr(), gm.data_ptr()
                t.dgamma, t.dbeta, t.gc, t.workspace = [v.data_ptr() for v in t.keep]
                ts.append(t)
            call("avt_bn_bwd_mask", P(gin), P(bits), ctypes.byref(ts[0]), ctypes.byref(ts[1]) if two else None, rows,
                 C, S())
            tag = f"{tag0} bwd_mask{2 if two else 1}"
            for i, t in enumerate(ts):
                for n, v in zip(("dgamma", "dbeta", "gc", "ws"), t.keep):
                    put(f"{tag} bn{i + 1} {n}", v)
            if small:
                mask = out.cpu() > 0
                ins = [("c", "st", "gamma"), ("cd", "st2", "gamma2")]
                for i, t in enumerate(ts):
                    x, s, gm = (cpu[n] for n in ins[i])
                    check_bwd(f"{tag} bn{i + 1}", cpu["gy2" if two else "gy"], mask, x, s, gm, t.keep[2], t.keep[0],
                              t.keep[1], t.keep[3])
        torch.cuda.synchronize()
        keep.clear()

    for C in CS:
        for rows in rows_of(C, T):
            run_case(rows, C)
    for rows in (50, 4099):
        run_case(rows, FALLBACK_C)
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump({"digests": digests, "failures": failures, "T": T}, f)


# ------------------------------------------------------------------------------------------------------ tests
def _run_child(tmp, ew):
    out = os.path.join(tmp, f"ew{ew}.json")
    env = dict(os.environ, AVT_BN_EW=str(ew), AVT_BN_EW_BPC="1")
    flags = ["-s"] if sys.flags.no_user_site else []
    p = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), out, str(ew)], env=env, cwd=HERE,
                       capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, (ew, p.stdout[-2000:], p.stderr[-4000:])
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("bn_rowwalk"))
    return _run_child(tmp, 0), _run_child(tmp, 1)


def _keys(run, C, kind):
    return sorted(k for k in run["digests"] if k.split(")")[0].endswith(f", {C}") and f") {kind}" in k)


@pytest.mark.parametrize("kind", ["apply ", "apply_mask", "bwd relu", "bwd y", "bwd nomask", "bwd_mask1", "bwd_mask2"])
@pytest.mark.parametrize("C", CS + [FALLBACK_C])
def test_rowwalk_bitwise_equals_gridstride(runs, C, kind):
    """Every output of every case -- gc, g', out, the mask bits, dgamma / dbeta after the finalize, and the whole
    workspace (header, k1 / k2, every slot) -- has the same bytes under AVT_BN_EW=0 and AVT_BN_EW=1."""
    old, new = runs
    ko, kn = _keys(old, C, kind), _keys(new, C, kind)
    assert ko == kn
    if C == FALLBACK_C and kind != "apply ":
        assert not ko  # the entries with a mask or a workspace refuse C/8 = 3
        return
    assert len(ko) >= 2 * (2 if C == FALLBACK_C else len(rows_of(C, old["T"])))
    diff = [k for k in ko if old["digests"][k] != new["digests"][k]]
    assert not diff, diff[:10]


def test_rowwalk_within_bounds(runs):
    """The new path's outputs at the cases of at most 2^20 elements are within bncheck's bounds (and the mask bits,
    the masked gradient and apply_mask's output are exact)."""
    _, new = runs
    assert not new["failures"], new["failures"][:10]


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2] == "1")
