"""Element-wise Adam checks shared by the GPU tests: the fp64 reference (oracle AdamRef), its fp32 yardstick
(torch.optim.Adam on the CPU, foreach=False) and the unit the errors are counted in.

Hyper-parameters: the kernels take them as fp32 (a device tensor, or C floats), so the reference and the yardstick
get those same fp32 values, widened -- as every parity test here feeds its reference the kernel's rounded inputs.
(1 - fp32(0.999) differs from 0.001 by 1.3e-5: against beta2 = 0.999 in double, exp_avg_sq would be off by that
much for a correct kernel.)

Unit of error: one fp32 ulp of the value, where "the value" of an element is the largest of the terms that form it
-- exp_avg = b1 m + (1 - b1) g with a fresh random g may cancel (so may g + wd p, which feeds both moments), and no
fp32 arithmetic holds an ulp of the difference.  An error made that way stays in the element: the unit of a moment
at step t is at least beta times its unit at step t - 1, and the unit of p grows by what one unit of each moment
moves the update (first-order propagation; it matters only for the p that start at 0 and consist of updates).

The yardstick E is the LARGEST error of the fp32 CPU Adam over all elements, in these units; every element of the
kernel's result must lie within max(3 E, 1) units of the fp64 reference.  (A bound taken element by element from
the CPU's error at that same element is zero wherever the CPU happens to round the right way; the rounding error
of one element over several steps is a random walk, and only the population's maximum estimates what the
arithmetic can do.  For the same reason a case of a handful of elements measures E on a few thousand elements
drawn the same way, of which the kernel's are the first.)"""
import math

import numpy as np
import torch

HYPER = (1e-6, 0.9, 0.999, 1e-8, 1e-4)  # the reference's lr, beta1, beta2, eps, weight decay


def f32(x):
    """x rounded to fp32, as a Python float."""
    return float(np.float32(x))


def ulp32(x):
    """Spacing of the fp32 numbers at |x| (x: an fp64 tensor), as fp64."""
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


class AdamPair:
    """The fp64 AdamRef and the fp32 CPU torch.optim.Adam, stepped together from the same fp32 start."""

    def __init__(self, p0, hyper=HYPER):
        import avenet_oracle as orc

        lr, b1, b2, eps, wd = (f32(h) for h in hyper)
        self.ref = orc.AdamRef(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
        self.pr = {"p": p0.double().clone()}
        self.q = torch.nn.Parameter(p0.clone())
        self.opt = torch.optim.Adam([self.q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
        self.unit = None  # the previous step's units

    def set(self, lr=None, wd=None):
        if lr is not None:
            self.ref.lr = self.opt.param_groups[0]["lr"] = f32(lr)
        if wd is not None:
            self.ref.wd = self.opt.param_groups[0]["weight_decay"] = f32(wd)

    def step(self, g):
        """One step of both on the fp32 gradient g; returns (ref, yard, unit), dicts over "p", "m", "v"."""
        p_prev = self.pr["p"].clone()
        m_prev, _ = self.ref.state.get("p", (torch.zeros_like(p_prev), None))
        self.ref.step(self.pr, {"p": g.double()})
        self.q.grad = g.clone()
        self.opt.step()
        m, v = self.ref.state["p"]
        st = self.opt.state[self.q]
        # the decayed gradient g + wd p is itself a sum whose terms may cancel: `a` is its larger term
        wd, b1, b2, t = self.ref.wd, self.ref.b1, self.ref.b2, self.ref.t
        a = torch.maximum(g.double().abs(), wd * p_prev.abs())
        geff = (g.double() + wd * p_prev).abs()
        um = ulp32(torch.maximum(torch.maximum(m_prev.abs(), (1 - b1) * a), m.abs()))
        uv = ulp32(torch.maximum(v, 2 * (1 - b2) * a * geff))
        up = ulp32(torch.maximum(p_prev.abs(), self.pr["p"].abs()))
        if self.unit is not None:
            um = torch.maximum(um, b1 * self.unit["m"])
            uv = torch.maximum(uv, b2 * self.unit["v"])
            up = torch.maximum(up, self.unit["p"])
        # d(update) for one unit of m and of v: update = step_size m / denom, denom = sqrt(v) / bc2_sqrt + eps
        step_size, bc2_sqrt = self.ref.lr / (1 - b1 ** t), math.sqrt(1 - b2 ** t)
        denom = v.sqrt() / bc2_sqrt + self.ref.eps
        ddenom = uv / (2 * v.sqrt().clamp_min(1e-300) * bc2_sqrt)
        up = up + step_size * (um + m.abs() * ddenom / denom) / denom
        self.unit = unit = {"p": up, "m": um, "v": uv}
        ref = {"p": self.pr["p"], "m": m, "v": v}
        yard = {"p": self.q.detach(), "m": st["exp_avg"], "v": st["exp_avg_sq"]}
        return ref, yard, unit


def check_elementwise(tag, got, ref, yard, unit, n=None):
    """got (dict of GPU tensors over the first n elements) against ref, bounded per element by max(3 E, 1) units,
    E the yardstick's largest error in units over the whole population.  Returns {name: (kernel max, E)}."""
    out, bad = {}, []
    for k in ("p", "m", "v"):
        n_k = ref[k].numel() if n is None else n
        E = ((yard[k].double() - ref[k]).abs() / unit[k]).max().item()
        err = (got[k].cpu().double() - ref[k][:n_k]).abs() / unit[k][:n_k]
        K = err.max().item()
        factor = max(3 * E, 1.0)
        out[k] = (K, E)
        print(f"{tag} {k}: kernel max {K:.2f} ulp  fp32 CPU Adam max {E:.2f} ulp  bound {factor:.2f} ulp")
        if not (err <= factor).all():
            bad.append((k, K, factor, int((~(err <= factor)).sum())))
    assert not bad, (tag, bad)
    return out
