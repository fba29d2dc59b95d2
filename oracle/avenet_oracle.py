"""CPU restatement of the reference hard-way train step — TEST INFRASTRUCTURE ONLY.

This module is the *oracle*: a plain PyTorch-CPU (fp32/fp64) restatement of
the reference's 1-frame audio-visual hard-way step.  Only ``tests/``,
``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may import
it, and only as the checker / the timed host baseline.  The product path
(``audio-visual-tubes_amd/``) never imports it.

Parity pin: the restatement is checked against golden vectors produced by the
reference itself (``oracle/gen_golden.py`` imports ``/root/reference/model.py``
in the survey container and writes ``tests/golden/*.npz``); see
``tests/test_oracle_golden.py``.

What it restates (reference file:line):
  * ResNet-18 with modal-selected stem, layer4 stride 1 — models/base_models.py:113-169,
    _forward_impl 195-210, BasicBlock.forward 53-69, conv3x3/conv1x1 23-30.
  * AVENet.__init__ re-init (kaiming fan_out, BN ~ N(1, 0.02)) — model.py:104-110.
  * AVENet.forward: normalise, A / A0 einsums, sigmoid trimap, sim1/sim/sim2,
    logits/0.07, weighted_A — model.py:112-154.
  * HardWayAttention.forward (the 3-D tube head) — model.py:46-60.
  * CrossEntropy(target 0) at the call site — train_hardway_1frame.py:113,130-131.
  * Adam(lr, betas (0.9,0.999), eps 1e-8, coupled L2 weight_decay) —
    train_hardway_1frame.py:116,134 (torch.optim.Adam semantics).
  * nn.DataParallel semantics: per-replica local negatives — model.py:114-115.
  * The 16-frame two-view step: frame/spectrogram folding, two forwards, lw*CE x2,
    (100-lw)*MSE(weighted_A, weighted_A_aug), PropagationLoss x2 — train_hardway.py:126-144,
    losses.py:16-23 (restated from text: losses.py is not importable).
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

# --------------------------------------------------------------------------------------
# parameter / buffer inventory (state_dict order of the reference AVENet)
# --------------------------------------------------------------------------------------

STAGES = [(64, 1), (128, 2), (256, 2), (512, 1)]  # (planes, stride); layer4 stride 1 — base_models.py:149


def _bn_entries(prefix: str, c: int) -> List[Tuple[str, tuple, str]]:
    return [
        (prefix + ".weight", (c,), "bn_w"),
        (prefix + ".bias", (c,), "bn_b"),
        (prefix + ".running_mean", (c,), "rm"),
        (prefix + ".running_var", (c,), "rv"),
        (prefix + ".num_batches_tracked", (), "nbt"),
    ]


def resnet18_entries(prefix: str) -> List[Tuple[str, tuple, str]]:
    """state_dict entries of base_models.resnet18 (base_models.py:113-169), in order."""
    e = [
        (prefix + "conv1_a.weight", (64, 1, 7, 7), "conv"),
        (prefix + "conv1.weight", (64, 3, 7, 7), "conv"),
        (prefix + "conv1_flow.weight", (64, 6, 7, 7), "conv"),
    ]
    e += _bn_entries(prefix + "bn1", 64)
    inplanes = 64
    for li, (planes, stride) in enumerate(STAGES, start=1):
        for bi in range(2):
            s = stride if bi == 0 else 1
            p = f"{prefix}layer{li}.{bi}."
            cin = inplanes if bi == 0 else planes
            e.append((p + "conv1.weight", (planes, cin, 3, 3), "conv"))
            e += _bn_entries(p + "bn1", planes)
            e.append((p + "conv2.weight", (planes, planes, 3, 3), "conv"))
            e += _bn_entries(p + "bn2", planes)
            if bi == 0 and (s != 1 or inplanes != planes):
                e.append((p + "downsample.0.weight", (planes, inplanes, 1, 1), "conv"))
                e += _bn_entries(p + "downsample.1", planes)
        inplanes = planes
    e.append((prefix + "fc.weight", (1000, 512), "fc_w"))
    e.append((prefix + "fc.bias", (1000,), "fc_b"))
    return e


def avenet_entries() -> List[Tuple[str, tuple, str]]:
    return resnet18_entries("imgnet.") + resnet18_entries("audnet.")


def make_state(seed: int = 0, dtype=torch.float32) -> "OrderedDict[str, torch.Tensor]":
    """Deterministic weights from a numpy PCG64 seed, following the reference init rule.

    conv: kaiming_normal_(mode='fan_out', nonlinearity='relu') -> N(0, 2/fan_out) (model.py:104-107);
    BN: weight ~ N(1, 0.02), bias 0 (model.py:108-110); running stats 0/1; fc: U(+-1/sqrt(512)).
    """
    rng = np.random.Generator(np.random.PCG64(seed))
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape, kind in avenet_entries():
        if kind == "conv":
            fan_out = shape[0] * shape[2] * shape[3]
            a = rng.standard_normal(shape, dtype=np.float64) * math.sqrt(2.0 / fan_out)
        elif kind == "bn_w":
            a = 1.0 + 0.02 * rng.standard_normal(shape, dtype=np.float64)
        elif kind in ("bn_b", "rm"):
            a = np.zeros(shape)
        elif kind == "rv":
            a = np.ones(shape)
        elif kind == "nbt":
            sd[name] = torch.zeros((), dtype=torch.long)
            continue
        elif kind in ("fc_w", "fc_b"):
            b = 1.0 / math.sqrt(512.0)
            a = rng.uniform(-b, b, size=shape)
        else:  # pragma: no cover
            raise ValueError(kind)
        sd[name] = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    return sd


# --------------------------------------------------------------------------------------
# synthetic inputs
# --------------------------------------------------------------------------------------

def make_image(batch: int, size: int = 224, seed: int = 1) -> torch.Tensor:
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.standard_normal((batch, 3, size, size), dtype=np.float32))


def make_gout(batch: int, h: int, w: int, seed: int = 7) -> torch.Tensor:
    """A fixed dense standard-normal upstream gradient of a trunk's layer4 map [batch,512,h,w], rounded to bf16 once
    (the trunk's backward takes it in bf16: both sides of a comparison then see the same values)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = torch.from_numpy(rng.standard_normal((batch, 512, h, w), dtype=np.float32))
    return g.to(torch.bfloat16).float()


def make_cot(batch: int, h: int, w: int, scale: float = 1.0, maps: bool = True, seed: int = 11) -> dict:
    """Fixed cotangents of the one-frame step's outputs for avenet_forced_grads: "scale" multiplies CE(logits, 0);
    with maps, dense standard-normal "wA" [batch,h,w] and "A", "Pos", "Neg" [batch,1,h,w] (fp32, as the head's
    backward takes them), else None."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cot = {"scale": scale, "wA": None, "A": None, "Pos": None, "Neg": None}
    if maps:
        cot["wA"] = torch.from_numpy(rng.standard_normal((batch, h, w), dtype=np.float32))
        for k in ("A", "Pos", "Neg"):
            cot[k] = torch.from_numpy(rng.standard_normal((batch, 1, h, w), dtype=np.float32))
    return cot


def make_spectrogram(batch: int, freq: int = 257, frames: int = 300, seed: int = 2) -> torch.Tensor:
    """log-spectrogram recipe of datasets/dataloader.py:86-96 on clipped Gaussian noise.

    scipy.signal.spectrogram(nperseg=512, noverlap=1) gives 257 bins; the sample count is
    chosen so the frame count is exactly ``frames`` (511*frames + 1 samples).  Reduced
    frequency sizes (tiny fixtures) keep the first ``freq`` bins.
    """
    from scipy import signal

    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.empty((batch, 1, freq, frames), dtype=np.float32)
    for b in range(batch):
        s = np.clip(0.1 * rng.standard_normal(511 * frames + 1), -1.0, 1.0)
        _, _, spec = signal.spectrogram(s, 16000, nperseg=512, noverlap=1)
        spec = np.log(spec + 1e-7) / 12.0
        out[b, 0] = spec[:freq, :frames].astype(np.float32)
    return torch.from_numpy(out)


def make_tube_features(b: int, t: int, hw: int, c: int, seed: int = 5):
    """Post-ReLU-like normalised features for the HardWayAttention head (fp64)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    vid = torch.from_numpy(np.abs(rng.standard_normal((b, c, t, hw, hw))))
    vid = F.normalize(vid, dim=1)
    aud = torch.from_numpy(np.abs(rng.standard_normal((b * t, c))) + 0.5)
    aud = F.normalize(aud, dim=1)
    return vid, aud


# --------------------------------------------------------------------------------------
# forward
# --------------------------------------------------------------------------------------

class Args:
    """The args namespace AVENet reads (model.py:98-102; defaults train_hardway_1frame.py:54-60)."""

    def __init__(self, epsilon=0.65, epsilon2=0.4, tri_map=True, Neg=True):
        self.epsilon, self.epsilon2, self.tri_map, self.Neg = epsilon, epsilon2, tri_map, Neg


def _bn(x, sd, prefix, training, momentum=0.1, eps=1e-5):
    # BatchNorm2d train mode: biased batch var for normalisation, unbiased var for running stats.
    if training and (prefix + ".num_batches_tracked") in sd:
        sd[prefix + ".num_batches_tracked"].add_(1)
    return F.batch_norm(x, sd[prefix + ".running_mean"], sd[prefix + ".running_var"],
                        sd[prefix + ".weight"], sd[prefix + ".bias"], training, momentum, eps)


def resnet18_forward(sd, prefix: str, x: torch.Tensor, modal: str, training: bool = True):
    """base_models.py:195-210 (stem chosen by modal, layer4 stride 1)."""
    stem = prefix + ("conv1_a.weight" if modal == "audio" else "conv1.weight")
    x = F.conv2d(x, sd[stem], stride=2, padding=3)
    x = F.relu(_bn(x, sd, prefix + "bn1", training))
    x = F.max_pool2d(x, 3, 2, 1)
    inplanes = 64
    for li, (planes, stride) in enumerate(STAGES, start=1):
        for bi in range(2):
            s = stride if bi == 0 else 1
            p = f"{prefix}layer{li}.{bi}."
            idt = x
            out = F.conv2d(x, sd[p + "conv1.weight"], stride=s, padding=1)
            out = F.relu(_bn(out, sd, p + "bn1", training))
            out = F.conv2d(out, sd[p + "conv2.weight"], stride=1, padding=1)
            out = _bn(out, sd, p + "bn2", training)
            if (p + "downsample.0.weight") in sd:
                idt = F.conv2d(x, sd[p + "downsample.0.weight"], stride=s)
                idt = _bn(idt, sd, p + "downsample.1", training)
            x = F.relu(out + idt)
        inplanes = planes
    return x


def _max_pool2d_last(x: torch.Tensor) -> torch.Tensor:
    """MaxPool2d(3, 2, 1) whose gradient goes to the LAST maximum of a window in scan order (torch's own, and the
    trunk's, go to the first): resnet18_forward_forced's "pool_last" fault."""
    xp = F.pad(x, (1, 1, 1, 1), value=float("-inf"))
    Ho, Wo = [(n - 1) // 2 + 1 for n in x.shape[2:]]
    taps = torch.stack([xp[:, :, dh:dh + 2 * Ho:2, dw:dw + 2 * Wo:2] for dh in range(3) for dw in range(3)])
    idx = 8 - taps.detach().flip(0).argmax(0, keepdim=True)  # argmax returns the first of equal maxima
    return taps.gather(0, idx)[0]


FORCED_FAULTS_2D = ("drop_identity", "drop_downsample", "mask_c2", "pool_last", "unmasked_class00")


def resnet18_forward_forced(sd, prefix: str, x: torch.Tensor, modal: str, tape: dict, grad_round=None,
                            fault: str = None) -> torch.Tensor:
    """resnet18_forward's graph in train mode, "teacher-forced" onto a recorded forward state: for a fixed forward
    state the backward is a linear map of the upstream gradient, so autograd through this function is the reference of
    a trunk's backward on that trunk's OWN forward, with the forward's rounding noise (flipped ReLU masks, shifted
    batch statistics) taken out of the comparison.  tape (NCHW): c0 the stem conv output, p0 the pooled stem output
    (block 0's input), blocks[i] = c1, h1, c2, cd (a downsample block), out.
      * every conv output is set to the tape's value, z + (v - z).detach(); the batch statistics are those of the
        forced conv outputs (no running statistics are read or written);
      * every ReLU output is z * [stored > 0] (h1, out: the recorded masks), then set to the stored value;
      * the stem's full-resolution ReLU output is on no tape: the max-pool acts on relu(bn(c0 forced)) computed here
        (torch routes a window's gradient to its first maximum), times [p0 > 0], set to p0;
      * sd: the weights to differentiate (the caller rounds the conv weights to bf16); x takes its bf16-rounded value
        here, its gradient passing straight through.
    grad_round: a function applied (as an autograd hook) to the gradient of every activation the trunk's backward
    stores -- c0, p0, c1, h1, c2, cd, out -- e.g. a rounding to bf16: the yardstick of a correct implementation with
    those storage formats.  fault (tests only; FORCED_FAULTS_2D): a deliberately mis-wired graph -- "drop_identity"
    layer1.1's identity branch passes no gradient, "drop_downsample" layer2.0's downsample branch passes none,
    "mask_c2" the block-output masks are [c2 > 0], "pool_last" the max-pool gradient goes to a window's last maximum,
    "unmasked_class00" layer1.1's output ReLU mask is not applied to the gradient at the (even, even) pixels (those a
    stride-2 conv1 dgrad leaves to the 1x1 downsample dgrad above it)."""
    assert fault is None or fault in FORCED_FAULTS_2D, fault
    stem = prefix + ("conv1_a.weight" if modal == "audio" else "conv1.weight")
    dt = sd[stem].dtype

    def keep(t):
        if grad_round is not None and t.requires_grad:
            t.register_hook(grad_round)
        return t

    def force(z, v):
        return keep(z + (v.to(dt) - z).detach())

    def bn(c, name):
        return F.batch_norm(c, None, None, sd[name + ".weight"], sd[name + ".bias"], True, 0.0, 1e-5)

    x = x.to(dt)
    x = x + (x.to(torch.bfloat16).to(dt) - x).detach()
    c = force(F.conv2d(x, sd[stem], stride=2, padding=3), tape["c0"])
    a = F.relu(bn(c, prefix + "bn1"))
    pooled = _max_pool2d_last(a) if fault == "pool_last" else F.max_pool2d(a, 3, 2, 1)
    x = force(pooled * (tape["p0"] > 0), tape["p0"])
    blocks = iter(tape["blocks"])
    for li, (planes, stride) in enumerate(STAGES, start=1):
        for bi in range(2):
            s = stride if bi == 0 else 1
            p = f"{prefix}layer{li}.{bi}."
            tb = next(blocks)
            c1 = force(F.conv2d(x, sd[p + "conv1.weight"], stride=s, padding=1), tb["c1"])
            h1 = force(bn(c1, p + "bn1") * (tb["h1"] > 0), tb["h1"])
            c2 = force(F.conv2d(h1, sd[p + "conv2.weight"], stride=1, padding=1), tb["c2"])
            z = bn(c2, p + "bn2")
            if (p + "downsample.0.weight") in sd:
                cd = force(F.conv2d(x, sd[p + "downsample.0.weight"], stride=s), tb["cd"])
                idt = bn(cd, p + "downsample.1")
                if fault == "drop_downsample" and (li, bi) == (2, 0):
                    idt = idt.detach()
            else:
                idt = x.detach() if fault == "drop_identity" and (li, bi) == (1, 1) else x
            mask = (tb["c2"] > 0) if fault == "mask_c2" else (tb["out"] > 0)
            if fault == "unmasked_class00" and (li, bi) == (1, 1):
                mask = mask.clone()
                mask[:, :, ::2, ::2] = True
            x = force((z + idt) * mask, tb["out"])
    return x


def resnet18_forced_grads(sd, x: torch.Tensor, modal: str, tape: dict, g_out: torch.Tensor,
                          round_grads: bool = False, fault: str = None, prefix: str = None):
    """{name without prefix: fp64 gradient} of (resnet18_forward_forced(...) * g_out).sum() on the CPU for every
    trainable parameter of the trunk (the modal stem, the BN affine parameters, the block convs), plus "input": the
    gradient of x at its bf16-rounded value.  Conv weights are the bf16-rounded parameters in fp64 (the gradient is
    taken at them), BN parameters stay fp64.  prefix: the trunk's keys in sd (default by modal: "audnet." /
    "imgnet.").  round_grads: every stored activation gradient is rounded to bf16 (the weight and input gradients
    stay full sums)."""
    if prefix is None:
        prefix = "audnet." if modal == "audio" else "imgnet."
    skip = ("conv1_flow.weight", "conv1.weight" if modal == "audio" else "conv1_a.weight")
    names = [n for n, _, kind in resnet18_entries(prefix)
             if kind in ("conv", "bn_w", "bn_b") and n[len(prefix):] not in skip]
    s = {}
    for n in names:
        v = sd[n].detach()
        v = v.to(torch.bfloat16) if v.dim() == 4 else v
        s[n] = v.to(torch.float64).clone().requires_grad_(True)
    xin = x.detach().to(torch.bfloat16).to(torch.float64).requires_grad_(True)
    rnd = (lambda g: g.to(torch.bfloat16).to(g.dtype)) if round_grads else None
    tape64 = {k: v.double() for k, v in tape.items() if k != "blocks"}
    tape64["blocks"] = [{k: v.double() for k, v in tb.items()} for tb in tape["blocks"]]
    feat = resnet18_forward_forced(s, prefix, xin, modal, tape64, grad_round=rnd, fault=fault)
    assert feat.shape == g_out.shape, (feat.shape, g_out.shape)
    (feat * g_out.double()).sum().backward()
    # (a parameter a fault cuts off the graph has no gradient: zeros)
    out = {n[len(prefix):]: (s[n].grad if s[n].grad is not None else torch.zeros_like(s[n])) for n in names}
    out["input"] = xin.grad
    return out


def hardway_head(img_n: torch.Tensor, aud_n: torch.Tensor, epsilon=0.65, epsilon2=0.4, tau=0.03,
                 tri_map=True, neg=True):
    """model.py:114-154 given the normalised maps: img_n [B,C,h,w], aud_n [B,C]."""
    B = img_n.shape[0]
    mask = 1 - 100 * torch.eye(B, B, dtype=img_n.dtype)
    A = torch.einsum("ncqa,nc->nqa", img_n, aud_n).unsqueeze(1)             # model.py:124
    A0 = torch.einsum("ncqa,kc->nkqa", img_n, aud_n)                         # model.py:125
    Pos = torch.sigmoid((A - epsilon) / tau)
    if tri_map:
        Neg = 1 - torch.sigmoid((A - epsilon2) / tau)
    else:
        Neg = 1 - Pos
    Pos_all = torch.sigmoid((A0 - epsilon) / tau)
    sim1 = (Pos * A).flatten(2).sum(-1) / Pos.flatten(2).sum(-1)
    sim = ((Pos_all * A0).flatten(2).sum(-1) / Pos_all.flatten(2).sum(-1)) * mask
    sim2 = (Neg * A).flatten(2).sum(-1) / Neg.flatten(2).sum(-1)
    logits = torch.cat((sim1, sim, sim2), 1) / 0.07 if neg else torch.cat((sim1, sim), 1) / 0.07
    norm_pos = F.normalize(Pos, dim=(2, 3))
    weighted_A = (img_n * norm_pos).mean(dim=1)
    return A, logits, weighted_A, Pos, Neg


def avenet_forward(sd, image, audio, args: Args = None, training: bool = True):
    """AVENet.forward (model.py:112-154). Returns (A, logits, weighted_A, Pos, Neg)."""
    args = args or Args()
    img = resnet18_forward(sd, "imgnet.", image, "vision", training)
    img = F.normalize(img, dim=1)
    aud = resnet18_forward(sd, "audnet.", audio, "audio", training)
    aud = F.adaptive_max_pool2d(aud, 1).flatten(1)
    aud = F.normalize(aud, dim=1)
    return hardway_head(img, aud, args.epsilon, args.epsilon2, 0.03, args.tri_map, args.Neg)


def hardway_attention(audio_features, video_features):
    """HardWayAttention.forward (model.py:46-60): aud [(b t), C], vid [b, C, t, h, w]."""
    b, c, t, h, w = video_features.shape
    vid = video_features.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)
    A, logits, _, _, _ = hardway_head(vid, audio_features, 0.65, 0.4, 0.03, True, True)
    return A, logits


def hardway_ce(logits: torch.Tensor) -> torch.Tensor:
    """nn.CrossEntropyLoss()(logits, zeros) — train_hardway_1frame.py:113,130-131."""
    target = torch.zeros(logits.shape[0], dtype=torch.long)
    return F.cross_entropy(logits, target)


# --------------------------------------------------------------------------------------
# train step (fwd + CE + bwd + Adam)
# --------------------------------------------------------------------------------------

def trainable_names(sd) -> List[str]:
    """Parameters that receive gradients on the 1-frame step (the stems of the other
    modality, conv1_flow and both fc never do — SURVEY §7 'Unused parameters')."""
    out = []
    for name, _, kind in avenet_entries():
        if kind not in ("conv", "bn_w", "bn_b"):
            continue
        if name.endswith("conv1_flow.weight"):
            continue
        if name.startswith("imgnet.") and name.endswith("conv1_a.weight"):
            continue
        if name.startswith("audnet.") and name.endswith("conv1.weight") and ".layer" not in name:
            continue
        out.append(name)
    return out


class AdamRef:
    """torch.optim.Adam (single-tensor, amsgrad=False, coupled weight decay) restated."""

    def __init__(self, lr=1e-6, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4):
        self.lr, self.b1, self.b2, self.eps, self.wd = lr, betas[0], betas[1], eps, weight_decay
        self.state: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        self.t = 0

    def step(self, params: Dict[str, torch.Tensor], grads: Dict[str, torch.Tensor]):
        self.t += 1
        bc1 = 1 - self.b1 ** self.t
        bc2 = 1 - self.b2 ** self.t
        step_size = self.lr / bc1
        bc2_sqrt = math.sqrt(bc2)
        for name, p in params.items():
            g = grads[name]
            if self.wd != 0:
                g = g + self.wd * p
            m, v = self.state.get(name, (torch.zeros_like(p), torch.zeros_like(p)))
            m = m * self.b1 + (1 - self.b1) * g
            v = v * self.b2 + (1 - self.b2) * g * g
            self.state[name] = (m, v)
            denom = v.sqrt() / bc2_sqrt + self.eps
            p -= step_size * m / denom


def train_step(sd, image, audio, opt: AdamRef = None, args: Args = None):
    """One hard-way step: forward, CE(target 0), backward, Adam. Mutates ``sd`` in place.

    Returns (loss, logits, grads) with grads keyed by parameter name.
    """
    names = trainable_names(sd)
    leaves = {n: sd[n].detach().clone().requires_grad_(True) for n in names}
    work = OrderedDict(sd)
    work.update(leaves)
    _, logits, _, _, _ = avenet_forward(work, image, audio, args, training=True)
    loss = hardway_ce(logits)
    gl = torch.autograd.grad(loss, [leaves[n] for n in names])
    grads = {n: g for n, g in zip(names, gl)}
    # BN running stats / num_batches_tracked were updated in place (shared tensors with sd)
    if opt is not None:
        with torch.no_grad():
            opt.step({n: sd[n] for n in names}, grads)
    return loss.detach(), logits.detach(), grads


# --------------------------------------------------------------------------------------
# 16-frame two-view step (train_hardway.py:126-144)
# --------------------------------------------------------------------------------------

def propagation_loss(heatmap: torch.Tensor) -> torch.Tensor:
    """PropagationLoss.forward (losses.py:22-23) on heatmap [b, t, h, w].  losses.py is not
    importable here (`from turtle import pos`, pytorch_metric_learning, torchvision: SURVEY §8c),
    so this one-liner is restated from its text."""
    return torch.abs(torch.diff(heatmap, dim=1)).mean(dim=(2, 3)).mean(dim=1).mean(dim=0)


def npratio_loss(heatmap: torch.Tensor) -> torch.Tensor:
    """NPRatio.forward (losses.py:13-14) on heatmap [b, t, h, w], restated from its text (losses.py is
    not importable here: SURVEY §8c)."""
    return torch.abs(torch.diff(torch.sum(heatmap, dim=(2, 3)), dim=1)).mean(dim=1).mean(dim=0)


def flip_loss(heatmap: torch.Tensor, flipped_heatmap: torch.Tensor) -> torch.Tensor:
    """FlipLoss.forward (losses.py:34-36): nn.L1Loss()(flipped_heatmap, RandomHorizontalFlip(p=1)(heatmap));
    torchvision's tensor hflip is heatmap.flip(-1) (torchvision is absent here: restated)."""
    return F.l1_loss(flipped_heatmap, heatmap.flip(-1))


def twoview_losses(out1, out2, b: int, t: int, loss_weight: float = 0.1):
    """train_hardway.py:134-142 given the two AVENet outputs (A, logits, weighted_A, Pos, Neg).
    weighted.reshape(batch_size, frame_density, 14, 14) is written for the layer4 map's own (h, w).
    Returns (combined, hardway, aug, l2, consistency)."""
    _, logits1, w1, _, _ = out1
    _, logits2, w2, _, _ = out2
    hardway = hardway_ce(logits1) * loss_weight
    aug = hardway_ce(logits2) * loss_weight
    l2 = F.mse_loss(w1, w2) * (100 - loss_weight)
    h, w = w1.shape[-2:]
    consistency = propagation_loss(w1.reshape(b, t, h, w)) + propagation_loss(w2.reshape(b, t, h, w))
    combined = (hardway + aug) / 2 + l2 + consistency
    return combined, hardway, aug, l2, consistency


def fold_frames(frames: torch.Tensor) -> torch.Tensor:
    """einops 'b c t h w -> (b t) c h w' (train_hardway.py:130-131)."""
    b, c, t, h, w = frames.shape
    return frames.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)


def fold_spec(spec: torch.Tensor, t: int) -> torch.Tensor:
    """spec.unsqueeze(2).repeat(1, 1, t, 1, 1) then 'b c t h w -> (b t) c h w' (train_hardway.py:128-129)."""
    return fold_frames(spec.unsqueeze(2).repeat(1, 1, t, 1, 1))


def twoview_step(sd, frames, augmented, spec, opt: AdamRef = None, args: Args = None, loss_weight: float = 0.1):
    """One train_hardway.py step (126-144): two AVENet forwards (frames, augmented) on the 16x
    repeated spectrogram, the combined loss, backward, Adam.  Mutates ``sd`` (BN buffers are updated
    by both forwards; Adam if ``opt``).  frames/augmented [b,3,t,H,W], spec [b,1,F,T].
    Returns (losses (combined, hardway, aug, l2, consistency), out1, out2, grads)."""
    b, t = frames.shape[0], frames.shape[2]
    names = trainable_names(sd)
    leaves = {n: sd[n].detach().clone().requires_grad_(True) for n in names}
    work = OrderedDict(sd)
    work.update(leaves)
    aud = fold_spec(spec, t)
    out1 = avenet_forward(work, fold_frames(frames), aud, args, training=True)
    out2 = avenet_forward(work, fold_frames(augmented), aud, args, training=True)
    losses = twoview_losses(out1, out2, b, t, loss_weight)
    gl = torch.autograd.grad(losses[0], [leaves[n] for n in names])
    grads = {n: g for n, g in zip(names, gl)}
    if opt is not None:
        with torch.no_grad():
            opt.step({n: sd[n] for n in names}, grads)
    return (tuple(x.detach() for x in losses), tuple(o.detach() for o in out1), tuple(o.detach() for o in out2),
            grads)


def make_frames(b: int, t: int, size: int = 224, seed: int = 3) -> torch.Tensor:
    """Seeded synthetic clip frames [b,3,t,H,W] (ImageNet-normalised range, like make_image)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.standard_normal((b, 3, t, size, size), dtype=np.float32))


# --------------------------------------------------------------------------------------
# the whole step's backward on a recorded forward ("forced tape")
# --------------------------------------------------------------------------------------

STEP_FAULTS = ("detach_audio", "const_norm", "pool_spread", "ce_sum", "gan_overwrite")


def _forced_leaves(sd):
    """(names, {name: fp64 leaf}) of trainable_names(sd): conv weights at their bf16-rounded values (the operands the
    trunks compute with), BN parameters as they are."""
    names = trainable_names(sd)
    s = {}
    for n in names:
        v = sd[n].detach()
        v = v.to(torch.bfloat16) if v.dim() == 4 else v
        s[n] = v.to(torch.float64).clone().requires_grad_(True)
    return names, s


def _bf16_leaf(x: torch.Tensor) -> torch.Tensor:
    return x.detach().to(torch.bfloat16).to(torch.float64).requires_grad_(True)


def _tape64(tape: dict) -> dict:
    out = {k: v.double() for k, v in tape.items() if k != "blocks"}
    out["blocks"] = [{k: v.double() for k, v in tb.items()} for tb in tape["blocks"]]
    return out


def _grad_or_zero(t: torch.Tensor) -> torch.Tensor:
    return t.grad if t.grad is not None else torch.zeros_like(t)  # (a fault may cut a leaf off the graph)


def _forced_audio_vectors(s, ain, tape_aud, amax, rnd, fault):
    """The audio trunk forced onto its tape, the global max-pool AT THE RECORDED POSITIONS amax [B,C] (row index
    y * w + x of the layer4 map), F.normalize: the unit vectors [B,C].  The recorded position must hold the channel's
    maximum: among equal bf16 maxima the gradient then goes where the recorded forward sent it."""
    a = resnet18_forward_forced(s, "audnet.", ain, "audio", _tape64(tape_aud), grad_round=rnd)
    flat = a.flatten(2)
    pooled = flat.gather(2, amax.long().unsqueeze(-1)).squeeze(-1)
    assert torch.equal(pooled.detach(), flat.detach().amax(-1)), "amax does not point at the channel maxima"
    if fault == "pool_spread":
        mean = flat.mean(-1)
        pooled = mean + (pooled - mean).detach()
    an = F.normalize(pooled, dim=1)
    return an.detach() if fault == "detach_audio" else an


def _forced_vision_map(s, xin, tape_img, rnd, fault):
    """The vision trunk forced onto its tape, L2-normalised over channels.  (The gradient of the stored map v is
    rounded by rnd: v is block 7's output, one of the tensors resnet18_forward_forced hooks.)"""
    v = resnet18_forward_forced(s, "imgnet.", xin, "vision", _tape64(tape_img), grad_round=rnd)
    if fault == "const_norm":
        return v / v.detach().norm(dim=1, keepdim=True).clamp_min(1e-12)
    return F.normalize(v, dim=1)


def _bf16_round(g):
    return g.to(torch.bfloat16).to(g.dtype)


def avenet_forced_grads(sd, image, audio, tape: dict, cot: dict, round_grads: bool = False, fault: str = None,
                        args: Args = None, tau: float = 0.03):
    """The one-frame step's backward on a recorded forward: {name: fp64 gradient} for trainable_names(sd), plus
    "image" and "audio" (the input gradients at the bf16-rounded inputs), of
        cot.scale * CE(logits, 0) + <cot.wA, weighted_A> + <cot.A, A> + <cot.Pos, Pos> + <cot.Neg, Neg>
    (make_cot; a None cotangent drops its term) with both trunks teacher-forced (resnet18_forward_forced) onto
    tape["img"] / tape["aud"] (NCHW: c0, p0, blocks), so that the head sees exactly the recorded layer4 maps, the
    audio pool taken at tape["amax"] [B,C], and the head (F.normalize, hardway_head with args and tau) in fp64.
    round_grads: the yardstick -- every activation gradient the trunks store in bf16 is rounded to bf16 (the set
    resnet18_forced_grads hooks; it includes both layer4 maps' gradients); the gradient of the audio vectors and the
    head's internals stay unrounded (kept in fp32 on the GPU).
    fault (tests only; STEP_FAULTS): "detach_audio" no gradient reaches the audio vectors, "const_norm" the vision
    map's L2 normalisation is a constant scale in the backward, "pool_spread" the audio pool's gradient is spread as
    a mean over positions, "ce_sum" CE summed over the batch."""
    assert fault is None or (fault in STEP_FAULTS and fault != "gan_overwrite"), fault
    args = args or Args()
    names, s = _forced_leaves(sd)
    xin, ain = _bf16_leaf(image), _bf16_leaf(audio)
    rnd = _bf16_round if round_grads else None
    vn = _forced_vision_map(s, xin, tape["img"], rnd, fault)
    an = _forced_audio_vectors(s, ain, tape["aud"], tape["amax"], rnd, fault)
    A, logits, wA, Pos, Neg = hardway_head(vn, an, args.epsilon, args.epsilon2, tau, args.tri_map, args.Neg)
    target = torch.zeros(logits.shape[0], dtype=torch.long)
    loss = cot["scale"] * F.cross_entropy(logits, target, reduction="sum" if fault == "ce_sum" else "mean")
    for k, out in (("wA", wA), ("A", A), ("Pos", Pos), ("Neg", Neg)):
        if cot.get(k) is not None:
            loss = loss + (cot[k].double().reshape(out.shape) * out).sum()
    loss.backward()
    grads = {n: _grad_or_zero(s[n]) for n in names}
    grads["image"], grads["audio"] = _grad_or_zero(xin), _grad_or_zero(ain)
    return grads


def twoview_forced_grads(sd, frames, augmented, spec, tape: dict, loss_weight: float = 0.1, dedup_audio: bool = True,
                         round_grads: bool = False, fault: str = None, args: Args = None, tau: float = 0.03):
    """The two-view step's backward (twoview_step's loss: twoview_losses(...)[0] with loss_weight) on a recorded
    forward.  frames, augmented [b,3,t,H,W], spec [b,1,F,T]; tape["img"] the two views' vision tapes (each view has
    its own batch statistics); dedup_audio: tape["aud"] = [one tape of the b spectrograms], tape["amax"] = [[b,C]] --
    the unit vectors are repeated t times ('(b t)' rows) and feed both views' heads, so the audio trunk receives the
    gradient summed over frames and views; else two tapes of the folded (b t) spectrograms, one per view.  Returns
    the summed gradients for trainable_names(sd), plus the input gradients "frames", "augmented" (folded,
    [(b t),3,H,W]) and "audio" (dedup) or "audio1", "audio2".  round_grads as avenet_forced_grads.  fault:
    avenet_forced_grads' (not "ce_sum"), or "gan_overwrite": view 1's head passes no gradient to the audio vectors
    (what is left when view 2's audio gradient replaces view 1's where it should add to it)."""
    assert fault is None or (fault in STEP_FAULTS and fault != "ce_sum"), fault
    args = args or Args()
    b, t = frames.shape[0], frames.shape[2]
    names, s = _forced_leaves(sd)
    rnd = _bf16_round if round_grads else None
    xs = [_bf16_leaf(fold_frames(frames)), _bf16_leaf(fold_frames(augmented))]
    assert len(tape["aud"]) == len(tape["amax"]) == (1 if dedup_audio else 2)
    ains = [_bf16_leaf(spec)] if dedup_audio else [_bf16_leaf(fold_spec(spec, t)) for _ in range(2)]
    ans = [_forced_audio_vectors(s, ain, ta, am, rnd, fault) for ain, ta, am in zip(ains, tape["aud"], tape["amax"])]
    if dedup_audio:
        ans = [ans[0].repeat_interleave(t, 0)] * 2
    if fault == "gan_overwrite":
        ans[0] = ans[0].detach()
    outs = [hardway_head(_forced_vision_map(s, x, ti, rnd, fault), an, args.epsilon, args.epsilon2, tau,
                         args.tri_map, args.Neg) for x, ti, an in zip(xs, tape["img"], ans)]
    twoview_losses(outs[0], outs[1], b, t, loss_weight)[0].backward()
    grads = {n: _grad_or_zero(s[n]) for n in names}
    grads["frames"], grads["augmented"] = _grad_or_zero(xs[0]), _grad_or_zero(xs[1])
    for k, ain in zip(("audio",) if dedup_audio else ("audio1", "audio2"), ains):
        grads[k] = _grad_or_zero(ain)
    return grads
