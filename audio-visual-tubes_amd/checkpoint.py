"""Reference-compatible checkpoints.

The reference saves (train_hardway_1frame.py:257-263, train_hardway.py, train_3D.py)
    torch.save({'epoch': epoch, 'model_state_dict': model.state_dict(),
                'optimizer_state_dict': optim.state_dict()}, path)
with ``model`` wrapped in nn.DataParallel (keys prefixed ``module.``) and ``optim`` a torch.optim.Adam
over ``model.parameters()``, and loads with ``model_dict.update(checkpoint['model_state_dict'])``
(train_hardway.py:94-100, test_hardway_dataset.py:66-70, test.py:64-68).

Here the same files are read and written: model keys with or without ``module.``; the optimizer
state either of a torch-API optimizer (``avt_amd.optim.Adam`` / ``torch.optim.Adam``: its own
state_dict) or of the fused steps' flat Adam (``HardWayTrainStep`` / ``TwoViewTrainStep``), which is
converted to and from torch.optim.Adam's layout (state indexed by position in model.parameters(),
conv moments in OIHW) so a checkpoint moves between the reference and this build in both directions.
The flat SGD of ``R3DTrainStep`` converts to and from torch.optim.SGD's layout the same way
(``momentum_buffer`` per parameter).
Files are read with ``torch.load(weights_only=True)``.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

PREFIX = "module."


def _strip(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return {(k[len(PREFIX):] if k.startswith(PREFIX) else k): v for k, v in sd.items()}


def _fused_opt(obj):
    """The FlatAdam / FlatSGD of a fused train step (or the flat optimizer itself), else None."""
    from .optim import FlatAdam, FlatSGD

    if isinstance(obj, (FlatAdam, FlatSGD)):
        return obj
    opt = getattr(obj, "opt", None)
    return opt if isinstance(opt, (FlatAdam, FlatSGD)) else None


def _is_sgd(opt) -> bool:
    from .optim import FlatSGD

    return isinstance(opt, FlatSGD)


def flat_adam_state_dict(model: torch.nn.Module, opt) -> dict:
    """torch.optim.Adam.state_dict() layout of a FlatAdam over ``model``'s parameters."""
    flat = opt.flat
    names = [n for n, _ in model.named_parameters()]
    step = float(opt.t)
    state = {}
    for i, n in enumerate(names):
        if not flat.trainable(n):
            continue  # never receives a gradient: torch's Adam holds no state for it either
        off, shape = flat.poff[n]
        k = 1
        for s in shape:
            k *= s
        views = []
        for buf in (opt.exp_avg, opt.exp_avg_sq):
            t = buf[off:off + k]
            t = t.view(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2) if len(shape) == 4 else t.view(shape)
            views.append(t.detach().clone().contiguous())
        state[i] = {"step": torch.tensor(step), "exp_avg": views[0], "exp_avg_sq": views[1]}
    group = {"lr": opt.lr, "betas": tuple(opt.betas), "eps": opt.eps, "weight_decay": opt.wd, "amsgrad": False,
             "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "params": list(range(len(names)))}
    if getattr(opt, "initial_lr", None) is not None:  # what torch's schedulers add to the group
        group["initial_lr"] = opt.initial_lr
    return {"state": state, "param_groups": [group]}


def load_flat_adam_state_dict(model: torch.nn.Module, opt, sd: dict) -> None:
    """Inverse of flat_adam_state_dict (e.g. a reference checkpoint's optimizer_state_dict)."""
    flat = opt.flat
    names = [n for n, _ in model.named_parameters()]
    groups = sd["param_groups"]
    if len(groups) != 1:
        raise ValueError("avt: expected one Adam param group (train_hardway*.py builds one)")
    g = groups[0]
    if len(g["params"]) != len(names):
        raise ValueError(f"avt: optimizer state covers {len(g['params'])} parameters, model has {len(names)}")
    opt.lr, opt.betas, opt.eps, opt.wd = g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]
    opt.initial_lr = g.get("initial_lr")
    steps = set()
    with torch.no_grad():
        opt.exp_avg.zero_()
        opt.exp_avg_sq.zero_()
        for pos, idx in enumerate(g["params"]):
            st = sd["state"].get(idx)
            if st is None:
                continue
            n = names[pos]
            if not flat.trainable(n):
                continue  # a stale moment of a parameter this step never updates
            off, shape = flat.poff[n]
            k = 1
            for s in shape:
                k *= s
            for buf, key in ((opt.exp_avg, "exp_avg"), (opt.exp_avg_sq, "exp_avg_sq")):
                src = st[key].to(buf.device, torch.float32)
                if len(shape) == 4:
                    src = src.permute(0, 2, 3, 1)
                buf[off:off + k].copy_(src.reshape(-1))
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError(f"avt: per-parameter Adam steps differ ({sorted(steps)}); the flat Adam keeps one")
        opt.t_dev.fill_(steps.pop() if steps else 0)


def _flat_slot(flat, name):
    """(offset, element count, shape) of a parameter in the flat buffers."""
    off, shape = flat.poff[name]
    k = 1
    for s in shape:
        k *= s
    return off, k, shape


def flat_sgd_state_dict(model: torch.nn.Module, opt) -> dict:
    """torch.optim.SGD.state_dict() layout of a FlatSGD over ``model``'s parameters: one ``momentum_buffer`` per
    trainable parameter, indexed by its position in model.parameters() (2-D conv buffers in OIHW; Conv3d, Linear and
    BatchNorm ones as stored).  Before the first step the state is empty, as torch's is; with momentum 0 every buffer
    is None, as torch's are."""
    flat = opt.flat
    names = [n for n, _ in model.named_parameters()]
    state = {}
    if opt.t > 0:
        for i, n in enumerate(names):
            if not flat.trainable(n):
                continue
            buf = None
            if opt.momentum_buffer is not None:
                off, k, shape = _flat_slot(flat, n)
                t = opt.momentum_buffer[off:off + k]
                t = (t.view(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2) if len(shape) == 4
                     else t.view(shape))
                buf = t.detach().clone().contiguous()
            state[i] = {"momentum_buffer": buf}
    group = {"lr": opt.lr, "momentum": opt.momentum, "dampening": opt.dampening, "weight_decay": opt.wd,
             "nesterov": bool(opt.nesterov), "maximize": False, "foreach": None, "differentiable": False, "fused": None,
             "params": list(range(len(names)))}
    if getattr(opt, "initial_lr", None) is not None:
        group["initial_lr"] = opt.initial_lr
    return {"state": state, "param_groups": [group]}


def load_flat_sgd_state_dict(model: torch.nn.Module, opt, sd: dict) -> None:
    """Inverse of flat_sgd_state_dict (e.g. the optimizer_state_dict of a torch.optim.SGD fine-tuning run).  torch's
    SGD keeps no step count: the flat one resumes at step 1 when any momentum buffer is restored (the next step then
    blends into the buffers) and at step 0 otherwise (the next step sets buf = g, as torch's does without a buffer)."""
    flat = opt.flat
    names = [n for n, _ in model.named_parameters()]
    groups = sd["param_groups"]
    if len(groups) != 1:
        raise ValueError("avt: expected one SGD param group")
    g = groups[0]
    if len(g["params"]) != len(names):
        raise ValueError(f"avt: optimizer state covers {len(g['params'])} parameters, model has {len(names)}")
    if g.get("maximize"):
        raise ValueError("avt: FlatSGD does not maximize")
    if g["momentum"] != 0 and opt.momentum_buffer is None:
        raise ValueError("avt: the checkpoint's SGD uses momentum; this FlatSGD was built without a buffer")
    opt.nesterov = False  # (so that no intermediate combination is refused)
    opt.momentum, opt.dampening = g["momentum"], g["dampening"]
    opt.nesterov = bool(g["nesterov"])
    opt.lr, opt.wd = g["lr"], g["weight_decay"]
    opt.initial_lr = g.get("initial_lr")
    restored = 0
    with torch.no_grad():
        if opt.momentum_buffer is not None:
            opt.momentum_buffer.zero_()
        for pos, idx in enumerate(g["params"]):
            st = sd["state"].get(idx)
            if st is None or st.get("momentum_buffer") is None:
                continue
            n = names[pos]
            if not flat.trainable(n):
                continue
            off, k, shape = _flat_slot(flat, n)
            src = st["momentum_buffer"].to(opt.momentum_buffer.device, torch.float32)
            if tuple(src.shape) != tuple(shape):
                raise ValueError(f"avt: momentum_buffer of {n} has shape {tuple(src.shape)}, expected {tuple(shape)}")
            if len(shape) == 4:
                src = src.permute(0, 2, 3, 1)
            opt.momentum_buffer[off:off + k].copy_(src.reshape(-1))
            restored += 1
        opt.t_dev.fill_(1 if restored else 0)


def save_checkpoint(path, epoch: int, model: torch.nn.Module, optimizer=None, data_parallel: bool = True) -> dict:
    """Write the reference's checkpoint dict; ``data_parallel`` adds the ``module.`` prefix the
    reference's nn.DataParallel-wrapped state_dict carries."""
    msd = model.state_dict()
    if data_parallel:
        msd = {PREFIX + k: v for k, v in msd.items()}
    ck = {"epoch": epoch, "model_state_dict": msd}
    if optimizer is not None:
        fused = _fused_opt(optimizer)
        if fused is None:
            ck["optimizer_state_dict"] = optimizer.state_dict()
        else:
            to_sd = flat_sgd_state_dict if _is_sgd(fused) else flat_adam_state_dict
            ck["optimizer_state_dict"] = to_sd(model, fused)
    if path is not None:
        torch.save(ck, path)
    return ck


def load_checkpoint(path_or_dict, model: torch.nn.Module, optimizer=None, map_location="cpu") -> Optional[int]:
    """``model_dict.update(checkpoint['model_state_dict'])`` then load (keys with or without
    ``module.``; keys the model lacks raise, like load_state_dict on the updated dict would).
    Optionally restores the optimizer state.  Returns the checkpoint's epoch (or None)."""
    ck = path_or_dict
    if not isinstance(ck, dict):
        ck = torch.load(path_or_dict, map_location=map_location, weights_only=True)
    sd = ck.get("model_state_dict", ck)
    model_dict = model.state_dict()
    upd = _strip(sd)
    unknown = sorted(set(upd) - set(model_dict))
    if unknown:
        raise KeyError(f"avt: checkpoint keys not in the model: {unknown[:5]}{' ...' if len(unknown) > 5 else ''}")
    model_dict.update(upd)
    model.load_state_dict(model_dict)
    if optimizer is not None and "optimizer_state_dict" in ck:
        fused = _fused_opt(optimizer)
        if fused is not None:
            load = load_flat_sgd_state_dict if _is_sgd(fused) else load_flat_adam_state_dict
            load(model, fused, ck["optimizer_state_dict"])
        else:
            optimizer.load_state_dict(ck["optimizer_state_dict"])
    return ck.get("epoch")
