"""3-D tube step (BASELINE config 4) on libavt: FullModel = R3D-18 video trunk (forward only inside FullModel;
trainable on its own after ``resnet3D.ResNet.enable_backward()``: R3DTrunk.backward / R3DEngine.backward) +
audio ResNet-18 (forward + backward) + the hard-way attention head.

Restates model.py:17-60 and the train_3D.py step (126-138):
  spec [b,1,F,T] --repeat t, fold (b t)--> audio [bt,1,F,T] --audnet--> [bt,512,h',w']
      --AdaptiveMaxPool2d(1), normalize--> an [bt,512]
  video [b,3,t,H,W] --vidnet (R3D-18, no max-pool)--> layer4 [b,512,t,h,w] (forward hook,
      DETACHED: model.py:12-15, 34) --normalize, '(b t) c h w'--> HardWayAttention -> (A, logits)
  CE(logits, 0) -> backward into audnet only -> Adam.
  Opt-in (FullModel.enable_video_backward): the layer4 map stays attached -- the head backward also yields
  gv, R3DTrunk.backward fills the vidnet gradients (all but vidnet.fc, which sits behind the tap) in the same flat
  buffer, on the current stream while the audio trunk's backward runs on the second one.

Device data flow (NHWC / NDHWC bf16 activations, fp32 statistics):
  video fp32 NCDHW --avt_video_stem_im2col--> [b,t,H,W,32] (7 temporal taps folded into channels)
      --avt_conv2d_fwd 7x7/s2 (32 ch)--> stem --BN--> layer1..4: avt_conv3d_fwd 3x3x3 (spatial
      stride 2 on layer2-4's first conv), 1x1x1/s(1,2,2) downsample as avt_conv2d_fwd over the b*t
      frames, BN3d + ReLU (+ residual) by avt_bn_apply --> v [b*t, h, w, 512] = '(b t) h w c'.
  The vidnet's avgpool/fc (resnet3D.py:208-212) feed only the discarded `_` of model.py:33: not run.
  Folded inference (opt-in, eval + no grad: FullModel.enable_folded_inference): every BatchNorm3d folded
  into its conv once (avt_fold_conv3d_bn_batched), the trunk then im2col + 20 avt_conv3d_fwd_bias /
  avt_conv2d_fwd_bias launches with bias (+ residual) (+ ReLU) epilogues -- no BN pass, no per-call weight pack.

Audio de-duplication: given the per-clip spectrogram [b,1,F,T] (what the dataloader yields, before
train_3D.py:128-130 repeats it), the audio trunk runs once per clip with BN statistics identical to
the repeated batch's (the running variance gets the repeated batch's unbiased factor,
avt_bn_finalize_rep); the unit vectors are repeated to the bt head rows and the head gradient is
summed back over each clip's t rows.  This is exact (the backward is linear in the upstream
gradient for the shared forward), and cuts the audio trunk's work by t.  Given the folded
[bt,1,F,T] batch (the reference's own API), the trunk runs over all bt rows.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch

from ._lib import call, query
from .engine import AVEngine, FlatStore, _EngineStore, desc_table
from .trunk import DEPTHS, BlockGraph, BNSpec, ConvProfiler, P, Trunk, _bn_finalize, build_blocks, conv_out, stream_ptr

R3D_STAGES = [(64, 1), (128, 2), (256, 2), (512, 2)]  # (planes, spatial stride) — resnet3D.py:136-150


def tube_trainable(name: str) -> bool:
    """FullModel parameters that receive gradients: the audio trunk on the audio path only (the
    vidnet output is detached; audnet.conv1 / conv1_flow / fc are unused)."""
    if not name.startswith("audnet."):
        return False
    if ".fc." in name or name.endswith("conv1_flow.weight") or name == "audnet.conv1.weight":
        return False
    return True


def tube_trainable_e2e(name: str) -> bool:
    """tube_trainable plus the video trunk up to the layer4 tap (FullModel.enable_video_backward): conv1, bn1 and
    layer1..4 with their downsamples.  vidnet.fc sits behind the tap (the discarded `_` of model.py:33) and never
    receives a gradient, so it stays outside the trainable segment: the flat Adam never touches it."""
    if name.startswith("vidnet."):
        return not name.startswith("vidnet.fc.")
    return tube_trainable(name)


@dataclass
class Conv3dSpec:
    name: str
    cin: int
    cout: int
    kt: int
    k: int
    stride: int  # spatial (temporal stride is 1 throughout the R3D-18 of model.py:20)
    pad_t: int
    pad: int
    stem: bool = False

    @property
    def kg(self) -> int:
        return self.k * self.k * 32 if self.stem else self.kt * self.k * self.k * self.cin


class R3DTrunk(BlockGraph):
    """resnet3D ResNet(BasicBlock, [2,2,2,2]) up to layer4, forward and (from a tape) backward; no_max_pool=True
    (FullModel, model.py:20) unless max_pool (the stem's MaxPool3d(3, 2, 1), resnet3D.py:129, 200-201)."""

    def __init__(self, prefix: str, max_pool: bool = False):
        self.prefix = prefix
        self.max_pool = max_pool
        self.stem = Conv3dSpec(prefix + "conv1.weight", 3, 64, 7, 7, 2, 3, 3, stem=True)
        self.bn1 = BNSpec(prefix + "bn1", 64)
        self.blocks = build_blocks(prefix, R3D_STAGES, DEPTHS,
                                   lambda name, cin, cout, k, s: Conv3dSpec(name, cin, cout, k, k, s, k // 2, k // 2))

    def _conv(self, x, b, T, H, W, spec: Conv3dSpec, bn: BNSpec, store, training):
        """Conv3d (+ BN statistics) -> (y [b*T, H', W', K] bf16, stats [4, K], H', W')."""
        Ho, Wo = conv_out(H, spec.k, spec.stride, spec.pad), conv_out(W, spec.k, spec.stride, spec.pad)
        y = torch.empty(b * T, Ho, Wo, spec.cout, device=x.device, dtype=torch.bfloat16)
        acc = store.stat_acc(bn, "fwd", b * T * Ho * Wo) if training else None
        wf = store.packed3d(spec)
        ev = ConvProfiler.begin()
        if spec.stem:  # 7 temporal taps folded into the 32 input channels (tube.hip)
            call("avt_conv2d_fwd", P(x), P(wf), P(y), P(acc), b * T, H, W, 32, spec.cout, spec.k, spec.k, spec.stride,
                 spec.pad, spec.kg, stream_ptr())
            real_k = spec.kt * spec.k * spec.k * spec.cin
        elif spec.kt == 1:  # 1x1x1 downsample: a 2-D conv over the b*T frames
            call("avt_conv2d_fwd", P(x), P(wf), P(y), P(acc), b * T, H, W, spec.cin, spec.cout, spec.k, spec.k,
                 spec.stride, spec.pad, spec.kg, stream_ptr())
            real_k = spec.cin * spec.k * spec.k
        else:
            call("avt_conv3d_fwd", P(x), P(wf), P(y), P(acc), b, T, H, W, spec.cin, spec.cout, spec.kt, spec.k,
                 spec.k, spec.stride, spec.pad_t, spec.pad, stream_ptr())
            real_k = spec.kt * spec.k * spec.k * spec.cin
        ConvProfiler.end(ev, "fwd3d", 2.0 * y.numel() * real_k, 2.0 * (x.numel() + wf.numel() + y.numel()))
        stats = _bn_finalize(y, acc, y.numel() // spec.cout, bn, store, training)
        return y, stats, Ho, Wo

    def forward(self, video: torch.Tensor, store, training: bool, tape: bool = False):
        """video fp32 [b,3,T,H,W] -> layer4 map as '(b t) h w c' bf16 [b*T, h, w, 512].  tape=True: returns
        (map, tape) with everything ``backward`` reads kept alive (the folded input, the stem's c0/s0/h0 and per
        block x, c1, s1, h1, c2, s2, cd, sd, out); without it the launches and the frees are unchanged."""
        tp = {"blocks": []} if tape else None
        video = video.contiguous().float()
        b, C, T, H, W = video.shape
        if C != 3:
            raise ValueError(f"avt: expected video [b,3,t,H,W], got {tuple(video.shape)}")
        x = torch.empty(b, T, H, W, 32, device=video.device, dtype=torch.bfloat16)
        call("avt_video_stem_im2col", P(video), P(x), b, C, T, H, W, self.stem.kt, self.stem.pad_t, stream_ptr())
        if tape:
            tp.update(b=b, x=x, dims=(T, H, W))
        c0, s0, H, W = self._conv(x, b, T, H, W, self.stem, self.bn1, store, training)
        del x
        rows = c0.numel() // 64
        h = torch.empty_like(c0)
        call("avt_bn_apply", P(c0), P(s0[0]), P(s0[1]), None, None, None, P(h), rows, 64, 1, stream_ptr())
        if tape:
            tp.update(c0=c0, s0=s0, h0=h, dims0=(T, H, W))
        del c0
        if self.max_pool:  # resnet3D.py:200-201
            To, Ho, Wo = (T - 1) // 2 + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1
            hp = torch.empty(b * To, Ho, Wo, 64, device=h.device, dtype=torch.bfloat16)
            call("avt_maxpool3d_fwd", P(h), P(hp), b, T, H, W, 64, stream_ptr())
            h, T, H, W = hp, To, Ho, Wo
        for blk in self.blocks:
            c1, s1, Ho, Wo = self._conv(h, b, T, H, W, blk["conv1"], blk["bn1"], store, training)
            h1 = torch.empty_like(c1)
            K = c1.shape[-1]
            rows = c1.numel() // K
            call("avt_bn_apply", P(c1), P(s1[0]), P(s1[1]), None, None, None, P(h1), rows, K, 1, stream_ptr())
            if tape:
                tp["blocks"].append(dict(x=h, c1=c1, s1=s1, h1=h1, dims=(T, H, W, Ho, Wo)))
            del c1
            c2, s2, _, _ = self._conv(h1, b, T, Ho, Wo, blk["conv2"], blk["bn2"], store, training)
            del h1
            out = torch.empty_like(c2)
            cd = sd = None
            if tape:
                tp["blocks"][-1].update(c2=c2, s2=s2, out=out)
            if blk["down"] is not None:
                cd, sd, _, _ = self._conv(h, b, T, H, W, blk["down"], blk["bnd"], store, training)
                if tape:
                    tp["blocks"][-1].update(cd=cd, sd=sd)
                call("avt_bn_apply", P(c2), P(s2[0]), P(s2[1]), P(cd), P(sd[0]), P(sd[1]), P(out), rows, K, 1,
                     stream_ptr())
            else:
                call("avt_bn_apply", P(c2), P(s2[0]), P(s2[1]), P(h), None, None, P(out), rows, K, 1, stream_ptr())
            h, H, W = out, Ho, Wo
        return (h, tp) if tape else h

    # ------------------------------------------------------------------ folded inference forward
    def _conv_bias(self, x, b, T, H, W, spec: Conv3dSpec, store, relu: bool, res=None):
        """relu?(conv3d(x, w * s) + bias (+ res)) in one launch on the folded operands (store.folded3d)."""
        Ho, Wo = conv_out(H, spec.k, spec.stride, spec.pad), conv_out(W, spec.k, spec.stride, spec.pad)
        y = torch.empty(b * T, Ho, Wo, spec.cout, device=x.device, dtype=torch.bfloat16)
        wf, bias = store.folded3d(spec)
        ev = ConvProfiler.begin()
        if spec.stem:  # the 49-tap 7x7 conv over the b*T frames of the 32-channel im2col input
            call("avt_conv3d_fwd_bias", P(x), P(wf), P(y), b * T, 1, H, W, 32, spec.cout, 1, spec.k, spec.k, spec.stride,
                 0, spec.pad, P(bias), P(res), int(relu), stream_ptr())
        elif spec.kt == 1:  # 1x1x1 downsample: a 2-D conv over the b*T frames
            call("avt_conv2d_fwd_bias", P(x), P(wf), P(y), b * T, H, W, spec.cin, spec.cout, spec.k, spec.k, spec.stride,
                 spec.pad, spec.kg, P(bias), P(res), int(relu), stream_ptr())
        else:
            call("avt_conv3d_fwd_bias", P(x), P(wf), P(y), b, T, H, W, spec.cin, spec.cout, spec.kt, spec.k, spec.k,
                 spec.stride, spec.pad_t, spec.pad, P(bias), P(res), int(relu), stream_ptr())
        ConvProfiler.end(ev, "fwd3d", 2.0 * y.numel() * spec.kt * spec.k * spec.k * spec.cin,
                         2.0 * (x.numel() + wf.numel() + y.numel() * (2 if res is not None else 1)))
        return y, Ho, Wo

    def forward_folded(self, video: torch.Tensor, store):
        """The eval-mode forward with every BatchNorm3d folded into its conv (store.folded3d: the operands of
        avt_fold_conv3d_bn_batched): im2col, the stem conv with bias + ReLU (its BN folds too: no fused max-pool
        kernel here), the max-pool when the trunk has one, then per block conv1 with bias + ReLU, the downsample with
        bias, conv2 with bias + residual + ReLU -- 1 + 20 launches (+ 1), no avt_bn_apply, no BN arithmetic, no
        weight pack, no statistics accumulator, no tape.  Returns forward()'s layer4 map."""
        video = video.contiguous().float()
        b, C, T, H, W = video.shape
        if C != 3:
            raise ValueError(f"avt: expected video [b,3,t,H,W], got {tuple(video.shape)}")
        x = torch.empty(b, T, H, W, 32, device=video.device, dtype=torch.bfloat16)
        call("avt_video_stem_im2col", P(video), P(x), b, C, T, H, W, self.stem.kt, self.stem.pad_t, stream_ptr())
        h, H, W = self._conv_bias(x, b, T, H, W, self.stem, store, True)
        del x
        if self.max_pool:  # resnet3D.py:200-201
            To, Ho, Wo = (T - 1) // 2 + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1
            hp = torch.empty(b * To, Ho, Wo, 64, device=h.device, dtype=torch.bfloat16)
            call("avt_maxpool3d_fwd", P(h), P(hp), b, T, H, W, 64, stream_ptr())
            h, T, H, W = hp, To, Ho, Wo
        for blk in self.blocks:
            h1, Ho, Wo = self._conv_bias(h, b, T, H, W, blk["conv1"], store, True)
            res = h
            if blk["down"] is not None:
                res, _, _ = self._conv_bias(h, b, T, H, W, blk["down"], store, False)
            h, _, _ = self._conv_bias(h1, b, T, Ho, Wo, blk["conv2"], store, True, res=res)
            H, W = Ho, Wo
        return h

    # ------------------------------------------------------------------ backward
    def _bn_relu(self, g, xc, stats, bn: BNSpec, store, training: bool):
        """bn -> relu backward by the train rule, or (training=False) the running-statistics one."""
        if training:
            return self._bn_relu_bwd(g, xc, stats, bn, store)
        return self._bn_eval_bwd(g, xc, stats, bn, store, mask_stats=stats)

    @staticmethod
    def _wgrad(x, gy, b, T, H, W, spec: Conv3dSpec, store):
        """dw (fp32 OIDHW view of the flat gradient) += the conv's weight gradient."""
        dw = store.grad(spec.name)
        ev = ConvProfiler.begin()
        if spec.kt == 1:  # 1x1x1 downsample: a 2-D wgrad over the b*T frames ([K][1][1][C] == OIDHW [K][C][1][1][1])
            wsb = int(query("avt_conv2d_wgrad_workspace", b * T, H, W, spec.cin, spec.cin, spec.cout, spec.k, spec.k,
                            spec.stride, spec.pad))
            ws = torch.empty(max(wsb, 16), device=x.device, dtype=torch.uint8)
            call("avt_conv2d_wgrad", P(x), P(gy), P(dw), b * T, H, W, spec.cin, spec.cin, spec.cout, spec.k, spec.k,
                 spec.stride, spec.pad, P(ws), wsb, stream_ptr())
        else:
            wsb = int(query("avt_conv3d_wgrad_workspace", b, T, H, W, spec.cin, spec.cout, spec.kt, spec.k, spec.k,
                            spec.stride, spec.pad_t, spec.pad))
            ws = torch.empty(max(wsb, 16), device=x.device, dtype=torch.uint8)
            call("avt_conv3d_wgrad", P(x), P(gy), P(dw), b, T, H, W, spec.cin, spec.cout, spec.kt, spec.k, spec.k,
                 spec.stride, spec.pad_t, spec.pad, P(ws), wsb, stream_ptr())
        ConvProfiler.end(ev, "wgrad3d", 2.0 * gy.numel() * spec.kt * spec.k * spec.k * spec.cin,
                         2.0 * (x.numel() + gy.numel()) + 8.0 * dw.numel())

    @staticmethod
    def _dgrad(gy, b, T, H, W, spec: Conv3dSpec, store, add=None):
        """Input gradient [b*T, H, W, cin] of a 3x3x3 conv (+ add, which may be the result tensor itself)."""
        wt = store.packed3d_t(spec)
        gx = torch.empty(b * T, H, W, spec.cin, device=gy.device, dtype=torch.bfloat16)
        ev = ConvProfiler.begin()
        call("avt_conv3d_dgrad", P(gy), P(wt), P(gx), P(add), b, T, H, W, spec.cin, spec.cout, spec.kt, spec.k, spec.k,
             spec.stride, spec.pad_t, spec.pad, stream_ptr())
        ConvProfiler.end(ev, "dgrad3d", 2.0 * gy.numel() * spec.kt * spec.k * spec.k * spec.cin,
                         2.0 * (gy.numel() + wt.numel() + gx.numel()))
        return gx

    def backward(self, tape, g: torch.Tensor, store, training: bool = True, gvideo=None, on_boundary=None) -> None:
        """g bf16 [b*T, h, w, 512] = d(loss)/d(layer4 map) -> the trunk's parameter gradients, accumulated into
        store.grad(name) (zeroed by the caller).  Blocks in reverse, unfused (autograd through BasicBlock.forward,
        resnet3D.py:45-61): bn2 (+ downsample.1) backward, conv2 wgrad + dgrad, bn1+relu backward, conv1 wgrad + dgrad
        with the residual gradient (identity: added in the dgrad's store; strided block: the in-place 2-D dgrad of
        the 1x1x1 downsample), then the stem's max-pool / BN+ReLU backward and its folded weight gradient.
        training=False: the tape of an eval-mode forward, every BatchNorm backward by the running-statistics rule
        (avt_bn_eval_bwd; a first block's bn2 + downsample.1 in one pass).  gvideo (fp32 [b,3,t,H,W], optional)
        receives the video's gradient (avt_video_stem_dgrad on the stem's gc0).  on_boundary(prefix + "hi") is called
        once layer4 and layer3 are done (as Trunk.backward: those gradients are final there)."""
        g = self.backward_blocks(tape, g, store, self.HI_BLOCK, len(self.blocks), training)
        if on_boundary is not None:
            on_boundary(self.prefix + "hi")
        g = self.backward_blocks(tape, g, store, 0, self.HI_BLOCK, training)
        self.backward_stem(tape, g, store, training, gvideo)

    def backward_blocks(self, tape, g: torch.Tensor, store, lo: int, hi: int, training: bool = True):
        """backward's blocks hi-1 .. lo; returns the gradient of block lo's input."""
        b = tape["b"]
        for blk, tb in zip(reversed(self.blocks[lo:hi]), reversed(tape["blocks"][lo:hi])):
            T, H, W, Ho, Wo = tb["dims"]
            gm = gcd = None
            if not training and blk["down"] is not None:  # the eval rule takes bn2 and downsample.1 in one pass
                gc2, gcd = self._bn_eval_bwd(g, tb["c2"], tb["s2"], blk["bn2"], store, y=tb["out"],
                                             second=(tb["cd"], tb["sd"], blk["bnd"]))
            else:
                gm = torch.empty_like(g)  # g * [out > 0]: shared by bn2, downsample.1 and the identity residual
                if training:
                    gc2 = self._bn_bwd(g, tb["out"], tb["c2"], tb["s2"], blk["bn2"], store, gmask_out=gm)
                else:
                    gc2 = self._bn_eval_bwd(g, tb["c2"], tb["s2"], blk["bn2"], store, y=tb["out"], gmask_out=gm)
            self._wgrad(tb["h1"], gc2, b, T, Ho, Wo, blk["conv2"], store)
            gh1 = self._dgrad(gc2, b, T, Ho, Wo, blk["conv2"], store)
            del gc2
            gc1 = self._bn_relu(gh1, tb["c1"], tb["s1"], blk["bn1"], store, training)
            del gh1
            self._wgrad(tb["x"], gc1, b, T, H, W, blk["conv1"], store)
            if blk["down"] is not None:
                if gcd is None:
                    gcd = self._bn_bwd(gm, None, tb["cd"], tb["sd"], blk["bnd"], store)
                self._wgrad(tb["x"], gcd, b, T, H, W, blk["down"], store)
                g = self._dgrad(gc1, b, T, H, W, blk["conv1"], store)
                dn = blk["down"]
                call("avt_conv2d_dgrad", P(gcd), P(store.packed3d_t(dn)), P(g), P(g), b * T, H, W, dn.cin, dn.cout,
                     dn.k, dn.k, dn.stride, dn.pad, stream_ptr())
            else:
                g = self._dgrad(gc1, b, T, H, W, blk["conv1"], store, add=gm)
        return g

    def backward_stem(self, tape, g: torch.Tensor, store, training: bool = True, gvideo=None) -> None:
        """backward's tail: the stem's max-pool / BN+ReLU backward, its folded weight gradient, the video's gradient."""
        b = tape["b"]
        T, H, W = tape["dims0"]
        if self.max_pool:  # resnet3D.py:200-201
            gp = torch.empty_like(tape["h0"])
            call("avt_maxpool3d_bwd", P(g), P(tape["h0"]), None, P(gp), b, T, H, W, 64, stream_ptr())
            g = gp
        gc0 = self._bn_relu(g, tape["c0"], tape["s0"], self.bn1, store, training)
        # the stem's weight gradient in its folded layout: a 2-D wgrad over the 32-channel im2col input, unfolded
        st, x = self.stem, tape["x"]
        Ti, Hi, Wi = tape["dims"]
        dwf = torch.zeros(st.cout, st.k, st.k, 32, device=g.device, dtype=torch.float32)
        wsb = int(query("avt_conv2d_wgrad_workspace", b * Ti, Hi, Wi, 32, 32, st.cout, st.k, st.k, st.stride, st.pad))
        ws = torch.empty(max(wsb, 16), device=g.device, dtype=torch.uint8)
        call("avt_conv2d_wgrad", P(x), P(gc0), P(dwf), b * Ti, Hi, Wi, 32, 32, st.cout, st.k, st.k, st.stride, st.pad,
             P(ws), wsb, stream_ptr())
        call("avt_stem3d_wgrad_unfold", P(dwf), P(store.grad(st.name)), st.cout, st.cin, st.kt, st.k, st.k,
             stream_ptr())
        if gvideo is not None:  # d(loss)/d(video), fp32 NCDHW
            ev = ConvProfiler.begin()
            call("avt_video_stem_dgrad", P(gc0), P(store.param(st.name)), P(store.packed3d_t(st)), P(gvideo), b, Ti, Hi,
                 Wi, stream_ptr())
            ConvProfiler.end(ev, "dgrad3d", 2.0 * gvideo.numel() * (st.kt * st.k * st.k / 4.0) * st.cout,
                             2.0 * gc0.numel() + 4.0 * gvideo.numel())


def _alloc_packs3d(engine, dev):
    """bf16 fwd operands of the R3D convs and the device table of the non-stem ones (one batched pack launch)."""
    import struct

    descs, max_k, max_row = [], 1, 1
    for spec in engine.vid.convs():
        wp = torch.empty(spec.cout, spec.kg, device=dev, dtype=torch.bfloat16)
        engine.packs3d[spec.name] = wp
        if not spec.stem:
            t = spec.kt * spec.k * spec.k
            descs.append(struct.pack("<QQiiii", engine.flat.raw(spec.name).data_ptr(), wp.data_ptr(), spec.cout,
                                     spec.cin, t, 0))
            max_k, max_row = max(max_k, spec.cout), max(max_row, spec.cin * t)
    engine._pack3d_table = desc_table(descs, "avt_pack3d_desc_bytes", dev)
    engine._pack3d_n, engine._pack3d_max = len(descs), (max_k, max_row)
    engine._pack3d_t_table = None
    if getattr(engine, "with_backward", False):  # the dgrad operands [cin][taps * cout] of the same convs
        descs, max_blocks = [], 1
        for spec in engine.vid.convs():
            if spec.stem:
                continue
            t = spec.kt * spec.k * spec.k
            wt = torch.empty(spec.cin, t * spec.cout, device=dev, dtype=torch.bfloat16)
            engine.packs3d_t[spec.name] = wt
            descs.append(struct.pack("<QQiiii", engine.flat.raw(spec.name).data_ptr(), wt.data_ptr(), spec.cout,
                                     spec.cin, t, 0))
            max_blocks = max(max_blocks, spec.cin * (spec.cout // 64))
        engine._pack3d_t_table = desc_table(descs, None, dev)  # (the record layout checked above)
        engine._pack3d_t_n, engine._pack3d_t_blocks = len(descs), max_blocks


def _pack3d(engine, stem_dgrad: bool = False):
    """vidnet weights (fp32 OIDHW, never updated by the optimizer) -> bf16 fwd operands, repacked every step so a
    load_state_dict is always picked up: the folded stem (its own layout) and one launch for all the other convs.
    stem_dgrad (a step whose video requires grad): the stem's dgrad operand too (avt_video_stem_dgrad's MFMA form)."""
    stem = engine.vid.stem
    call("avt_pack_conv3d_weight", P(engine.flat.raw(stem.name)), P(engine.packs3d[stem.name]), stem.cout, stem.cin,
         stem.kt, stem.k, stem.k, 1, stream_ptr())
    call("avt_pack_conv3d_weights_batched", P(engine._pack3d_table), engine._pack3d_n, *engine._pack3d_max,
         stream_ptr())
    if engine._pack3d_t_table is not None:  # a trainable trunk: the dgrad operands too (one more launch)
        call("avt_pack_conv3d_weights_dgrad_batched", P(engine._pack3d_t_table), engine._pack3d_t_n,
             engine._pack3d_t_blocks, stream_ptr())
        if stem_dgrad:
            if stem.name not in engine.packs3d_t:
                engine.packs3d_t[stem.name] = torch.empty(int(query("avt_video_stem_dgrad_pack_bytes")),
                                                          device=engine.flat.flat.device, dtype=torch.uint8)
            call("avt_pack_video_stem_dgrad", P(engine.flat.raw(stem.name)), P(engine.packs3d_t[stem.name]),
                 stream_ptr())


def _alloc_folds3d(engine):
    """The folded operands of the video trunk (first folded forward), kept next to packs3d: per conv the bf16 image
    of w * bn_scale (the stem in its 32-channel layout) and the fp32 bias, and the device table of one record per
    (conv, BN) pair for avt_fold_conv3d_bn_batched."""
    import struct

    flat, vid = engine.flat, engine.vid
    dev = flat.flat.device
    engine.folds3d = {}
    descs, max_k, max_row = [], 1, 1
    for spec, bn in vid.conv_bn_pairs():
        wf = torch.empty(spec.cout, spec.kg, device=dev, dtype=torch.bfloat16)
        bias = torch.empty(spec.cout, device=dev, dtype=torch.float32)
        engine.folds3d[spec.name] = (wf, bias)
        ptrs = [flat.raw(spec.name), wf, flat.raw(bn.prefix + ".weight"), flat.raw(bn.prefix + ".bias"),
                flat.rawbuf(bn.prefix + ".running_mean"), flat.rawbuf(bn.prefix + ".running_var"), bias]
        descs.append(struct.pack("<QQQQQQQiiiiiifi", *[t.data_ptr() for t in ptrs], spec.cout, spec.cin, spec.kt,
                                 spec.k, spec.k, int(spec.stem), AVEngine.BN_EPS, 0))
        max_k, max_row = max(max_k, spec.cout), max(max_row, spec.cin * spec.kt * spec.k * spec.k)
    engine._fold3d_table = desc_table(descs, "avt_fold3d_desc_bytes", dev)
    engine._fold3d_n, engine._fold3d_max = len(descs), (max_k, max_row)


def _fold3d(engine):
    """One launch: refold the video trunk's BatchNorm3d's into its convs from the flat store (current stream)."""
    call("avt_fold_conv3d_bn_batched", P(engine._fold3d_table), engine._fold3d_n, *engine._fold3d_max, stream_ptr())
    engine.fold_launches += 1


class _TubeStore(_EngineStore):
    def packed3d(self, spec: Conv3dSpec):
        return self.e.packs3d[spec.name]

    def folded3d(self, spec: Conv3dSpec):
        return self.e.folds3d[spec.name]

    def packed3d_t(self, spec: Conv3dSpec):
        return self.e.packs3d_t[spec.name]


class TubeEngine(AVEngine):
    """R3D-18 + audio ResNet-18 + HardWayAttention head on one device.  video_backward (a FullModel after
    ``enable_video_backward()``; flat's trainable segment then holds the vidnet parameters): the Conv3d dgrad operands
    are packed with the forward ones, a train-mode forward keeps the video trunk's tape, the head backward also
    produces gv, and ``backward`` runs R3DTrunk.backward on the current stream next to the audio trunk's on the second
    one."""

    def __init__(self, flat: FlatStore, video_backward: bool = False):
        self.video_backward = self.with_backward = bool(video_backward)  # (with_backward: read by _alloc_packs3d)
        self.packs3d_t: Dict[str, torch.Tensor] = {}
        super().__init__(flat, 0.65, 0.4, 0.03, True, True)  # HardWayAttention's fixed constants (model.py:41-44)
        self.store = _TubeStore(self)

    def _setup_trunks(self):
        self.aud = Trunk("audnet.", "audio")
        self.vid = R3DTrunk("vidnet.")
        self.packs3d: Dict[str, torch.Tensor] = {}
        self.folds3d = None  # folded inference operands of the video trunk (forward_folded: allocated at first use)
        self.trunks2d = [self.aud]
        self.bn_trunks = [self.aud, self.vid]

    def _alloc(self, dev):
        super()._alloc(dev)
        _alloc_packs3d(self, dev)

    def pack_weights(self):
        super().pack_weights()
        _pack3d(self)

    # ----------------------------------------------------------------------------- forward
    @staticmethod
    def _check_tube_inputs(audio: torch.Tensor, video: torch.Tensor):
        """-> (B = b*t head rows, rep: how many head rows share one audio row)."""
        if not audio.is_cuda or not video.is_cuda:
            raise RuntimeError("avt: inputs must be on the GPU (no CPU path)")
        if video.dim() != 5 or audio.dim() != 4 or audio.shape[1] != 1:
            raise ValueError(f"avt: expected audio [bt,1,F,T] and video [b,3,t,H,W], got {tuple(audio.shape)} "
                             f"and {tuple(video.shape)}")
        b, t = video.shape[0], video.shape[2]
        B = b * t
        if audio.shape[0] == B:
            rep = 1
        elif audio.shape[0] == b:
            rep = t
        else:
            raise ValueError(f"avt: audio batch {audio.shape[0]} must be b*t={B} (folded) or b={b} (per clip)")
        return B, rep

    def forward(self, audio: torch.Tensor, video: torch.Tensor, training: bool, with_ce: bool = False,
                ce_scale: float = 1.0, vision_pre=None):
        """audio: [b*t,1,F,T] (folded repeated spectrogram, model.py API) or [b,1,F,T] (one per clip,
        de-duplicated); video: [b,3,t,H,W].  Returns ({'A', 'logits'[, 'loss', 'dlogits']}, tape).  vision_pre():
        launches issued ahead of the trunks (the data-parallel step's Adam prep and gradient zeroing, train.py).
        video_backward: a train-mode tape also holds the video trunk's (tape["vid"])."""
        B, rep = self._check_tube_inputs(audio, video)
        self.pack_weights()
        if training:
            self.flat.nbt.add_(1)
        if vision_pre is not None:
            vision_pre()
        xa = self._to_nhwc(audio, 1)
        self.aud.bn_rep = rep
        try:
            a, tape_a = self.aud.forward(xa, self.store, training)
        finally:
            self.aud.bn_rep = 1
        tape_v = None
        if training and self.video_backward:
            v, tape_v = self.vid.forward(video, self.store, training, tape=True)
        else:
            v = self.vid.forward(video, self.store, training)
        out, tape = self._tube_head(a, tape_a, v, B, rep, training, with_ce, ce_scale)
        if tape is not None:
            tape["vid"] = tape_v
        return out, tape

    def forward_folded(self, audio: torch.Tensor, video: torch.Tensor):
        """forward(training=False) on the folded inference path (FullModel.enable_folded_inference): the audio trunk
        as Trunk.forward_folded (bn_rep plays no part in eval), the video trunk as R3DTrunk.forward_folded, then the
        same pool + head -- no BatchNorm launch, no per-call BN arithmetic, no weight pack.  The folded operands of
        both trunks are rebuilt (one launch per trunk) only when fold_state() has moved since they were built.
        Returns forward()'s (out, None)."""
        B, rep = self._check_tube_inputs(audio, video)
        if self.folds is None:
            self._alloc_folds()
        if self.folds3d is None:
            _alloc_folds3d(self)
        state = self.fold_state()
        if state != self._fold_key:
            self.fold_trunk(self.aud)
            _fold3d(self)
        self._fold_key = state
        a = self.aud.forward_folded(self._to_nhwc(audio, 1), self.store)
        v = self.vid.forward_folded(video, self.store)
        return self._tube_head(a, None, v, B, rep, False, False, 1.0)

    def _tube_head(self, a, tape_a, v, B, rep, training, with_ce, ce_scale):
        """AdaptiveMaxPool2d + normalize of the audio map, the hard-way head on (v, an) and the forward's tape."""
        dev = v.device
        _, h, w, C = v.shape
        Pn = h * w
        Ba = a.shape[0]
        f32 = dict(device=dev, dtype=torch.float32)
        an_a = torch.empty(Ba, C, **f32)
        amax = torch.empty(Ba, C, device=dev, dtype=torch.int32)
        anorm = torch.empty(Ba, **f32)
        call("avt_audio_pool_norm_fwd", P(a), P(an_a), P(amax), P(anorm), Ba, a.shape[1] * a.shape[2], C, stream_ptr())
        if rep > 1:
            an = torch.empty(B, C, **f32)
            call("avt_repeat_rows_f32", P(an_a), P(an), Ba, rep, C, stream_ptr())
        else:
            an = an_a
        L = B + 2
        inv = torch.empty(B, Pn, **f32)
        vsum = torch.empty(B, Pn, **f32)
        A0 = torch.empty(B, Pn, B, **f32)
        save = torch.empty(int(query("avt_hardway_save_floats", B)), **f32)
        logits = torch.empty(B, L, **f32)
        A = torch.empty(B, 1, h, w, **f32)
        Pos = torch.empty(B, 1, h, w, **f32)
        Neg = torch.empty(B, 1, h, w, **f32)
        wA = torch.empty(B, h, w, **f32)
        call("avt_hardway_fwd", P(v), P(an), B, Pn, C, self.epsilon, self.epsilon2, self.tau, 1, 1, P(inv), P(vsum),
             P(A0), P(save), P(logits), P(A), P(Pos), P(Neg), P(wA), stream_ptr())
        out = {"A": A, "logits": logits, "v": v}
        tape = None
        if training:
            tape = {"aud": tape_a, "v": v, "a": a, "an": an, "an_a": an_a, "amax": amax, "anorm": anorm, "inv": inv,
                    "A0": A0, "save": save, "B": B, "P": Pn, "C": C, "rep": rep, "Ba": Ba}
        if with_ce:
            loss = torch.empty((), **f32)
            dlogits = torch.empty(B, L, **f32) if training else None
            call("avt_hardway_ce", P(logits), B, L, ce_scale, P(loss), P(dlogits), stream_ptr())
            out["loss"] = loss
            out["dlogits"] = dlogits
        return out, tape

    # ----------------------------------------------------------------------------- backward
    def backward_order(self):
        return [self.vid, self.aud] if self.video_backward else [self.aud]

    def backward(self, tape, dlogits: Optional[torch.Tensor], gflat: torch.Tensor, on_boundary=None, dA=None):
        """Accumulate d(loss)/d(audnet params) into gflat[:n_train] (caller zeroes it).  dA (optional):
        upstream gradient of the returned A map (model.py:60).  video_backward: the vidnet parameters' too
        (_backward_e2e)."""
        if self.video_backward:
            return self._backward_e2e(tape, dlogits, gflat, on_boundary, dA)
        B, Pn, C, rep, Ba = tape["B"], tape["P"], tape["C"], tape["rep"], tape["Ba"]
        dev = tape["A0"].device
        f32 = dict(device=dev, dtype=torch.float32)
        dA0 = torch.empty(B, Pn, B, **f32)
        gan = torch.empty(B, C, **f32)
        dlogits = torch.zeros(B, B + 2, **f32) if dlogits is None else dlogits.contiguous().float()
        dA = None if dA is None else dA.contiguous().float()
        call("avt_hardway_bwd_ex", P(tape["v"]), P(tape["an"]), P(tape["inv"]), P(tape["A0"]), P(tape["save"]),
             P(dlogits), B, Pn, C, self.epsilon, self.epsilon2, self.tau, 1, 1, None, None, None, P(dA), None, None,
             P(dA0), None, None, P(gan), 0, P(self.head_ws(B, C)), stream_ptr())
        if rep > 1:
            gan_a = torch.empty(Ba, C, **f32)
            call("avt_sum_rep_rows_f32", P(gan), P(gan_a), Ba, rep, C, stream_ptr())
        else:
            gan_a = gan
        a = tape["a"]
        ga = torch.empty_like(a)
        call("avt_audio_pool_norm_bwd", P(gan_a), P(tape["an_a"]), P(tape["amax"]), P(tape["anorm"]), P(ga), Ba,
             a.shape[1] * a.shape[2], C, stream_ptr())
        self.store.grads = self.flat.grad_views(gflat)
        try:
            self.aud.backward(tape["aud"], ga, self.store, on_boundary)
            if on_boundary is not None:
                on_boundary(self.aud.prefix + "lo")
        finally:
            self.store.grads = None

    def _backward_e2e(self, tape, dlogits, gflat, on_boundary, dA):
        """backward with the video trunk attached: the head backward with gv (AVEngine.head_backward: dvh fp32
        [B][P][C], gv bf16 '(b t) h w c' -- the layout R3DTrunk.backward reads), then the two trunks' backwards, which
        share nothing but the read-only tape: the video trunk's on the current stream, the audio trunk's (the row sum
        over each clip's frames, the pool/normalise backward, Trunk.backward) on the second one, forked behind the head
        and joined before returning -- two branches, as AVEngine's.  on_boundary (the data-parallel schedule): both
        trunks' layer4+layer3, a join and on_boundary(("vidnet.hi", "audnet.hi")), then the rest of both, a join and
        on_boundary(("vidnet.lo", "audnet.lo")), on the current stream as AVEngine.backward calls it.  No atomics; each
        wgrad sums its own slabs in split order, so the gradient bits do not depend on the streams."""
        if tape.get("vid") is None:
            raise RuntimeError("avt: this tape holds no video-trunk tape (a forward of an engine without video_backward)")
        B, C, rep, Ba = tape["B"], tape["C"], tape["rep"], tape["Ba"]
        gv, gan = self.head_backward(tape, dlogits, dA=dA)
        a, aud, vid, ta, tv = tape["a"], self.aud, self.vid, tape["aud"], tape["vid"]
        hi = aud.HI_BLOCK  # (BlockGraph's: the same index in both trunks)

        def audio_hi():
            if rep > 1:
                gan_a = torch.empty(Ba, C, device=gan.device, dtype=torch.float32)
                call("avt_sum_rep_rows_f32", P(gan), P(gan_a), Ba, rep, C, stream_ptr())
            else:
                gan_a = gan
            ga = torch.empty_like(a)
            call("avt_audio_pool_norm_bwd", P(gan_a), P(tape["an_a"]), P(tape["amax"]), P(tape["anorm"]), P(ga), Ba,
                 a.shape[1] * a.shape[2], C, stream_ptr())
            return aud.backward_blocks(ta, ga, self.store, hi, len(aud.blocks))

        def audio_lo(g, pm):
            g, _ = aud.backward_blocks(ta, g, self.store, 0, hi, pm)
            aud.backward_stem(ta, g, self.store)

        self.store.grads = self.flat.grad_views(gflat)
        try:
            with self._branch():
                ga, pm = audio_hi()
                if on_boundary is None:
                    audio_lo(ga, pm)
            gv = vid.backward_blocks(tv, gv, self.store, hi, len(vid.blocks))
            if on_boundary is not None:
                self._join()
                on_boundary((vid.prefix + "hi", aud.prefix + "hi"))
                with self._branch():
                    audio_lo(ga, pm)
            gv = vid.backward_blocks(tv, gv, self.store, 0, hi)
            vid.backward_stem(tv, gv, self.store)
            self._join()
            if on_boundary is not None:
                on_boundary((vid.prefix + "lo", aud.prefix + "lo"))
        finally:
            self.store.grads = None


class R3DEngine(AVEngine):
    """The R3D-18 trunk called on its own -- ``FullModel.vidnet(video)`` or a standalone
    ``resnet3D.generate_model(18, ...)(video)`` (resnet3D.py:197-213; with or without the stem max-pool): the conv stem ..
    layer4 on libavt as inside FullModel (R3DTrunk), then AdaptiveAvgPool3d((1,1,1)) + fc on the pooled
    fp32 features.  with_backward (a standalone module after ``enable_backward()``): the dgrad operands are packed
    too, ``forward(..., tape=True)`` keeps the backward's tape and ``backward`` fills the flat gradient of every
    vidnet parameter; ``FullModel.vidnet(video)`` called on its own stays forward-only (the reference detaches the trunk,
    model.py:14; FullModel.enable_video_backward trains it from the model's loss, through TubeEngine)."""

    def __init__(self, flat: FlatStore, prefix: str, max_pool: bool = False, with_backward: bool = False):
        self._prefix = prefix
        self._max_pool = max_pool
        self.with_backward = with_backward
        self.packs3d_t: Dict[str, torch.Tensor] = {}
        super().__init__(flat)
        self.concurrent = False
        self.store = _TubeStore(self)
        self._nbt_idx = torch.tensor([i for i, n in enumerate(flat.nbt_names) if n.startswith(prefix)],
                                     device=flat.flat.device, dtype=torch.long)

    def _setup_trunks(self):
        self.vid = R3DTrunk(self._prefix, self._max_pool)
        self.packs3d: Dict[str, torch.Tensor] = {}
        self.folds3d = None  # folded inference operands of the video trunk (forward_folded: allocated at first use)
        self.trunks2d = []
        self.bn_trunks = [self.vid]

    def _alloc(self, dev):
        super()._alloc(dev)
        _alloc_packs3d(self, dev)

    def pack_weights(self, stem_dgrad: bool = False):
        _pack3d(self, stem_dgrad)

    def forward(self, video: torch.Tensor, training: bool, tape: bool = False, input_grad: bool = False):
        """video fp32 [b,3,t,H,W] -> fc logits [b, n_classes] fp32 (tape=True: (logits, tape) for ``backward``; the
        tape of a training=False forward holds the running-statistics (scale, shift, mean, invstd) and no running
        statistic is touched).  input_grad: ``backward`` will be asked for the video's gradient (the stem's dgrad
        operand is packed with the others)."""
        if not video.is_cuda:
            raise RuntimeError("avt: inputs must be on the GPU (no CPU path)")
        if video.dim() != 5:
            raise ValueError(f"avt: expected video [b,3,t,H,W], got {tuple(video.shape)}")
        self.pack_weights(stem_dgrad=tape and input_grad)
        if training and self._nbt_idx.numel():
            self.flat.nbt.index_add_(0, self._nbt_idx, torch.ones_like(self._nbt_idx))
        b = video.shape[0]
        w, bias = self.flat.raw(self._prefix + "fc.weight"), self.flat.raw(self._prefix + "fc.bias")
        if tape:
            if not self.with_backward:
                raise RuntimeError("avt: this R3D engine was built forward-only")
            v, tp = self.vid.forward(video, self.store, training, tape=True)
            feat = v.view(b, -1, v.shape[-1]).float().mean(1)
            tp.update(v_shape=tuple(v.shape), feat=feat, training=training, video_shape=tuple(video.shape),
                      stem_dgrad=input_grad)
            return torch.addmm(bias, feat, w.t()), tp
        v = self.vid.forward(video, self.store, training)  # [(b t), h, w, 512] bf16
        feat = v.view(b, -1, v.shape[-1]).float().mean(1)  # AdaptiveAvgPool3d((1,1,1)) + flatten
        return torch.addmm(bias, feat, w.t())  # nn.Linear (resnet3D.py:212)

    def forward_folded(self, video: torch.Tensor):
        """forward(training=False) on the folded inference path (resnet3D.ResNet.enable_folded_inference):
        R3DTrunk.forward_folded, then the same mean + addmm.  The folded operands are rebuilt (one launch) only
        when fold_state() has moved since they were built."""
        if not video.is_cuda:
            raise RuntimeError("avt: inputs must be on the GPU (no CPU path)")
        if video.dim() != 5:
            raise ValueError(f"avt: expected video [b,3,t,H,W], got {tuple(video.shape)}")
        if self.folds3d is None:
            _alloc_folds3d(self)
        state = self.fold_state()
        if state != self._fold_key:
            _fold3d(self)
        self._fold_key = state
        b = video.shape[0]
        w, bias = self.flat.raw(self._prefix + "fc.weight"), self.flat.raw(self._prefix + "fc.bias")
        v = self.vid.forward_folded(video, self.store)  # [(b t), h, w, 512] bf16
        feat = v.view(b, -1, v.shape[-1]).float().mean(1)  # AdaptiveAvgPool3d((1,1,1)) + flatten
        return torch.addmm(bias, feat, w.t())  # nn.Linear (resnet3D.py:212)

    def backward(self, tape, glogits: torch.Tensor, gflat: torch.Tensor, want_gvideo: bool = False):
        """d(loss)/d(logits) [b, n_classes] -> the gradient of every vidnet parameter, accumulated into the flat
        buffer gflat[:n_train] (zeroed by the caller).  The fc and AdaptiveAvgPool3d backward run in torch on the
        [b, 512] features (a few kilobytes); the rest is R3DTrunk.backward, in the mode (train / eval BatchNorm) of
        the forward that made the tape.  want_gvideo (a forward with input_grad=True): returns d(loss)/d(video),
        fp32 [b,3,t,H,W]; otherwise None."""
        gvideo = None
        if want_gvideo:
            if not tape.get("stem_dgrad"):
                raise RuntimeError("avt: the video's gradient needs a forward(..., tape=True, input_grad=True)")
            gvideo = torch.empty(tape["video_shape"], device=glogits.device, dtype=torch.float32)
        grads = self.flat.grad_views(gflat)
        glogits = glogits.contiguous().float()
        w = self.flat.raw(self._prefix + "fc.weight")
        grads[self._prefix + "fc.weight"].addmm_(glogits.t(), tape["feat"])
        grads[self._prefix + "fc.bias"].add_(glogits.sum(0))
        n, h, wd, C = tape["v_shape"]
        b = glogits.shape[0]
        per = (n // b) * h * wd  # positions the average pool spans per clip
        gfeat = torch.mm(glogits, w) / per
        g = gfeat.to(torch.bfloat16).view(b, 1, C).expand(b, per, C).contiguous().view(n, h, wd, C)
        self.store.grads = grads
        try:
            self.vid.backward(tape, g, self.store, training=tape.get("training", True), gvideo=gvideo)
        finally:
            self.store.grads = None
        return gvideo

    # ------------------------------------------------------------------ the classifier step, all on libavt
    def forward_cls(self, video: torch.Tensor, labels: torch.Tensor, training: bool = True, ce_scale: float = 1.0):
        """video fp32 [b,3,t,H,W], labels int64 [b] -> (out, tape): the trunk's taped forward, then the head on the
        device -- avt_cls_pool_fwd, avt_cls_fc_fwd, avt_softmax_ce (resnet3D.py:208-212 + nn.CrossEntropyLoss; a label
        outside [0, n_classes) is an ignored row).  out = {"loss": [1], "logits": [b, n], "dlogits": [b, n],
        "correct": int32 [1]}, device tensors, no host sync; the tape also carries what ``backward_cls`` reads.
        ``forward`` / ``backward`` (the torch head under autograd) are not involved and keep their launch sequence."""
        if not video.is_cuda or not labels.is_cuda:
            raise RuntimeError("avt: inputs must be on the GPU (no CPU path)")
        if video.dim() != 5:
            raise ValueError(f"avt: expected video [b,3,t,H,W], got {tuple(video.shape)}")
        b = video.shape[0]
        if labels.dim() != 1 or labels.shape[0] != b or labels.is_floating_point():
            raise ValueError(f"avt: expected {b} integer class labels, got {tuple(labels.shape)} {labels.dtype}")
        if not self.with_backward:
            raise RuntimeError("avt: this R3D engine was built forward-only")
        labels = labels.to(torch.long).contiguous()
        self.pack_weights()
        if training and self._nbt_idx.numel():
            self.flat.nbt.index_add_(0, self._nbt_idx, torch.ones_like(self._nbt_idx))
        w, bias = self.flat.raw(self._prefix + "fc.weight"), self.flat.raw(self._prefix + "fc.bias")
        v, tp = self.vid.forward(video, self.store, training, tape=True)  # [(b t), h, w, 512] bf16
        dev, C, n = v.device, v.shape[-1], w.shape[0]
        per = v.numel() // (b * C)  # positions the average pool spans per clip
        wsb = int(query("avt_cls_pool_ws_bytes", b, per, C))
        ws = torch.empty(max(wsb, 16), device=dev, dtype=torch.uint8)
        feat = torch.empty(b, C, device=dev, dtype=torch.float32)
        call("avt_cls_pool_fwd", P(v), P(feat), b, per, C, P(ws), wsb, stream_ptr())
        logits = torch.empty(b, n, device=dev, dtype=torch.float32)
        call("avt_cls_fc_fwd", P(feat), P(w), P(bias), P(logits), b, C, n, stream_ptr())
        loss = torch.empty(1, device=dev, dtype=torch.float32)
        dlogits = torch.empty_like(logits)
        correct = torch.empty(1, device=dev, dtype=torch.int32)
        call("avt_softmax_ce", P(logits), P(labels), b, n, ce_scale, P(loss), P(dlogits), P(correct), stream_ptr())
        tp.update(v_shape=tuple(v.shape), feat=feat, training=training, video_shape=tuple(video.shape),
                  stem_dgrad=False, dlogits=dlogits, labels=labels)
        return {"loss": loss, "logits": logits, "dlogits": dlogits, "correct": correct}, tp

    def backward_cls(self, tape, gflat: torch.Tensor) -> None:
        """The backward of ``forward_cls`` from its tape: avt_cls_fc_bwd stores the fc gradients into their slots of
        the flat buffer gflat[:n_train] and yields d(loss)/d(features), avt_cls_pool_bwd broadcasts it over the layer4
        map, R3DTrunk.backward accumulates every other gradient (gflat zeroed by the caller), in the mode (train /
        eval BatchNorm) of the forward that made the tape."""
        grads = self.flat.grad_views(gflat)
        feat, dlogits = tape["feat"], tape["dlogits"]
        w = self.flat.raw(self._prefix + "fc.weight")
        b, C = feat.shape
        n = w.shape[0]
        gfeat = torch.empty_like(feat)
        call("avt_cls_fc_bwd", P(dlogits), P(feat), P(w), P(grads[self._prefix + "fc.weight"]),
             P(grads[self._prefix + "fc.bias"]), P(gfeat), b, C, n, stream_ptr())
        g = torch.empty(tape["v_shape"], device=feat.device, dtype=torch.bfloat16)
        call("avt_cls_pool_bwd", P(gfeat), P(g), b, g.numel() // (b * C), C, stream_ptr())
        self.store.grads = grads
        try:
            self.vid.backward(tape, g, self.store, training=tape.get("training", True))
        finally:
            self.store.grads = None
