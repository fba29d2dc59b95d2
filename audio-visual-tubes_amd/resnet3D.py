"""Module shells of the R3D-18 video trunk (reference models/resnet3D.py), for FullModel.vidnet.

Same module tree, construction order and init as ``resnet3D.generate_model(18, no_max_pool=True,
n_classes=1039)`` (model.py:20; resnet3D.py:103-234), so ``torch.manual_seed(s)`` gives the
reference's weights and ``state_dict`` keys/shapes match (``vidnet.conv1.weight`` [64,3,7,7,7],
``vidnet.layerL.B.downsample.{0,1}.*``, ``vidnet.fc.*``).  Inside FullModel the compute runs in its
engine (tube.py); called on its own (``FullModel.vidnet(video)`` or a standalone
``generate_model(18, ...)``, with the stem max-pool or without) the same kernels run through tube.R3DEngine and return
the ``fc`` logits as resnet3D.ResNet.forward does (resnet3D.py:197-213).

Forward only by default: FullModel detaches the video trunk, so a call that would need gradients raises.  A
standalone module becomes trainable with ``net.enable_backward()`` (fine-tuning or pre-training the trunk the
reference loads Kinetics weights into, train_3D.py:89): every parameter then receives its gradient from libavt's
Conv3d dgrad / wgrad, BatchNorm and max-pool backward kernels (tube.R3DTrunk.backward) through one
``autograd.Function``, and ``torch.optim`` optimizers work on ``net.parameters()`` (views of the flat store).
Two further opt-ins, both off by default: ``net.enable_backward(input_grad=True)`` also returns the gradient of a video
that requires grad (``video.grad``, fp32 [b,3,t,H,W], through libavt's ``avt_video_stem_dgrad``: saliency /
attribution over a clip, adversarial or consistency training, a learnable module in front of the trunk -- it works
with every parameter frozen); ``net.enable_backward(eval_grad=True)`` differentiates an eval-mode trunk (BatchNorm
frozen on its running statistics, which are read and never updated: ``avt_bn_eval_bwd``).
Inference: ``net.enable_folded_inference()`` (opt-in) runs eval-mode calls that need no gradient with every BatchNorm3d
folded into its conv (tube.R3DEngine.forward_folded); inside a FullModel the trunk follows its parent's flag.
"""
from __future__ import annotations

import torch
from torch import nn

from .engine import FlatStore, ParentLink


def get_inplanes():
    return [64, 128, 256, 512]


def conv3x3x3(in_planes, out_planes, stride=1):
    return nn.Conv3d(in_planes, out_planes, kernel_size=3, stride=stride, padding=1, bias=False)


def conv1x1x1(in_planes, out_planes, stride=1):
    return nn.Conv3d(in_planes, out_planes, kernel_size=1, stride=stride, bias=False)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, in_planes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv3x3x3(in_planes, planes, stride)
        self.bn1 = nn.BatchNorm3d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3x3(planes, planes)
        self.bn2 = nn.BatchNorm3d(planes)
        self.downsample = downsample
        self.stride = stride


class ResNet(ParentLink, nn.Module):
    """resnet3D.ResNet(BasicBlock, layers, ...) parameter/buffer holder (shortcut 'B' only)."""

    def __init__(self, block, layers, block_inplanes, n_input_channels=3, conv1_t_size=7, conv1_t_stride=1,
                 no_max_pool=False, shortcut_type="B", widen_factor=1.0, n_classes=400):
        super().__init__()
        if shortcut_type != "B" or block is not BasicBlock or conv1_t_stride != 1:
            raise NotImplementedError("avt: R3D with BasicBlock, shortcut 'B' and temporal stride 1 only "
                                      "(the FullModel configuration, model.py:20)")
        block_inplanes = [int(x * widen_factor) for x in block_inplanes]
        self.in_planes = block_inplanes[0]
        self.no_max_pool = no_max_pool
        self.conv1 = nn.Conv3d(n_input_channels, self.in_planes, kernel_size=(conv1_t_size, 7, 7),
                               stride=(conv1_t_stride, 2, 2), padding=(conv1_t_size // 2, 3, 3), bias=False)
        self.bn1 = nn.BatchNorm3d(self.in_planes)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool3d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, block_inplanes[0], layers[0])
        self.layer2 = self._make_layer(block, block_inplanes[1], layers[1], stride=(1, 2, 2))
        self.layer3 = self._make_layer(block, block_inplanes[2], layers[2], stride=(1, 2, 2))
        self.layer4 = self._make_layer(block, block_inplanes[3], layers[3], stride=(1, 2, 2))
        self.avgpool = nn.AdaptiveAvgPool3d((1, 1, 1))
        self.fc = nn.Linear(block_inplanes[3] * block.expansion, n_classes)
        for m in self.modules():  # resnet3D.py:152-158
            if isinstance(m, nn.Conv3d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm3d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self._avt_parent = None  # (weakref to the owning FullModel, prefix) once adopted
        self._avt_engine = None
        self._own_flat = None  # a standalone module's flat storage, created at its first .to() / forward
        self._avt_backward = False  # enable_backward(): every parameter trainable (standalone modules only)
        self._avt_input_grad = False  # enable_backward(input_grad=True): a video that requires grad gets its gradient
        self._avt_eval_grad = False  # enable_backward(eval_grad=True): eval-mode (running-statistics BN) backward
        self._avt_folded = False  # enable_folded_inference(): BatchNorm3d folded into the convs for no-grad eval calls

    def enable_folded_inference(self):
        """Opt in to the folded inference forward: an eval-mode call that needs no gradient (under
        ``torch.no_grad()``, or with nothing requiring grad) runs with every BatchNorm3d folded into its conv --
        im2col, 20 conv launches with bias / residual / ReLU epilogues (+ the max-pool), no BatchNorm pass, no
        per-call weight pack (tube.R3DEngine.forward_folded) -- then the same pooling and ``fc``.  The folded weights
        are rebuilt, one launch, whenever a parameter or BN buffer has changed since the last fold.  Train mode and
        calls that take the autograd path (``enable_backward(eval_grad=True)``) run exactly as before, as does a
        trunk that never calls this.  A trunk owned by a FullModel follows its parent's flag
        (``FullModel.enable_folded_inference``).  Idempotent; returns self."""
        self._avt_folded = True
        return self

    def invalidate_folded(self):
        """Force the next folded forward to refold (after a write torch cannot see, e.g. through ``tensor.data``)."""
        if self._avt_engine is not None:
            self._avt_engine._fold_key = None
        return self

    def _folded(self) -> bool:
        return bool(getattr(self._resolve()[0] or self, "_avt_folded", False))

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None  # built before the block, as resnet3D.py:169-184 (RNG order)
        if stride != 1 or self.in_planes != planes * block.expansion:
            downsample = nn.Sequential(conv1x1x1(self.in_planes, planes * block.expansion, stride),
                                       nn.BatchNorm3d(planes * block.expansion))
        layers = [block(in_planes=self.in_planes, planes=planes, stride=stride, downsample=downsample)]
        self.in_planes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.in_planes, planes))
        return nn.Sequential(*layers)

    def _flat_store(self):
        if self._own_flat is None:
            # nothing of the video trunk is trained unless enable_backward() was called (then: every parameter)
            self._own_flat = FlatStore(self, (lambda n: True) if self._avt_backward else (lambda n: False))
        return self._own_flat

    def enable_backward(self, input_grad: bool = False, eval_grad: bool = False):
        """Make this standalone trunk trainable: its flat store is rebuilt with every parameter in the trainable
        segment, and grad-mode calls in train mode go through the backward kernels.  input_grad=True: a video that
        requires grad also receives its gradient (fp32, the video's layout; one that does not costs nothing more).
        eval_grad=True: grad-mode calls of an eval-mode trunk are differentiated too, BatchNorm by its
        running-statistics rule (no running statistic or num_batches_tracked changes).  A later call can only widen
        the opt-in, and rebuilds nothing once the trunk is trainable.  Raises on a trunk adopted by a FullModel (the
        reference detaches that trunk, model.py:14; ``FullModel.enable_video_backward()`` is the opt-in that trains
        it, from the model's loss)."""
        if self._avt_parent is not None:
            raise RuntimeError("avt: enable_backward() is for a standalone R3D trunk; to train FullModel.vidnet end to "
                               "end call FullModel.enable_video_backward() on the owning model (the trunk's gradients "
                               "then come from the model's loss)")
        if not self._avt_backward:
            self._avt_backward = True
            if self._own_flat is not None:  # rebuild from the current parameter values (and device)
                self._own_flat = FlatStore(self, lambda n: True)
            self._avt_engine = None
        self._avt_input_grad = self._avt_input_grad or bool(input_grad)
        self._avt_eval_grad = self._avt_eval_grad or bool(eval_grad)
        return self

    def forward(self, x):
        """resnet3D.ResNet.forward (resnet3D.py:197-213): x fp32 [b,3,t,H,W] -> fc logits [b, n_classes]."""
        from .tube import R3DEngine

        need_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if need_grad and x.requires_grad and not self._avt_input_grad:
            raise NotImplementedError("avt: no input gradient is computed for the video of the R3D trunk; pass a video "
                                      "tensor that does not require grad (a standalone trunk computes it after "
                                      "net.enable_backward(input_grad=True))")
        if need_grad and not (self._avt_backward and self._avt_parent is None):
            raise NotImplementedError("avt: the R3D trunk called on its own is forward-only inside a FullModel (the "
                                      "model trains it from its loss after FullModel.enable_video_backward()); call "
                                      "it under torch.no_grad() or with requires_grad_(False) parameters.  A "
                                      "standalone trunk becomes trainable after net.enable_backward().")
        if need_grad and not self.training and not self._avt_eval_grad:
            raise NotImplementedError("avt: gradients through an eval-mode trunk are not computed (train-mode "
                                      "BatchNorm only; a standalone trunk computes them after "
                                      "net.enable_backward(eval_grad=True))")
        if need_grad:
            flat = self._flat_store()
            if self._avt_engine is None or self._avt_engine.flat is not flat or not self._avt_engine.with_backward:
                self._avt_engine = R3DEngine(flat, "", max_pool=not self.no_max_pool, with_backward=True)
            named = dict(self.named_parameters())
            names = [n for n in flat.pnames if named[n].requires_grad]
            return _R3DFunction.apply(self._avt_engine, names, self.training, x, *[named[n] for n in names])
        _, prefix, flat = self._resolve()
        if self._avt_engine is None or self._avt_engine.flat is not flat:
            self._avt_engine = R3DEngine(flat, prefix, max_pool=not self.no_max_pool)
        if not self.training and self._folded():
            return self._avt_engine.forward_folded(x)
        return self._avt_engine.forward(x, self.training)


class _R3DFunction(torch.autograd.Function):
    """Bridge of a trainable standalone trunk into autograd (as model._TrunkFunction): forward keeps the engine's
    tape, backward returns the per-parameter views of one flat gradient buffer (None for a parameter that is not an
    input: one with requires_grad False) and, for a video that requires grad, its gradient."""

    @staticmethod
    def forward(ctx, engine, names, training, x, *params):
        want_gx = ctx.needs_input_grad[3]
        out, tape = engine.forward(x.detach(), training, tape=True, input_grad=want_gx)
        ctx.engine, ctx.tape, ctx.names, ctx.want_gx, ctx.x_dtype = engine, tape, names, want_gx, x.dtype
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None, None, None, None) + (None,) * len(ctx.names)
        if ctx.tape is None:
            raise RuntimeError("avt: second backward through a trunk forward")
        flat = ctx.engine.flat
        gflat = torch.zeros(flat.n_train, device=g.device, dtype=torch.float32)
        gx = ctx.engine.backward(ctx.tape, g, gflat, want_gvideo=ctx.want_gx)
        ctx.tape = None
        views = flat.param_grad_views(gflat)
        if gx is not None and gx.dtype != ctx.x_dtype:
            gx = gx.to(ctx.x_dtype)
        return (None, None, None, gx) + tuple(views[n] for n in ctx.names)


def generate_model(model_depth, **kwargs):
    if model_depth != 18:
        raise NotImplementedError("avt: only the R3D-18 used by FullModel (model.py:20) is built")
    return ResNet(BasicBlock, [2, 2, 2, 2], get_inplanes(), **kwargs)
