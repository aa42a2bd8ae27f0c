"""Train-mode batch normalisation of the fine-tune phase on the GPU, with the ReLU and the residual add that follow it fused in.

The reference's trainers call `self.model.train()` (reid/trainers.py:21,128,212), so the 53 `BatchNorm2d` layers of ResNet-50 and
`feat_bn` (`BatchNorm1d`, reid/models/resnet.py:65) run on batch statistics, forward and backward.  Here that is four entry points of
csrc/batchnorm.hip (`ssg_bn_stats_f32`, `ssg_bn_apply_f32`, `ssg_bn_backward_reduce_f32`, `ssg_bn_backward_apply_f32`): float32
tensors in and out, channel sums and the per-element arithmetic in float64, every reduction in a fixed order (the same call gives the
same bits), no host read -- also none for the cumulative average, whose factor the kernel takes from `num_batches_tracked` itself.

    y = batch_norm_train(x, weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps, relu=False, residual=None)

is `F.batch_norm(training=True)`, then `+ residual`, then `relu`, as one differentiable function: a forward is two passes over x and
one store, a backward two passes; only x and y are saved (the ReLU mask is read from y).  `BatchNorm2d` / `BatchNorm1d` are the torch
modules with that forward in train mode, `use_device_batchnorm(model)` swaps them into a torch model that is already built.

There is no CPU fallback: without a GPU the train-mode forward raises SSGError (eval mode is torch's own forward)."""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, _train
from ._lib import check, ptr, stream

__all__ = ["batch_norm_train", "BatchNorm1d", "BatchNorm2d", "use_device_batchnorm", "FUSE_DEFAULT"]

# `use_device_batchnorm(model)` without `fuse=`: the fused block forward is the default only where it measured faster than the plain
# swap by more than the spread of the repeated medians (profiles/batchnorm_times.txt, tools/time_batchnorm.py)
FUSE_DEFAULT = False


def _layout(t):
    """-> (tensor in a layout the kernels take, channels_last flag): NCHW contiguous as it is, torch's channels_last as it is, anything
    else made contiguous first, as torch does"""
    if t.is_contiguous():
        return t, 0
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
        return t, 1
    return t.contiguous(), 0


def _like(t, channels_last):
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t.contiguous()


class _Running(object):
    """the buffers a forward updates in place (not seen by autograd: they are no inputs of the graph)"""
    __slots__ = ("mean", "var", "nbt", "momentum")

    def __init__(self, mean, var, nbt, momentum):
        self.mean, self.var, self.nbt, self.momentum = mean, var, nbt, momentum


def _on(t, dev, dtype):
    """t on `dev` as `dtype` (the tensor itself when it is already there)"""
    return t if (t.device == dev and t.dtype == dtype) else t.detach().to(dev, dtype)


class _BatchNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, running, eps, relu):
        dev = _train.device("batchnorm")
        L = _lib.lib()
        xd, cl = _layout(x.detach().to(dev, torch.float32))
        N, C = xd.shape[0], xd.shape[1]
        HW = xd.numel() // (N * C)
        w = weight.detach().to(dev, torch.float32).contiguous()
        b = bias.detach().to(dev, torch.float32).contiguous()
        r = None if residual is None else _like(residual.detach().to(dev, torch.float32), cl)
        nws = L.ssg_bn_workspace_bytes(N, C, HW, cl)
        if nws == 0:
            raise ValueError("batch_norm_train: %s" % L.ssg_last_error().decode("utf-8", "replace"))
        ws = torch.empty(nws // 8, dtype=torch.float64, device=dev)
        stat = torch.empty((3, C), dtype=torch.float64, device=dev)
        rm = rv = nbt = None
        if running.mean is not None:
            rm, rv = _on(running.mean, dev, torch.float32), _on(running.var, dev, torch.float32)
            if not (rm.is_contiguous() and rv.is_contiguous()):
                raise ValueError("batch_norm_train: running_mean / running_var must be contiguous")
        if running.nbt is not None:
            running.nbt.add_(1)                       # as nn.BatchNorm does before the statistics; the kernel reads the new count
            nbt = _on(running.nbt, dev, torch.int64)
        momentum = -1.0 if running.momentum is None else float(running.momentum)
        if momentum < 0.0 and nbt is None:
            raise ValueError("batch_norm_train: momentum=None (cumulative average) needs num_batches_tracked")
        check(L.ssg_bn_stats_f32(ptr(xd), N, C, HW, cl, float(eps), momentum, ptr(nbt), ptr(rm), ptr(rv), ptr(stat), ptr(ws), nws, stream()),
              "ssg_bn_stats_f32")
        if rm is not None and rm is not running.mean:
            running.mean.copy_(rm)
            running.var.copy_(rv)
        y = torch.empty_like(xd)                      # preserve_format: the strides of xd
        check(L.ssg_bn_apply_f32(ptr(xd), ptr(stat), ptr(w), ptr(b), ptr(r), int(bool(relu)), N, C, HW, cl, ptr(y), stream()), "ssg_bn_apply_f32")
        ctx.save_for_backward(xd, y if relu else None, w, stat)
        ctx.geom = (N, C, HW, cl, nws)
        ctx.src = _train.src(x, weight, bias, residual)
        return y

    @staticmethod
    @once_differentiable                              # a double backward raises
    def backward(ctx, gy):
        xd, y, w, stat = ctx.saved_tensors
        N, C, HW, cl, nws = ctx.geom
        dev = xd.device
        L = _lib.lib()
        g = _like(gy.to(dev, torch.float32), cl)
        ws = torch.empty(nws // 8, dtype=torch.float64, device=dev)
        coef = torch.empty((2, C), dtype=torch.float64, device=dev)
        dw = torch.empty(C, dtype=torch.float32, device=dev)
        db = torch.empty(C, dtype=torch.float32, device=dev)
        check(L.ssg_bn_backward_reduce_f32(ptr(g), ptr(xd), ptr(y), ptr(stat), N, C, HW, cl, ptr(coef), ptr(dw), ptr(db), ptr(ws), nws, stream()),
              "ssg_bn_backward_reduce_f32")
        sx, sw, sb, sr = ctx.src
        need_x, need_r = ctx.needs_input_grad[0], sr is not None and ctx.needs_input_grad[3]
        dx = dr = None
        if need_x or need_r:
            dx = torch.empty_like(xd)
            dr = torch.empty_like(xd) if need_r else None
            check(L.ssg_bn_backward_apply_f32(ptr(g), ptr(xd), ptr(y), ptr(stat), ptr(w), ptr(coef), N, C, HW, cl, ptr(dx), ptr(dr), stream()),
                  "ssg_bn_backward_apply_f32")
        return (_train.back(dx if need_x else None, sx), _train.back(dw, sw), _train.back(db, sb), _train.back(dr, sr), None, None, None)


def _check_train_input(x, weight):
    if x.dim() < 2:
        raise ValueError("batch_norm_train: input must be [N, C, ...] (got %r)" % (tuple(x.shape),))
    if x.shape[1] != weight.shape[0]:
        raise ValueError("batch_norm_train: %d channels, weight has %d" % (x.shape[1], weight.shape[0]))
    n = x.numel() // x.shape[1] if x.shape[1] else 0
    if n <= 1:          # torch.nn.functional._verify_batch_size
        raise ValueError("Expected more than 1 value per channel when training, got input size {}".format(x.size()))


def batch_norm_train(x, weight, bias, running_mean, running_var, num_batches_tracked=None, momentum=0.1, eps=1e-5, relu=False, residual=None):
    """`F.batch_norm(x, running_mean, running_var, weight, bias, training=True, momentum, eps)`, then `+ residual` (same shape as x) when
    given, then `relu` when asked, in one differentiable function on the current GPU: y float32 [same shape and memory format as x].
    Gradients go to x, weight, bias and residual, in their dtype and on their device; a double backward raises.

    running_mean / running_var (both or neither) are updated in place; the running variance takes the unbiased n / (n - 1) form.
    num_batches_tracked, when given, is incremented first, as nn.BatchNorm does; momentum=None is the cumulative average
    1 / num_batches_tracked (read on the device: no synchronisation).  x: [N, C], [N, C, L] or [N, C, H, W], contiguous or
    channels_last (anything else is made contiguous first)."""
    x = torch.as_tensor(x)
    _check_train_input(x, weight)
    if residual is not None and tuple(residual.shape) != tuple(x.shape):
        raise ValueError("batch_norm_train: residual %r does not match the input %r" % (tuple(residual.shape), tuple(x.shape)))
    if (running_mean is None) != (running_var is None):
        raise ValueError("batch_norm_train: running_mean and running_var go together")
    return _BatchNormFn.apply(x, weight, bias, residual, _Running(running_mean, running_var, num_batches_tracked, momentum), float(eps), bool(relu))


class _DeviceBatchNorm(object):
    """forward of the device modules (in front of nn.BatchNorm1d / nn.BatchNorm2d in the MRO)"""

    def _ssg_init(self, relu):
        if not (self.affine and self.track_running_stats):
            raise ValueError("the device batch norm is affine and tracks running statistics (use torch's module otherwise)")
        self.relu = bool(relu)

    def forward(self, input, residual=None):
        if not self.training:                         # torch's own forward: the bits of eval mode are unchanged
            y = super(_DeviceBatchNorm, self).forward(input)
            if residual is not None:
                y = y + residual
            return torch.relu(y) if self.relu else y
        self._check_input_dim(input)
        return batch_norm_train(input, self.weight, self.bias, self.running_mean, self.running_var, self.num_batches_tracked, self.momentum,
                                self.eps, self.relu, residual)

    def extra_repr(self):
        return super(_DeviceBatchNorm, self).extra_repr() + (", relu=True" if self.relu else "")


class BatchNorm2d(_DeviceBatchNorm, nn.BatchNorm2d):
    """nn.BatchNorm2d (same parameters, buffers and state-dict keys) whose train-mode forward runs on the HIP kernels.  relu=True
    applies a ReLU to the output; forward(input, residual=None) adds `residual` before it."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, relu=False, **kw):
        super(BatchNorm2d, self).__init__(num_features, eps, momentum, affine, track_running_stats, **kw)
        self._ssg_init(relu)


class BatchNorm1d(_DeviceBatchNorm, nn.BatchNorm1d):
    """nn.BatchNorm1d likewise ([B, C] or [B, C, L])."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, relu=False, **kw):
        super(BatchNorm1d, self).__init__(num_features, eps, momentum, affine, track_running_stats, **kw)
        self._ssg_init(relu)


def _swap(old):
    """the device module in place of the plain `old`, holding the same Parameter and buffer objects; None when `old` is not affine
    or does not track running statistics"""
    if not (old.affine and old.track_running_stats):
        return None
    cls = BatchNorm2d if isinstance(old, nn.BatchNorm2d) else BatchNorm1d
    return _train.adopt(cls(old.num_features, old.eps, old.momentum), old, ("weight", "bias"), ("running_mean", "running_var", "num_batches_tracked"))


def _fused_bottleneck_forward(self, x):
    """Bottleneck.forward (reid/models/base.py:73-93) with bn1 / bn2 carrying their ReLU and bn3 the residual add and the last ReLU"""
    residual = x if self.downsample is None else self.downsample(x)
    out = self.bn1(self.conv1(x))
    out = self.bn2(self.conv2(out))
    return self.bn3(self.conv3(out), residual)


def _fused_basicblock_forward(self, x):
    """BasicBlock.forward (reid/models/base.py:38-54) likewise"""
    residual = x if self.downsample is None else self.downsample(x)
    out = self.bn1(self.conv1(x))
    return self.bn2(self.conv2(out), residual)


_FUSED_CLASSES = {}


def _block_kind(m):
    """'bottleneck' / 'basic' for a module with the attribute shape of torchvision's (and reid/models/base.py's) blocks, else None"""
    sub = m._modules
    if type(m) in _FUSED_CLASSES.values():
        return None                                    # already fused
    if not all(k in sub for k in ("conv1", "bn1", "conv2", "bn2", "relu")) or not isinstance(sub["relu"], nn.ReLU):
        return None
    if not hasattr(m, "downsample") or not (m.downsample is None or isinstance(m.downsample, nn.Module)):
        return None                                    # (downsample=None is a plain attribute, not an entry of _modules)
    has3 = "conv3" in sub and "bn3" in sub
    if ("conv3" in sub) != ("bn3" in sub):
        return None
    names = ("bn1", "bn2", "bn3") if has3 else ("bn1", "bn2")
    if not all(isinstance(sub[k], BatchNorm2d) for k in names):
        return None
    if set(sub) - {"conv1", "bn1", "conv2", "bn2", "conv3", "bn3", "relu", "downsample"}:
        return None                                    # something else lives in the block: its forward is not the one restated here
    return "bottleneck" if has3 else "basic"


def _fuse_block(m, kind):
    for k in (("bn1", "bn2", "bn3") if kind == "bottleneck" else ("bn1", "bn2")):
        m._modules[k].relu = True
    cls = type(m)
    if cls not in _FUSED_CLASSES:                      # a subclass, not an instance attribute: nn.DataParallel's replicas keep it
        fwd = _fused_bottleneck_forward if kind == "bottleneck" else _fused_basicblock_forward
        _FUSED_CLASSES[cls] = type("Fused" + cls.__name__, (cls,), {"forward": fwd, "__module__": cls.__module__})
    m.__class__ = _FUSED_CLASSES[cls]


def _is_stem_host(m):
    """a module with the attribute shape of torchvision's ResNet: conv1, bn1, relu, maxpool in this order, then layer1"""
    names = list(m._modules)
    return (names[:4] == ["conv1", "bn1", "relu", "maxpool"] and "layer1" in m._modules and isinstance(m._modules["relu"], nn.ReLU)
            and isinstance(m._modules["bn1"], BatchNorm2d))


def use_device_batchnorm(model, fuse=None):
    """Replace every affine `nn.BatchNorm1d` / `nn.BatchNorm2d` that tracks running statistics in `model` (also under nn.DataParallel:
    the walk goes through `.module`) by the device module.  The Parameter and buffer objects are kept, so optimiser groups built before
    the call and the state-dict keys stay valid.  The qualified names of the batch-norm modules left alone (affine=False,
    track_running_stats=False, other subclasses of _BatchNorm) are listed in `model._ssg_bn_skipped`.

    fuse=True also gives every block with the attribute shape of torchvision's `Bottleneck` / `BasicBlock` (conv1, bn1, conv2, bn2[,
    conv3, bn3], relu, downsample) a forward in which bn1 / bn2 carry their ReLU and the last batch norm carries the residual add and
    the last ReLU, and lets the stem's `bn1` absorb the `relu` that follows it (which becomes nn.Identity: the module names a loop over
    `base._modules` sees are unchanged).  Blocks of any other shape keep their forward and get the plain swap.  fuse=None: FUSE_DEFAULT.
    Returns the model."""
    fuse = FUSE_DEFAULT if fuse is None else bool(fuse)

    def fuse_one(m):
        kind = _block_kind(m)
        if kind:
            _fuse_block(m, kind)
        elif _is_stem_host(m):
            m._modules["bn1"].relu = True
            m._modules["relu"] = nn.Identity()

    return _train.swap_modules(model, "_ssg_bn_skipped", nn.modules.batchnorm._BatchNorm, (nn.BatchNorm1d, nn.BatchNorm2d),
                               lambda m: isinstance(m, _DeviceBatchNorm), _swap, fuse_one if fuse else None)
