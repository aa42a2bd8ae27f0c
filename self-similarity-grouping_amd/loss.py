"""Classification losses of the fine-tune phase on the GPU (csrc/softmax_ce.hip): the reference's FocalLoss (reid/loss/triplet.py:79-106),
WeightCE (reid/loss/weight_cross_entropy.py), OIMLoss (reid/loss/oim.py), the nn.CrossEntropyLoss of reid/eug.py:132, and `accuracy`
(reid/evaluation_metrics/classification.py).

All four criteria are row-wise log-softmax cross-entropy over logits [B, C] with a per-row factor:

    lse_i = logsumexp(x_i), logpt_i = x[i][t_i] - lse_i, s_i = row_w_i * class_w[t_i] * (1 - exp(logpt_i))^gamma, loss_i = -s_i * logpt_i
    dx[i][j] = g_i * r * s_i * (softmax(x_i)[j] - [j == t_i])          the factor is a constant of the backward, as in the reference

in float64 rounded once, with no float atomics, reductions cut by the shape alone, no host read and no synchronisation, so with the
other train-mode pieces a whole training step gives the same bits run to run.

    cross_entropy_train(input, target, weight, row_weight, gamma, reduction, ignore_index)     the one autograd function
    CrossEntropyLoss      nn.CrossEntropyLoss whose forward is that function (isinstance checks of the trainers keep holding)
    FocalLoss, WeightCE   the reference's classes; FocalLoss's constructor works under Python 3
    oim, OIMLoss          the lookup-table logits (ssg_linear_fwd_f32 / ssg_linear_dgrad_f32) and the table update in the backward
    accuracy              top-k precision as one-element device tensors; a tie goes to the lower index

A target outside [0, C) that is not ignore_index cannot be refused without a host read: its row, the batch loss and its row of the
gradient are NaN (the TripletLoss convention of INTEGRATION.md section 4).  There is no CPU fallback: without a GPU the forward raises
SSGError."""
import ctypes

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, _train
from ._lib import check, ptr, stream
from .head import linear_unsupported_reason

__all__ = ["cross_entropy_train", "CrossEntropyLoss", "FocalLoss", "WeightCE", "oim", "OIMLoss", "accuracy"]

# the reduction codes of ssg_softmax_ce_fwd_f32; 'mean' is torch's rule (the weighted mean over the rows that are not ignored),
# 'batch_mean' divides by B whatever the weights (FocalLoss's loss.mean(), WeightCE's loss / B)
REDUCTIONS = {"none": 0, "sum": 1, "batch_mean": 2, "mean": 3}
NO_IGNORE = -(1 << 62)                                # FocalLoss and WeightCE ignore no row: every target outside [0, C) gives NaN


def _rows(x):
    """x [B, C] as the kernels read it, and its row stride: a view whose rows are dense is used where it lies (a column slice too)"""
    if (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x, (max(x.stride(0), x.shape[1]) if x.shape[0] > 1 else x.shape[1])


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, weight, row_weight, gamma, reduction, ignore_index):
        dev = _train.device("loss")
        xd, ldx = _rows(x.detach().to(dev, torch.float32))
        t = target.detach().to(dev, torch.int64).contiguous()
        cw = None if weight is None else weight.detach().to(dev, torch.float32).contiguous()
        rw = None if row_weight is None else row_weight.detach().to(dev, torch.float32).contiguous()
        B, C = xd.shape
        keep = torch.empty((2 * B + 1,), dtype=torch.float64, device=dev)      # lse [B], s [B], r
        lse, s, r = keep[:B], keep[B:2 * B], keep[2 * B:]
        code = REDUCTIONS[reduction]
        out = torch.empty((B,) if code == 0 else (), dtype=torch.float32, device=dev)
        check(_lib.lib().ssg_softmax_ce_fwd_f32(ptr(xd), ldx, ptr(t), ignore_index, ptr(rw), ptr(cw), gamma, code, B, C, ptr(lse), ptr(s), ptr(r),
                                                ptr(out) if code == 0 else None, None if code == 0 else ptr(out), stream()), "ssg_softmax_ce_fwd_f32")
        ctx.save_for_backward(xd, t, keep)
        ctx.geom = (ldx, ignore_index, code)
        ctx.src = _train.src(x)
        return out

    @staticmethod
    @once_differentiable                              # a double backward raises
    def backward(ctx, gy):
        xd, t, keep = ctx.saved_tensors
        ldx, ignore_index, code = ctx.geom
        B, C = xd.shape
        g = gy.to(xd.device, torch.float32).contiguous()
        dx = torch.empty((B, C), dtype=torch.float32, device=xd.device)
        check(_lib.lib().ssg_softmax_ce_bwd_f32(ptr(xd), ldx, ptr(t), ignore_index, ptr(keep[:B]), ptr(keep[B:2 * B]), ptr(keep[2 * B:]), ptr(g),
                                                1 if code == 0 else 0, ptr(dx), C, B, C, stream()), "ssg_softmax_ce_bwd_f32")
        return _train.back(dx, ctx.src[0]), None, None, None, None, None, None


def cross_entropy_train(input, target, weight=None, row_weight=None, gamma=0.0, reduction="mean", ignore_index=-100):
    """Softmax cross-entropy with a per-row factor as one differentiable function on the current GPU.  input [B, C] float32 (rows
    dense; a column slice of a wider matrix is read where it lies), target [B] int64, weight [C] (per class) and row_weight [B] float32
    or None, gamma >= 0 the focal exponent (0: the plain loss).  reduction: 'mean' is torch's rule -- sum of w_i ce_i over the sum of
    w_i = row_weight_i * weight[t_i] over the rows that are not ignored -- 'batch_mean' divides by B, 'sum', 'none' ([B] losses).  Rows
    whose target is ignore_index count nowhere and get a zero gradient; a target outside [0, C) gives NaN in its row, in the batch loss
    and in its gradient row.  The weights get no gradient: one that requires grad raises ValueError, as does any other broken rule; a
    double backward raises.  No host read, no synchronisation."""
    why = None
    if input.dim() != 2 or target.dim() != 1:
        why = "input must be [B, C] and target [B] (got %r, %r)" % (tuple(input.shape), tuple(target.shape))
    elif input.shape[0] < 1 or input.shape[1] < 1:
        why = "B >= 1 and C >= 1 are required: the input is empty %r" % (tuple(input.shape),)
    elif target.shape[0] != input.shape[0]:
        why = "input has %d rows, target %d" % (input.shape[0], target.shape[0])
    elif input.dtype != torch.float32:
        why = "input must be float32 (got %s)" % input.dtype
    elif target.dtype != torch.int64:
        why = "target must be int64 class indices (got %s)" % target.dtype
    elif reduction not in REDUCTIONS:
        why = "reduction must be one of %s (got %r)" % (", ".join(repr(k) for k in REDUCTIONS), reduction)
    elif not (float(gamma) >= 0.0) or float(gamma) == float("inf"):
        why = "gamma must be finite and not negative (got %r)" % (gamma,)
    for name, w, n in (("weight", weight, input.shape[-1] if input.dim() else 0), ("row_weight", row_weight, input.shape[0] if input.dim() else 0)):
        if why is None and w is not None:
            if tuple(w.shape) != (n,):
                why = "%s must have %d entries (got %r)" % (name, n, tuple(w.shape))
            elif w.dtype != torch.float32:
                why = "%s must be float32 (got %s)" % (name, w.dtype)
            elif w.requires_grad:
                why = "%s requires grad, and the weights get no gradient here: detach it" % name
    _train.refuse("cross_entropy_train", why)
    return _CrossEntropyFn.apply(input, target, weight, row_weight, float(gamma), reduction, int(ignore_index))


class CrossEntropyLoss(nn.CrossEntropyLoss):
    """nn.CrossEntropyLoss (same constructor, `weight` buffer and attributes; the legacy size_average / reduce are mapped as torch
    maps them) whose forward runs `cross_entropy_train`.  Class-index targets only: label_smoothing != 0 and probability targets raise
    ValueError."""

    def __init__(self, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean", label_smoothing=0.0):
        _train.refuse("ssg_amd.CrossEntropyLoss", None if label_smoothing == 0 else "label_smoothing must be 0 (got %r)" % (label_smoothing,))
        super(CrossEntropyLoss, self).__init__(weight, size_average, ignore_index, reduce, reduction, 0.0)
        _train.refuse("ssg_amd.CrossEntropyLoss", None if self.reduction in ("mean", "sum", "none") else
                      "reduction must be 'mean', 'sum' or 'none' (got %r)" % (self.reduction,))

    def forward(self, input, target):
        if target.is_floating_point() or target.dim() == input.dim():
            raise ValueError("ssg_amd.CrossEntropyLoss: class-index targets [B] only, no class probabilities (got %s %r)" % (target.dtype, tuple(target.shape)))
        w = None if self.weight is None else self.weight.detach()
        return cross_entropy_train(input, target, weight=w, reduction=self.reduction, ignore_index=self.ignore_index)


class FocalLoss(nn.Module):
    """reid/loss/triplet.py:79-106 with a constructor that works under Python 3: loss_i = -alpha[t_i] (1 - pt_i)^gamma log pt_i, the
    mean over the rows (size_average) or their sum; pt is detached, as in the reference.  A float or int alpha becomes [alpha, 1 - alpha],
    a list becomes a tensor; alpha must have exactly C entries (the reference's gather on a shorter table can only be checked with a host
    read).  `epoch` is ignored, as in the reference."""

    def __init__(self, gamma=2.0, alpha=None, size_average=True):
        super(FocalLoss, self).__init__()
        self.gamma = gamma
        self.alpha = alpha
        if isinstance(alpha, (float, int)) and not isinstance(alpha, bool):
            self.alpha = torch.Tensor([alpha, 1 - alpha])
        if isinstance(alpha, list):
            self.alpha = torch.Tensor(alpha)
        self.size_average = size_average

    def forward(self, input, target, epoch=None):
        if input.dim() > 2:
            input = input.view(input.size(0), input.size(1), -1)         # N,C,H,W => N,C,H*W
            input = input.transpose(1, 2)                                # N,C,H*W => N,H*W,C
            input = input.contiguous().view(-1, input.size(2))           # N,H*W,C => N*H*W,C
        target = target.view(-1)
        if self.alpha is not None:
            if self.alpha.dim() != 1 or self.alpha.shape[0] != input.shape[-1]:
                raise ValueError("ssg_amd.FocalLoss: alpha must have exactly C = %d entries (got %r)" % (input.shape[-1], tuple(self.alpha.shape)))
            if self.alpha.device != input.device or self.alpha.dtype != torch.float32:
                self.alpha = self.alpha.detach().to(input.device, torch.float32)
        return cross_entropy_train(input, target, weight=self.alpha, gamma=self.gamma, reduction="batch_mean" if self.size_average else "sum",
                                   ignore_index=NO_IGNORE)


class WeightCE(nn.Module):
    """reid/loss/weight_cross_entropy.py:17-23: sum_i w_i CE_i / B, in one call where the reference makes B.  w gets no gradient."""

    def __init__(self, margin=0, num_instances=0, use_semi=True):
        super(WeightCE, self).__init__()
        self.margin = margin
        self.use_semi = use_semi

    def forward(self, inputs, targets, w):
        if w.dim() != 1 or inputs.dim() != 2 or inputs.size(0) != w.size(0):
            raise ValueError("ssg_amd.WeightCE: inputs [B, C] and w [B] are required (got %r, %r)" % (tuple(inputs.shape), tuple(w.shape)))
        return cross_entropy_train(inputs, targets, row_weight=w.detach().to(torch.float32), reduction="batch_mean", ignore_index=NO_IGNORE)


class _OIMFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inputs, targets, lut, momentum, anchor):
        dev = _train.device("loss")
        xd = inputs.detach().to(dev, torch.float32).contiguous()
        t = targets.detach().to(dev, torch.int64).contiguous()
        (B, F), C = xd.shape, lut.shape[0]
        y = torch.empty((B, C), dtype=torch.float32, device=dev)
        check(_lib.lib().ssg_linear_fwd_f32(ptr(xd), ptr(lut), None, ptr(y), B, F, C, stream()), "ssg_linear_fwd_f32")
        ctx.save_for_backward(xd, t)
        ctx.lut, ctx.momentum = lut, momentum         # the table itself: the backward reads it, then updates it in place
        ctx.src = _train.src(inputs)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xd, t = ctx.saved_tensors
        lut, L = ctx.lut, _lib.lib()
        (B, F), C = xd.shape, lut.shape[0]
        dx = None
        if ctx.needs_input_grad[0]:                   # first the gradient, on the table as the forward saw it (oim.py:22-23)
            g = gy.to(xd.device, torch.float32).contiguous()
            dx = torch.empty((B, F), dtype=torch.float32, device=xd.device)
            check(L.ssg_linear_dgrad_f32(ptr(g), ptr(lut), ptr(dx), B, F, C, stream()), "ssg_linear_dgrad_f32")
        check(L.ssg_oim_update_f32(ptr(xd), F, ptr(t), ptr(lut), F, B, C, F, ctx.momentum, stream()), "ssg_oim_update_f32")
        return _train.back(dx, ctx.src[0]), None, None, None, None


def oim(inputs, targets, lut, momentum=0.5):
    """reid/loss/oim.py:8-31 as a new-style autograd function (the reference's legacy one cannot run on a current torch): the logits
    inputs @ lut.T, and in the backward first grad @ lut on the table as it stands, then for the rows in batch order
    lut[y] = normalise(momentum * lut[y] + (1 - momentum) * x), in place.  inputs [B, F] float32 with F % 32 == 0, targets [B] int64,
    lut [C, F] float32, contiguous, on the current GPU.  The update also runs when `inputs` needs no gradient (the logits then hang on
    a hidden leaf, so that a backward through them reaches this function); without a backward the table is not touched."""
    why = None
    if inputs.dim() != 2 or lut.dim() != 2 or targets.dim() != 1:
        why = "inputs must be [B, F], targets [B] and lut [C, F] (got %r, %r, %r)" % (tuple(inputs.shape), tuple(targets.shape), tuple(lut.shape))
    if why is None:
        why = linear_unsupported_reason(lut.shape[1], lut.shape[0])
        why = why and why.replace("in_features", "num_features").replace("K", "F")
    if why is None and inputs.shape[1] != lut.shape[1]:
        why = "inputs have %d features, the table F=%d" % (inputs.shape[1], lut.shape[1])
    if why is None and (inputs.shape[0] < 1 or targets.shape[0] != inputs.shape[0]):
        why = "B >= 1 rows and as many targets are required (got %r, %r)" % (tuple(inputs.shape), tuple(targets.shape))
    if why is None and (inputs.dtype != torch.float32 or lut.dtype != torch.float32 or targets.dtype != torch.int64):
        why = "inputs and lut must be float32 and targets int64 (got %s, %s, %s)" % (inputs.dtype, lut.dtype, targets.dtype)
    if why is None and (not lut.is_contiguous() or lut.requires_grad):
        why = "the table must be contiguous and must not require grad: it is updated in place"
    if why is None and (not (float(momentum) >= 0.0) or float(momentum) == float("inf")):
        why = "momentum must be finite and not negative (got %r)" % (momentum,)
    if why is None and torch.cuda.is_available() and not lut.is_cuda:
        why = "the table must be on the GPU: it is updated in place (it is on %s)" % lut.device
    _train.refuse("oim", why)
    anchor = None
    if torch.is_grad_enabled() and not inputs.requires_grad:
        anchor = torch.zeros((), requires_grad=True)
    return _OIMFn.apply(inputs, targets, lut, float(momentum), anchor)


class OIMLoss(nn.Module):
    """reid/loss/oim.py:34-52: `lut` buffer [num_classes, num_features] (the reference's key), forward(inputs, targets) ->
    (loss, scalar * logits) with differentiable logits; `weight` per class and `size_average` as F.cross_entropy takes them."""

    def __init__(self, num_features, num_classes, scalar=1.0, momentum=0.5, weight=None, size_average=True):
        super(OIMLoss, self).__init__()
        self.num_features = num_features
        self.num_classes = num_classes
        self.momentum = momentum
        self.scalar = scalar
        self.weight = weight
        self.size_average = size_average
        self.register_buffer('lut', torch.zeros(num_classes, num_features))

    def forward(self, inputs, targets):
        logits = oim(inputs, targets, self.lut, momentum=self.momentum) * self.scalar
        w = None if self.weight is None else self.weight.detach().to(logits.device, torch.float32)
        return cross_entropy_train(logits, targets, weight=w, reduction="mean" if self.size_average else "sum"), logits


def accuracy(output, target, topk=(1,)):
    """reid/evaluation_metrics/classification.py:6-19 on the current GPU: [correct_k / batch_size for k in topk], each a one-element
    float32 device tensor, the float32 product float(count) * float32(1 / B) of the reference.  A logit equal to the target's counts
    as ahead of it only at a lower index (torch.topk leaves the order of ties open).  No host read."""
    why = None
    ks = [int(k) for k in topk]
    if output.dim() != 2 or target.dim() != 1 or output.shape[0] != target.shape[0] or output.shape[0] < 1 or output.shape[1] < 1:
        why = "output must be [B, C] and target [B] with B >= 1, C >= 1 (got %r, %r)" % (tuple(output.shape), tuple(target.shape))
    elif output.dtype != torch.float32 or target.dtype != torch.int64:
        why = "output must be float32 and target int64 (got %s, %s)" % (output.dtype, target.dtype)
    elif not ks or min(ks) < 1:
        why = "topk must name at least one k >= 1 (got %r)" % (tuple(topk),)
    _train.refuse("accuracy", why)
    dev = _train.device("loss")
    L = _lib.lib()
    xd, ldx = _rows(output.detach().to(dev))
    t = target.detach().to(dev).contiguous()
    B, C = xd.shape
    rank = torch.empty((B,), dtype=torch.int32, device=dev)
    step = L.ssg_topk_correct_max_k()
    outs = []
    for i in range(0, len(ks), step):
        part = ks[i:i + step]
        out = torch.empty((len(part),), dtype=torch.float32, device=dev)
        check(L.ssg_topk_correct_f32(ptr(xd), ldx, ptr(t), B, C, (ctypes.c_int * len(part))(*part), len(part), ptr(rank), ptr(out), stream()),
              "ssg_topk_correct_f32")
        outs += [out[j:j + 1] for j in range(len(part))]
    return outs
