"""Train-mode head of the fine-tune phase on the GPU: stripe pooling and Linear (csrc/head_train.hip).

The reference's model (reid/models/resnet.py:86-134) average-pools the layer4 map S + 2 times with separate `F.avg_pool2d` calls
(S = num_split) and sends the global average through `feat = Linear(out_planes, num_features, bias=False)`, `feat_bn`, a ReLU and,
under SSG++, dropout and `classifier_x2 = Linear(num_features, num_classes)`.  This module runs the pools and the Linears on the
project's kernels, float32, with no float atomics and a summation order that depends on the shape alone, so together with
`ssg_amd.conv`, `ssg_amd.conv_strided` and `ssg_amd.batchnorm` a whole training step gives the same bits run to run:

    sets = ssg_gap_stripes(x)                  one launch for all S + 1 averages (one when S == 1)
    dX   = ssg_gap_stripes_bwd(g, mask)        dX[b,y,x,c] = g0 / (h w) + g_stripe(y) / ((h // S) w), every element written once
    y    = ssg_linear_fwd_f32(x, W, bias)      fp32-MFMA GEMMs on nn.Linear's own [N, K] weight: no pack launch, no transposed copy
    dX   = ssg_linear_dgrad_f32(dY, W)
    dW, db = ssg_linear_wgrad_f32(dY, x)       db in float64, ascending b

    sets = stripe_pool_train(x, num_split)     tuple of [B, C] tensors
    y = linear_train(x, weight, bias=None)     Linear (nn.Linear with that forward, train and eval)
    use_device_head(model)                     swaps the Linears and gives the model DeviceHeadMixin's forward

There is no CPU fallback: without a GPU the forward raises SSGError."""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, _train
from ._lib import check, ptr, stream
from .conv import CL

__all__ = ["stripe_pool_train", "linear_train", "Linear", "DeviceHeadMixin", "use_device_head", "linear_unsupported_reason",
           "stripe_pool_unsupported_reason"]

MAX_SPLIT = 30                                        # the sets are named by the bits of an int
HEAD_ATTRIBUTES = ("base", "num_split", "num_features", "num_classes", "cluster")


# ---- stripe pooling ------------------------------------------------------------------------------------------------------------------------

def stripe_pool_unsupported_reason(shape, num_split):
    """None when a [B, C, h, w] map can be pooled into `num_split` stripes on the device, else the rule it breaks (one line)"""
    if len(shape) != 4:
        return "x must be [B, C, h, w] (got %r)" % (tuple(shape),)
    B, C, h, w = shape
    if int(num_split) != num_split or num_split < 1 or num_split > MAX_SPLIT:
        return "num_split must be an integer in 1 .. %d (got %r)" % (MAX_SPLIT, num_split)
    if min(B, C, h, w) < 1:
        return "the input is empty %r" % (tuple(shape),)
    if num_split > h:
        return "num_split must not exceed the map's height: a stripe needs at least one row (num_split=%d, h=%d)" % (num_split, h)
    if C % 4:
        return "C %% 4 == 0 is required (got C=%d)" % C
    return None


class _StripePoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, S):
        dev = _train.device("conv")
        xd = x.detach().to(dev, torch.float32).contiguous(memory_format=CL)
        B, C, h, w = xd.shape
        nsets = S + 1 if S > 1 else 1
        out = torch.empty((nsets, B, C), dtype=torch.float32, device=dev)
        check(_lib.lib().ssg_gap_stripes(ptr(xd), ptr(out), B, h, w, C, S, stream()), "ssg_gap_stripes")
        ctx.geom = (B, C, h, w, S)                    # nothing about x is kept but its shape
        ctx.src = _train.src(x)
        ctx.dev = dev
        ctx.set_materialize_grads(False)              # a set that got no gradient arrives as None and is not read
        return tuple(out[i] for i in range(nsets))

    @staticmethod
    @once_differentiable                              # a double backward raises
    def backward(ctx, *grads):
        B, C, h, w, S = ctx.geom
        dev = ctx.dev
        g = torch.empty((len(grads), B, C), dtype=torch.float32, device=dev)
        mask = 0
        for i, gi in enumerate(grads):
            if gi is not None:
                g[i].copy_(gi)
                mask |= 1 << i
        dx = torch.empty((B, C, h, w), dtype=torch.float32, device=dev, memory_format=CL)
        check(_lib.lib().ssg_gap_stripes_bwd(ptr(g), mask, ptr(dx), B, h, w, C, S, stream()), "ssg_gap_stripes_bwd")
        return _train.back(dx, ctx.src[0]), None


def stripe_pool_train(x, num_split=1):
    """The average pools of the reference's head (resnet.py:93-114) as one differentiable function on the current GPU.  x [B, C, h, w]
    float32 with C % 4 == 0, used as it is when `channels_last`, laid out first otherwise.  Returns a tuple of [B, C] tensors, slices of
    one [nsets, B, C] buffer written by one launch: set 0 the global average and, when num_split = S > 1, set s = 1..S the average of
    rows [(s-1)*(h//S), s*(h//S)) -- the reference's slicing, so with h % S != 0 the trailing rows belong to no stripe.  The backward is
    one launch that writes every element of dX (channels_last) once; the sets that received no gradient are not read.  Anything else
    raises ValueError naming the rule; a double backward raises.  No host read, no synchronisation."""
    why = stripe_pool_unsupported_reason(tuple(x.shape), num_split)
    if why is None and x.dtype != torch.float32:
        why = "x must be float32 (got %s)" % x.dtype
    _train.refuse("stripe_pool_train", why)
    return _StripePoolFn.apply(x, int(num_split))


# ---- Linear ----------------------------------------------------------------------------------------------------------------------------------

def linear_unsupported_reason(in_features, out_features):
    """None when a Linear with these sizes is in the device class, else the rule it breaks (one line)"""
    if in_features <= 0 or in_features % 32:
        return "K %% 32 == 0 is required of in_features (got K=%d)" % in_features
    if out_features < 1:
        return "out_features must be at least 1 (got N=%d)" % out_features
    return None


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        dev = _train.device("conv")
        xd = x.detach().to(dev, torch.float32).contiguous()
        w = weight.detach().to(dev, torch.float32)
        b = None if bias is None else bias.detach().to(dev, torch.float32).contiguous()
        (B, K), N = xd.shape, w.shape[0]
        y = torch.empty((B, N), dtype=torch.float32, device=dev)
        check(_lib.lib().ssg_linear_fwd_f32(ptr(xd), ptr(w), ptr(b), ptr(y), B, K, N, stream()), "ssg_linear_fwd_f32")
        ctx.save_for_backward(xd, w)                  # only x and the weight are kept
        ctx.src = _train.src(x, weight, bias)
        return y

    @staticmethod
    @once_differentiable                              # a double backward raises
    def backward(ctx, gy):
        xd, w = ctx.saved_tensors
        dev = xd.device
        L = _lib.lib()
        (B, K), N = xd.shape, w.shape[0]
        g = gy.to(dev, torch.float32).contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((B, K), dtype=torch.float32, device=dev)
            check(L.ssg_linear_dgrad_f32(ptr(g), ptr(w), ptr(dx), B, K, N, stream()), "ssg_linear_dgrad_f32")
        want_db = ctx.src[2] is not None and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_db:
            if ctx.needs_input_grad[1]:
                dw = torch.empty((N, K), dtype=torch.float32, device=dev)
            if want_db:
                db = torch.empty((N,), dtype=torch.float32, device=dev)
            check(L.ssg_linear_wgrad_f32(ptr(g), ptr(xd), ptr(dw), ptr(db), B, K, N, stream()), "ssg_linear_wgrad_f32")
        return tuple(_train.back(g, where) for g, where in zip((dx, dw, db), ctx.src))


def linear_train(x, weight, bias=None):
    """`F.linear(x, weight, bias)` as one differentiable function on the current GPU.  x [B, K] with B >= 1, weight [N, K] contiguous
    with K % 32 == 0 and N >= 1, bias [N] or None, all float32.  The weight is read where it lies by all three kernels.  A frozen input
    skips the data gradient, a frozen weight the weight gradient; only x and the weight are kept for the backward.  Anything else raises
    ValueError naming the rule; a double backward raises.  No host read, no synchronisation."""
    why = None
    if x.dim() != 2 or weight.dim() != 2:
        why = "x must be [B, K] and weight [N, K] (got %r, %r)" % (tuple(x.shape), tuple(weight.shape))
    if why is None:
        why = linear_unsupported_reason(weight.shape[1], weight.shape[0])
    if why is None and x.shape[1] != weight.shape[1]:
        why = "x has %d features, the weight takes K=%d" % (x.shape[1], weight.shape[1])
    if why is None and x.shape[0] < 1:
        why = "B >= 1 is required: the input is empty %r" % (tuple(x.shape),)
    if why is None and not weight.is_contiguous():
        why = "the weight must be contiguous (strides %r)" % (tuple(weight.stride()),)
    if why is None and bias is not None and tuple(bias.shape) != (weight.shape[0],):
        why = "bias must be [N] = [%d] (got %r)" % (weight.shape[0], tuple(bias.shape))
    if why is None and any(t.dtype != torch.float32 for t in (x, weight, bias) if t is not None):
        why = "x, weight and bias must be float32 (got %s)" % ", ".join(str(t.dtype) for t in (x, weight, bias) if t is not None)
    _train.refuse("linear_train", why)
    return _LinearFn.apply(x, weight, bias)


class Linear(nn.Linear):
    """nn.Linear (same parameters and state-dict keys) whose forward, data gradient and weight / bias gradient run on the HIP kernels,
    in train and in eval mode.  Only the device class (in_features % 32 == 0) can be built; the input is [B, in_features]."""

    def __init__(self, in_features, out_features, bias=True, **kw):
        _train.refuse("ssg_amd.Linear", linear_unsupported_reason(in_features, out_features))
        super(Linear, self).__init__(in_features, out_features, bias, **kw)

    def forward(self, input):
        return linear_train(input, self.weight, self.bias)


def _swap(m):
    """the device module holding the Parameter objects of the plain nn.Linear `m`, None when `m` is outside the device class"""
    if linear_unsupported_reason(m.in_features, m.out_features) is not None:
        return None
    if not (all(p.dtype == torch.float32 for p in (m.weight, m.bias) if p is not None) and m.weight.is_contiguous()):
        return None
    return _train.adopt(Linear(m.in_features, m.out_features, m.bias is not None, device="meta"), m, ("weight", "bias"))


# ---- the model's forward ------------------------------------------------------------------------------------------------------------------

class DeviceHeadMixin(object):
    """The forward of the reference's ResNet (reid/models/resnet.py:86-134) with one `stripe_pool_train` call where the reference
    makes S + 2 `F.avg_pool2d` calls.  The host keeps its modules and attributes (`base`, `num_split`, `num_features`, `num_classes`,
    `cluster`, and `feat`, `feat_bn`, `relu`, `drop`, `classifier_x2`, `assignment` as the reference builds them); the outputs have the
    reference's tuple / list structure.  `use_device_head` puts it in front of the model's own class."""

    def forward(self, x, for_eval=False):
        for name, module in self.base._modules.items():
            if name == 'avgpool':
                break
            x = module(x)
        sets = stripe_pool_train(x, self.num_split)
        x1 = list(sets) if self.num_split > 1 else sets[0]
        if self.num_features > 0:
            x2 = self.relu(self.feat_bn(self.feat(sets[0])))
        if self.num_classes > 0:
            x2 = self.classifier_x2(self.drop(x2))

        if for_eval and isinstance(x1, list):
            return torch.cat(x1, dim=1), x2
        if self.cluster:
            x3 = self.assignment(torch.cat(x1, dim=1) if isinstance(x1, list) else x1)
            return x1, x2, x3
        return x1, x2


_HEAD_CLASSES = {}


def use_device_head(model):
    """Put the head of the reference's torch model (also under nn.DataParallel) on the device path.  Every plain `nn.Linear` with
    in_features % 32 == 0, float32 and contiguous becomes `ssg_amd.Linear` holding the same Parameter objects, so optimiser groups
    built before the call and the state-dict keys stay valid; the qualified names of the other Linears are listed in
    `model._ssg_linear_skipped`.  The host module (the model, or its `.module`) gets the class `(DeviceHeadMixin, its own class)`, whose
    forward pools with one `stripe_pool_train` call; it must have the attributes `base`, `num_split`, `num_features`, `num_classes` and
    `cluster`, else ValueError names the missing one and nothing is changed.  A second call changes nothing.  Returns the model."""
    host = model.module if isinstance(model, nn.DataParallel) else model
    for a in HEAD_ATTRIBUTES:
        if not hasattr(host, a):
            raise ValueError("use_device_head: the model has no attribute `%s` (it needs %s, as reid/models/resnet.py's ResNet has them)"
                             % (a, ", ".join(HEAD_ATTRIBUTES)))
    _train.swap_modules(model, "_ssg_linear_skipped", nn.Linear, (nn.Linear,), lambda m: isinstance(m, Linear), _swap)
    if not isinstance(host, DeviceHeadMixin):
        cls = type(host)
        if cls not in _HEAD_CLASSES:
            _HEAD_CLASSES[cls] = type("DeviceHead" + cls.__name__, (DeviceHeadMixin, cls), {})
        host.__class__ = _HEAD_CLASSES[cls]
    return model
