"""Train-mode strided Conv2d, the 7x7 stem and MaxPool2d(3, 2, 1) of the fine-tune phase on the GPU (csrc/conv_strided.hip).

The rest of the backbone beside the stride-1 convolutions, float32 NHWC, with no float atomics and every reduction cut by the shape
alone, so a forward + backward gives the same bits run to run.  The convolutions are the stride-2 class of `ssg_amd.conv` (one
autograd function for both strides) and are re-exported here under their names; the max-pool lives here:

    class S   groups 1, dilation 1, no bias, stride 2;  1x1 with padding 0, or 3x3 with padding 1;  Cin % 64 == 0 and Cout % 64 == 0
    stem      7x7, stride 2, padding 3, 3 -> 64, no bias; the images must not require grad
    pool      MaxPool2d(3, stride 2, padding 1), dilation 1, ceil_mode False, C % 4 == 0

    y  = ssg_conv2d_nhwc_f32(x, w_fwd, stride 2)     the embedder's fp32-MFMA convolution (the stem on RGB0 pixels)
    dX = ssg_conv_dgrad_strided_f32(dY, w_dgrad)     four dense GEMMs, one per (h mod 2, w mod 2) class of input pixels
    dW = ssg_conv_wgrad_strided_f32(dY, x)           fp32-MFMA partial sums over fixed pixel slices, added in float64
    pool: ssg_maxpool3x3s2_idx_nhwc records each window's winner, ssg_maxpool3x3s2_bwd_nhwc gathers dY through it

    y = conv2d_train_strided(x, weight, stride, padding)      StridedConv2d       use_device_conv(model, strided=True)
    y = max_pool2d_train(x)                                   MaxPool2d           use_device_maxpool(model)

There is no CPU fallback: without a GPU the forward raises SSGError."""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, _train
from ._lib import check, ptr, stream
from .conv import CL, StridedConv2d, _pair, conv2d_train_strided, strided_unsupported_reason  # noqa: F401 (the convolutions live in ssg_amd/conv.py)

__all__ = ["conv2d_train_strided", "StridedConv2d", "strided_unsupported_reason", "max_pool2d_train", "MaxPool2d", "use_device_maxpool",
           "pool_unsupported_reason"]


# ---- MaxPool2d(3, 2, 1) ------------------------------------------------------------------------------------------------------------------

def pool_unsupported_reason(kernel_size, stride=None, padding=0, dilation=1, return_indices=False, ceil_mode=False):
    """None for MaxPool2d(3, stride 2, padding 1, dilation 1, ceil_mode False, no indices), else the rule it breaks"""
    k, s = _pair(kernel_size), _pair(kernel_size if stride is None else stride)
    if k != (3, 3):
        return "kernel_size must be 3 (got %r)" % (k,)
    if s != (2, 2):
        return "stride must be 2 (got %r)" % (s,)
    if _pair(padding) != (1, 1):
        return "padding must be 1 (got %r)" % (padding,)
    if _pair(dilation) != (1, 1):
        return "dilation must be 1 (got %r)" % (dilation,)
    if ceil_mode:
        return "ceil_mode must be False"
    if return_indices:
        return "return_indices must be False"
    return None


class _MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        dev = _train.device("conv")
        L = _lib.lib()
        xd = x.detach().to(dev, torch.float32).contiguous(memory_format=CL)
        B, C, H, W = xd.shape
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty((B, C, OH, OW), dtype=torch.float32, device=dev, memory_format=CL)
        idx = torch.empty((B, OH, OW, C), dtype=torch.uint8, device=dev)
        check(L.ssg_maxpool3x3s2_idx_nhwc(ptr(xd), ptr(y), ptr(idx), B, H, W, C, stream()), "ssg_maxpool3x3s2_idx_nhwc")
        ctx.save_for_backward(idx)
        ctx.geom = (B, C, H, W)
        ctx.src = _train.src(x)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (idx,) = ctx.saved_tensors
        dev = idx.device
        B, C, H, W = ctx.geom
        g = gy.to(dev, torch.float32).contiguous(memory_format=CL)
        dx = torch.empty((B, C, H, W), dtype=torch.float32, device=dev, memory_format=CL)
        check(_lib.lib().ssg_maxpool3x3s2_bwd_nhwc(ptr(g), ptr(idx), ptr(dx), B, H, W, C, stream()), "ssg_maxpool3x3s2_bwd_nhwc")
        return _train.back(dx, ctx.src[0])


def max_pool2d_train(x, kernel_size=3, stride=2, padding=1, dilation=1, ceil_mode=False, return_indices=False):
    """`F.max_pool2d(x, 3, 2, 1)` as one differentiable function on the current GPU.  x [B, C, H, W] float32 with C % 4 == 0, used as it
    is when `channels_last`; y and dX come back `channels_last`.  The forward equals torch's bit for bit (a NaN in a window wins); the
    gradient of a window goes to its first maximum in row-major order, torch's CPU rule, and overlapping windows are added in a fixed
    order without atomics.  Any other pool raises ValueError naming the rule."""
    why = pool_unsupported_reason(kernel_size, stride, padding, dilation, return_indices, ceil_mode)
    if why is None and x.dim() != 4:
        why = "x must be [B, C, H, W] (got %r)" % (tuple(x.shape),)
    if why is None and (x.shape[1] % 4 or min(x.shape) < 1):
        why = "C %% 4 == 0 and a non-empty input are required (got %r)" % (tuple(x.shape),)
    if why is None and x.dtype != torch.float32:
        why = "x must be float32 (got %s)" % x.dtype
    _train.refuse("max_pool2d_train", why)
    return _MaxPoolFn.apply(x)


class MaxPool2d(nn.MaxPool2d):
    """nn.MaxPool2d(3, 2, 1) whose forward and backward run on the HIP kernels; no other pool can be built"""

    def __init__(self, kernel_size=3, stride=2, padding=1, dilation=1, return_indices=False, ceil_mode=False):
        why = pool_unsupported_reason(kernel_size, stride, padding, dilation, return_indices, ceil_mode)
        _train.refuse("ssg_amd.MaxPool2d", why)
        super(MaxPool2d, self).__init__(kernel_size, stride, padding, dilation, return_indices, ceil_mode)

    def forward(self, input):
        return max_pool2d_train(input)


def use_device_maxpool(model):
    """Replace every `nn.MaxPool2d(3, stride 2, padding 1)` in `model` (also under nn.DataParallel) by `ssg_amd.MaxPool2d`; the
    qualified names of the other max-pools are listed in `model._ssg_maxpool_skipped`.  Returns the model."""
    def swap(m):
        if pool_unsupported_reason(m.kernel_size, m.stride, m.padding, m.dilation, m.return_indices, m.ceil_mode) is None:
            return _train.adopt(MaxPool2d(), m)
        return None

    if type(model) is nn.MaxPool2d:
        raise ValueError("use_device_maxpool: pass the model that holds the pool, not the pool itself")
    return _train.swap_modules(model, "_ssg_maxpool_skipped", nn.MaxPool2d, (nn.MaxPool2d,), lambda m: isinstance(m, MaxPool2d), swap)
