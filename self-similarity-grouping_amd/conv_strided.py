"""Train-mode strided Conv2d, the 7x7 stem and MaxPool2d(3, 2, 1) of the fine-tune phase on the GPU (csrc/conv_strided.hip).

`ssg_amd.conv` covers the stride-1 convolutions of a ResNet.  This module covers the rest of the backbone, float32 NHWC, with no
float atomics and every reduction cut by the shape alone, so a forward + backward gives the same bits run to run:

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

from . import _lib
from ._lib import check, ptr, stream
from .conv import CL, _device, _pair, _zeros

__all__ = ["conv2d_train_strided", "StridedConv2d", "strided_unsupported_reason", "max_pool2d_train", "MaxPool2d", "use_device_maxpool",
           "pool_unsupported_reason"]


def strided_unsupported_reason(cin, cout, kernel_size, stride=2, padding=0, dilation=1, groups=1, bias=False, padding_mode="zeros"):
    """None when a convolution with these hyper-parameters is in class S or is the stem, else the rule it breaks (one line)"""
    k, s, d = _pair(kernel_size), _pair(stride), _pair(dilation)
    if groups != 1:
        return "groups must be 1 (got %d)" % groups
    if d != (1, 1):
        return "dilation must be 1 (got %r)" % (d,)
    if bias:
        return "the convolution must have no bias"
    if padding_mode != "zeros":
        return "padding_mode must be 'zeros' (got %r)" % (padding_mode,)
    if s != (2, 2):
        return "stride must be 2 (got %r)" % (s,)
    if k not in ((1, 1), (3, 3), (7, 7)):
        return "the kernel must be 1x1, 3x3 or the 7x7 stem (got %dx%d)" % k
    if isinstance(padding, str) or _pair(padding) != (k[0] // 2, k[0] // 2):
        return "padding must be %d for a %dx%d kernel (got %r)" % (k[0] // 2, k[0], k[1], padding)
    if k == (7, 7):
        if (cin, cout) != (3, 64):
            return "the 7x7 kernel is the stem only: Cin = 3 and Cout = 64 (got Cin=%d, Cout=%d)" % (cin, cout)
    elif cin % 64 or cout % 64 or cin <= 0 or cout <= 0:
        return "Cin %% 64 == 0 and Cout %% 64 == 0 are required (got Cin=%d, Cout=%d)" % (cin, cout)
    return None


class _StridedConv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        dev = _device()
        L = _lib.lib()
        w = weight.detach().to(dev, torch.float32)
        cout, cin, kh, kw = w.shape
        B, _, H, W = x.shape
        stem = kh == 7
        pad = kh // 2
        OH, OW = (H + 2 * pad - kh) // 2 + 1, (W + 2 * pad - kw) // 2 + 1
        s = w.stride()
        if stem:
            xn = x.detach().to(dev, torch.float32)
            xd = torch.empty((B, H, W, 4), dtype=torch.float32, device=dev)          # RGB0 pixels
            if xn.is_contiguous():
                check(L.ssg_nchw_to_nhwc4(ptr(xn), ptr(xd), B, H, W, 0, stream()), "ssg_nchw_to_nhwc4")
            else:                                     # channels_last images are RGB pixels already: one copy into RGB0, no NCHW detour
                xd[..., :3].copy_(xn.permute(0, 2, 3, 1))
                xd[..., 3].zero_()
            wf = torch.empty((cout, 32 * ((kh * kw + 7) // 8)), dtype=torch.float32, device=dev)
        else:
            xd = x.detach().to(dev, torch.float32).contiguous(memory_format=CL)
            wf = torch.empty((cout, kh * kw * cin), dtype=torch.float32, device=dev)
        check(L.ssg_conv_pack_strided_f32(ptr(w), s[0], s[1], s[2], s[3], cout, cin, kh, kw, ptr(wf), None, stream()), "ssg_conv_pack_strided_f32")
        y = torch.empty((B, cout, OH, OW), dtype=torch.float32, device=dev, memory_format=CL)
        check(L.ssg_conv2d_nhwc_f32(ptr(xd), ptr(wf), ptr(_zeros(dev, cout)), None, ptr(y), B, H, W, 4 if stem else cin, cout, kh, kw, 2, pad, 0,
                                    stream()), "ssg_conv2d_nhwc_f32 (strided forward)")
        ctx.save_for_backward(xd, w)
        ctx.geom = (B, H, W)
        ctx.src = tuple((t.device, t.dtype) for t in (x, weight))
        return y

    @staticmethod
    @once_differentiable                              # a double backward raises
    def backward(ctx, gy):
        xd, w = ctx.saved_tensors
        dev = xd.device
        L = _lib.lib()
        B, H, W = ctx.geom
        cout, cin, kh, kw = w.shape
        g = gy.to(dev, torch.float32).contiguous(memory_format=CL)
        (xdev, xdt), (wdev, wdt) = ctx.src
        dx = dw = None
        if ctx.needs_input_grad[0]:                   # never the stem: conv2d_train_strided refuses an x that requires grad
            s = w.stride()
            wd = torch.empty((kh * kw, cout, cin), dtype=torch.float32, device=dev)
            check(L.ssg_conv_pack_strided_f32(ptr(w), s[0], s[1], s[2], s[3], cout, cin, kh, kw, None, ptr(wd), stream()), "ssg_conv_pack_strided_f32")
            dx = torch.empty((B, cin, H, W), dtype=torch.float32, device=dev, memory_format=CL)
            check(L.ssg_conv_dgrad_strided_f32(ptr(g), ptr(wd), ptr(dx), B, H, W, cin, cout, kh, kw, 2, stream()), "ssg_conv_dgrad_strided_f32")
            dx = dx.to(device=xdev, dtype=xdt)
        if ctx.needs_input_grad[1]:
            M = g.shape[0] * g.shape[2] * g.shape[3]
            nws = L.ssg_conv_wgrad_strided_workspace_bytes(M, cout, kh, kw, cin, 2)
            if nws == 0:
                raise ValueError("conv2d_train_strided: %s" % L.ssg_last_error().decode("utf-8", "replace"))
            ws = torch.empty(nws // 4, dtype=torch.float32, device=dev)
            dw = torch.empty_like(w)                  # preserve_format: the weight's strides (contiguous or channels_last)
            s = dw.stride()
            check(L.ssg_conv_wgrad_strided_f32(ptr(g), ptr(xd), B, H, W, cin, cout, kh, kw, 2, ptr(dw), s[0], s[1], s[2], s[3], ptr(ws), nws, 3,
                                               stream()), "ssg_conv_wgrad_strided_f32")
            dw = dw.to(device=wdev, dtype=wdt)
        return dx, dw


def conv2d_train_strided(x, weight, stride=2, padding=0, dilation=1, groups=1, bias=None):
    """`F.conv2d(x, weight, None, stride, padding)` for the stride-2 classes (see the module docstring) as one differentiable function
    on the current GPU.  Layout rules as for `conv2d_train`: x [B, Cin, H, W] and weight [Cout, Cin, KH, KW] float32; a `channels_last`
    x is used as it is, anything else is laid out first; y and dX come back `channels_last`, dW in the weight's shape and memory
    format.  The stem (7x7, 3 -> 64) has no data gradient: an x that requires grad raises ValueError.  A shape outside the classes
    raises ValueError naming the rule; a double backward raises.  No host read, no synchronisation."""
    if x.dim() != 4 or weight.dim() != 4:
        raise ValueError("conv2d_train_strided: x must be [B, Cin, H, W] and weight [Cout, Cin, KH, KW] (got %r, %r)" % (tuple(x.shape), tuple(weight.shape)))
    cout, cin_w, kh, kw = weight.shape
    why = strided_unsupported_reason(x.shape[1] if groups == 1 else cin_w * groups, cout, (kh, kw), stride, padding, dilation, groups, bias is not None)
    if why is None and x.shape[1] != cin_w:
        why = "x has %d channels, the weight takes %d" % (x.shape[1], cin_w)
    if why is None and (x.shape[0] < 1 or x.shape[2] < 1 or x.shape[3] < 1):
        why = "the input is empty %r" % (tuple(x.shape),)
    if why is None and (x.dtype != torch.float32 or weight.dtype != torch.float32):
        why = "x and weight must be float32 (got %s, %s)" % (x.dtype, weight.dtype)
    if why is None and kh == 7 and x.requires_grad and torch.is_grad_enabled():
        why = "the stem has no data gradient: x must not require grad"
    if why is not None:
        raise ValueError("conv2d_train_strided: " + why)
    return _StridedConv2dFn.apply(x, weight)


class StridedConv2d(nn.Conv2d):
    """nn.Conv2d (same parameter and state-dict key) for the stride-2 classes and the stem, on the HIP kernels in train and in eval
    mode.  Nothing else can be built; the output is `channels_last`."""
    _ssg_device_conv = True                           # use_device_conv leaves it alone and off the skipped list

    def __init__(self, in_channels, out_channels, kernel_size, stride=2, padding=0, dilation=1, groups=1, bias=False, padding_mode="zeros", **kw):
        why = strided_unsupported_reason(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode)
        if why is not None:
            raise ValueError("ssg_amd.StridedConv2d: " + why)
        super(StridedConv2d, self).__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, **kw)

    def forward(self, input):
        return conv2d_train_strided(input, self.weight, self.stride, self.padding)


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
        dev = _device()
        L = _lib.lib()
        xd = x.detach().to(dev, torch.float32).contiguous(memory_format=CL)
        B, C, H, W = xd.shape
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty((B, C, OH, OW), dtype=torch.float32, device=dev, memory_format=CL)
        idx = torch.empty((B, OH, OW, C), dtype=torch.uint8, device=dev)
        check(L.ssg_maxpool3x3s2_idx_nhwc(ptr(xd), ptr(y), ptr(idx), B, H, W, C, stream()), "ssg_maxpool3x3s2_idx_nhwc")
        ctx.save_for_backward(idx)
        ctx.geom = (B, C, H, W)
        ctx.src = (x.device, x.dtype)
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
        return dx.to(device=ctx.src[0], dtype=ctx.src[1])


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
    if why is not None:
        raise ValueError("max_pool2d_train: " + why)
    return _MaxPoolFn.apply(x)


class MaxPool2d(nn.MaxPool2d):
    """nn.MaxPool2d(3, 2, 1) whose forward and backward run on the HIP kernels; no other pool can be built"""

    def __init__(self, kernel_size=3, stride=2, padding=1, dilation=1, return_indices=False, ceil_mode=False):
        why = pool_unsupported_reason(kernel_size, stride, padding, dilation, return_indices, ceil_mode)
        if why is not None:
            raise ValueError("ssg_amd.MaxPool2d: " + why)
        super(MaxPool2d, self).__init__(kernel_size, stride, padding, dilation, return_indices, ceil_mode)

    def forward(self, input):
        return max_pool2d_train(input)


def use_device_maxpool(model):
    """Replace every `nn.MaxPool2d(3, stride 2, padding 1)` in `model` (also under nn.DataParallel) by `ssg_amd.MaxPool2d`; the
    qualified names of the other max-pools are listed in `model._ssg_maxpool_skipped`.  Returns the model."""
    skipped = []

    def walk(parent, prefix):
        for name, child in list(parent._modules.items()):
            if child is None or isinstance(child, MaxPool2d):
                continue
            if isinstance(child, nn.MaxPool2d):
                if type(child) is nn.MaxPool2d and pool_unsupported_reason(child.kernel_size, child.stride, child.padding, child.dilation,
                                                                           child.return_indices, child.ceil_mode) is None:
                    new = MaxPool2d()
                    new.training = child.training
                    parent._modules[name] = new
                else:
                    skipped.append(prefix + name)
                continue
            walk(child, prefix + name + ".")

    if type(model) is nn.MaxPool2d:
        raise ValueError("use_device_maxpool: pass the model that holds the pool, not the pool itself")
    walk(model, "")
    model._ssg_maxpool_skipped = skipped
    return model
