"""Train-mode Conv2d of the fine-tune phase on the GPU: forward, data gradient and weight gradient, float32 NHWC.

The reference trains torch's ResNet (reid/trainers.py), so its convolutions are the vendor library's.  This module runs a ResNet's
convolutions on the project's kernels, in two stride classes (groups 1, dilation 1, no bias in both):

    stride 1   1x1 with padding 0, or 3x3 with padding 1;  Cin % 64 == 0 and Cout % 64 == 0
               (46 of ResNet-50's 53 convolutions, all of layer1 of resnet18/34)
    stride 2   class S: the same kernels, paddings and channel rule;  the stem: 7x7, padding 3, 3 -> 64, the images must not require grad

    stride 1   y  = ssg_conv2d_nhwc_f32(x,  w_fwd)      the embedder's fp32-MFMA convolution (zero bias, no residual, no ReLU)
               dX = ssg_conv2d_nhwc_f32(dY, w_dgrad)    the same kernel: the weight transposed in (Cout, Cin), rotated by 180 degrees in (r, s)
               dW = ssg_conv_wgrad_f32(dY, x)           csrc/conv_train.hip: fp32-MFMA partial sums over fixed pixel slices, added in float64
    stride 2   y  = ssg_conv2d_nhwc_f32(x, w_fwd, stride 2)     the same convolution (the stem on RGB0 pixels)
               dX = ssg_conv_dgrad_strided_f32(dY, w_dgrad)     csrc/conv_strided.hip: four dense GEMMs, one per (h mod 2, w mod 2) class
               dW = ssg_conv_wgrad_strided_f32(dY, x)           the same partial sums and float64 slice sum

`ssg_conv_pack_train_f32` / `ssg_conv_pack_strided_f32` write the packings from the weight in one launch per pass.  No float atomics,
and every reduction is cut by the shape alone, so a forward + backward gives the same bits run to run.

    y = conv2d_train(x, weight, stride=1, padding=0)             Conv2d          nn.Conv2d with that forward (train and eval: the
    y = conv2d_train_strided(x, weight, stride=2, padding=0)     StridedConv2d   convolution has no mode)
    use_device_conv(model)          swaps every nn.Conv2d of the stride-1 class in a built model (strided=True: also the stride-2 classes)

There is no CPU fallback: without a GPU the forward raises SSGError."""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, _train
from ._lib import check, ptr, stream

__all__ = ["conv2d_train", "Conv2d", "use_device_conv", "unsupported_reason"]

CL = torch.channels_last

# stride class -> (function, module, packing, workspace size and weight gradient entry points)
_NAMES = {1: ("conv2d_train", "Conv2d", "ssg_conv_pack_train_f32", "ssg_conv_wgrad_workspace_bytes", "ssg_conv_wgrad_f32"),
          2: ("conv2d_train_strided", "StridedConv2d", "ssg_conv_pack_strided_f32", "ssg_conv_wgrad_strided_workspace_bytes",
              "ssg_conv_wgrad_strided_f32")}


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def _reason(cls, cin, cout, kernel_size, stride, padding, dilation, groups, bias, padding_mode):
    """None when a convolution with these hyper-parameters is in stride class `cls` (1 or 2), else the rule it breaks (one line)"""
    k, s, d = _pair(kernel_size), _pair(stride), _pair(dilation)
    if groups != 1:
        return "groups must be 1 (got %d)" % groups
    if d != (1, 1):
        return "dilation must be 1 (got %r)" % (d,)
    if bias:
        return "the convolution must have no bias"
    if padding_mode != "zeros":
        return "padding_mode must be 'zeros' (got %r)" % (padding_mode,)
    if s != (cls, cls):
        return "stride must be %d (got %r)" % (cls, s)
    if cls == 1 and k not in ((1, 1), (3, 3)):
        return "the kernel must be 1x1 or 3x3 (got %dx%d)" % k
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


def unsupported_reason(cin, cout, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=False, padding_mode="zeros"):
    """None when a convolution with these hyper-parameters is in the stride-1 class, else the rule it breaks (one line)"""
    return _reason(1, cin, cout, kernel_size, stride, padding, dilation, groups, bias, padding_mode)


def strided_unsupported_reason(cin, cout, kernel_size, stride=2, padding=0, dilation=1, groups=1, bias=False, padding_mode="zeros"):
    """None when a convolution with these hyper-parameters is in class S or is the stem, else the rule it breaks (one line)"""
    return _reason(2, cin, cout, kernel_size, stride, padding, dilation, groups, bias, padding_mode)


def _zeros(dev, n):
    """the zero bias vector the convolution kernel reads (it dereferences `bias` unconditionally)"""
    return torch.zeros(n, dtype=torch.float32, device=dev)


def _pack(L, cls, w, wf, wd):
    cout, cin, kh, kw = w.shape
    s = w.stride()
    check(getattr(L, _NAMES[cls][2])(ptr(w), s[0], s[1], s[2], s[3], cout, cin, kh, kw, ptr(wf), ptr(wd), stream()), _NAMES[cls][2])


def _rgb0(L, x, dev):
    """the stem's images as [B, H, W, 4] RGB0 pixels"""
    B, _, H, W = x.shape
    xn = x.detach().to(dev, torch.float32)
    xd = torch.empty((B, H, W, 4), dtype=torch.float32, device=dev)
    if xn.is_contiguous():
        check(L.ssg_nchw_to_nhwc4(ptr(xn), ptr(xd), B, H, W, 0, stream()), "ssg_nchw_to_nhwc4")
    else:                                             # channels_last images are RGB pixels already: one copy into RGB0, no NCHW detour
        xd[..., :3].copy_(xn.permute(0, 2, 3, 1))
        xd[..., 3].zero_()
    return xd


class _ConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, cls):
        dev = _train.device("conv")
        L = _lib.lib()
        w = weight.detach().to(dev, torch.float32)
        cout, cin, kh, kw = w.shape
        B, _, H, W = x.shape
        stem = kh == 7
        pad = kh // 2
        OH, OW = (H + 2 * pad - kh) // cls + 1, (W + 2 * pad - kw) // cls + 1
        if stem:
            xd = _rgb0(L, x, dev)
            wf = torch.empty((cout, 32 * ((kh * kw + 7) // 8)), dtype=torch.float32, device=dev)
        else:
            xd = x.detach().to(dev, torch.float32).contiguous(memory_format=CL)
            wf = torch.empty((cout, kh * kw * cin), dtype=torch.float32, device=dev)
        _pack(L, cls, w, wf, None)
        y = torch.empty((B, cout, OH, OW), dtype=torch.float32, device=dev, memory_format=CL)
        check(L.ssg_conv2d_nhwc_f32(ptr(xd), ptr(wf), ptr(_zeros(dev, cout)), None, ptr(y), B, H, W, 4 if stem else cin, cout, kh, kw, cls, pad, 0,
                                    stream()), "ssg_conv2d_nhwc_f32 (%sforward)" % ("strided " if cls == 2 else ""))
        ctx.save_for_backward(xd, w)
        ctx.geom = (B, H, W, cls)
        ctx.src = _train.src(x, weight)
        return y

    @staticmethod
    @once_differentiable                              # a double backward raises
    def backward(ctx, gy):
        xd, w = ctx.saved_tensors
        dev = xd.device
        L = _lib.lib()
        B, H, W, cls = ctx.geom
        cout, cin, kh, kw = w.shape
        fn, _, _, ws_bytes, wgrad = _NAMES[cls]
        g = gy.to(dev, torch.float32).contiguous(memory_format=CL)
        dx = dw = None
        if ctx.needs_input_grad[0]:                   # never the stem: conv2d_train_strided refuses an x that requires grad
            wd = torch.empty((cin, kh * kw * cout) if cls == 1 else (kh * kw, cout, cin), dtype=torch.float32, device=dev)
            _pack(L, cls, w, None, wd)
            dx = torch.empty((B, cin, H, W), dtype=torch.float32, device=dev, memory_format=CL)
            if cls == 1:
                check(L.ssg_conv2d_nhwc_f32(ptr(g), ptr(wd), ptr(_zeros(dev, cin)), None, ptr(dx), B, H, W, cout, cin, kh, kw, 1, kh // 2, 0, stream()),
                      "ssg_conv2d_nhwc_f32 (data gradient)")
            else:
                check(L.ssg_conv_dgrad_strided_f32(ptr(g), ptr(wd), ptr(dx), B, H, W, cin, cout, kh, kw, 2, stream()), "ssg_conv_dgrad_strided_f32")
        if ctx.needs_input_grad[1]:
            tail = () if cls == 1 else (2,)           # the strided entry points take the stride after the kernel size
            M = g.shape[0] * g.shape[2] * g.shape[3]
            nws = getattr(L, ws_bytes)(M, cout, kh, kw, cin, *tail)
            if nws == 0:
                raise ValueError("%s: %s" % (fn, L.ssg_last_error().decode("utf-8", "replace")))
            ws = torch.empty(nws // 4, dtype=torch.float32, device=dev)
            dw = torch.empty_like(w)                  # preserve_format: the weight's strides (contiguous or channels_last)
            s = dw.stride()
            check(getattr(L, wgrad)(ptr(g), ptr(xd), B, H, W, cin, cout, kh, kw, *tail, ptr(dw), s[0], s[1], s[2], s[3], ptr(ws), nws, 3, stream()),
                  wgrad)
        return _train.back(dx, ctx.src[0]), _train.back(dw, ctx.src[1]), None


def _conv2d_train(cls, x, weight, stride, padding, dilation=1, groups=1, bias=None):
    fn = _NAMES[cls][0]
    if x.dim() != 4 or weight.dim() != 4:
        raise ValueError("%s: x must be [B, Cin, H, W] and weight [Cout, Cin, KH, KW] (got %r, %r)" % (fn, tuple(x.shape), tuple(weight.shape)))
    cout, cin_w, kh, kw = weight.shape
    why = _reason(cls, x.shape[1] if groups == 1 else cin_w * groups, cout, (kh, kw), stride, padding, dilation, groups, bias is not None, "zeros")
    if why is None and x.shape[1] != cin_w:
        why = "x has %d channels, the weight takes %d" % (x.shape[1], cin_w)
    if why is None and (x.shape[0] < 1 or x.shape[2] < 1 or x.shape[3] < 1):
        why = "the input is empty %r" % (tuple(x.shape),)
    if why is None and (x.dtype != torch.float32 or weight.dtype != torch.float32):
        why = "x and weight must be float32 (got %s, %s)" % (x.dtype, weight.dtype)
    if why is None and kh == 7 and x.requires_grad and torch.is_grad_enabled():
        why = "the stem has no data gradient: x must not require grad"
    _train.refuse(fn, why)
    return _ConvFn.apply(x, weight, cls)


def conv2d_train(x, weight, stride=1, padding=0, dilation=1, groups=1, bias=None):
    """`F.conv2d(x, weight, None, stride, padding)` for the stride-1 class (see the module docstring) as one differentiable function on
    the current GPU.  x [B, Cin, H, W] and weight [Cout, Cin, KH, KW] float32; a `channels_last` x is used as it is, anything else is
    made `channels_last` first.  y and dX come back `channels_last`, dW in the weight's shape and memory format.  When x does not require
    grad the data gradient is skipped, when weight does not the weight gradient is.  A shape outside the class raises ValueError
    naming the rule; a double backward raises.  No host read, no synchronisation."""
    return _conv2d_train(1, x, weight, stride, padding, dilation, groups, bias)


def conv2d_train_strided(x, weight, stride=2, padding=0, dilation=1, groups=1, bias=None):
    """`F.conv2d(x, weight, None, stride, padding)` for the stride-2 classes (see the module docstring) as one differentiable function
    on the current GPU.  Layout rules as for `conv2d_train`: x [B, Cin, H, W] and weight [Cout, Cin, KH, KW] float32; a `channels_last`
    x is used as it is, anything else is laid out first; y and dX come back `channels_last`, dW in the weight's shape and memory
    format.  The stem (7x7, 3 -> 64) has no data gradient: an x that requires grad raises ValueError.  A shape outside the classes
    raises ValueError naming the rule; a double backward raises.  No host read, no synchronisation."""
    return _conv2d_train(2, x, weight, stride, padding, dilation, groups, bias)


class _DeviceConv(object):
    """__init__ and forward of the device modules (in front of nn.Conv2d in the MRO); `_ssg_stride` is the stride class"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=None, padding=0, dilation=1, groups=1, bias=False, padding_mode="zeros", **kw):
        stride = self._ssg_stride if stride is None else stride
        _train.refuse("ssg_amd." + _NAMES[self._ssg_stride][1],
                      _reason(self._ssg_stride, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode))
        super(_DeviceConv, self).__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, **kw)

    def forward(self, input):
        return _conv2d_train(self._ssg_stride, input, self.weight, self.stride, self.padding)


class Conv2d(_DeviceConv, nn.Conv2d):
    """nn.Conv2d (same parameter and state-dict key) whose forward, data gradient and weight gradient run on the HIP kernels, in train
    and in eval mode.  Only the stride-1 class can be built (stride=None: 1); the output is `channels_last`."""
    _ssg_stride = 1


class StridedConv2d(_DeviceConv, nn.Conv2d):
    """nn.Conv2d (same parameter and state-dict key) for the stride-2 classes and the stem, on the HIP kernels in train and in eval
    mode.  Nothing else can be built (stride=None: 2); the output is `channels_last`."""
    _ssg_stride = 2


def use_device_conv(model, strided=False):
    """Replace every `nn.Conv2d` of the stride-1 class in `model` (also under nn.DataParallel: the walk goes through `.module`) by
    `ssg_amd.Conv2d`.  The Parameter objects are kept, so optimiser groups built before the call and the state-dict keys stay valid.
    The qualified names of the convolutions left alone (strided, 7x7, with a bias, ..., and other subclasses of nn.Conv2d) are listed
    in `model._ssg_conv_skipped`.  `strided=True` also swaps the stride-2 1x1 / 3x3 convolutions and the 7x7 stem for
    `ssg_amd.StridedConv2d`, which leaves none of a ResNet's convolutions on the skipped list; a later call
    without the keyword leaves those modules where they are and does not list them.  Run the model
    on `channels_last` input (`model.to(memory_format=torch.channels_last)`) so that no layout copy is made between the layers.
    Returns the model."""
    def swap(m):
        for new in (Conv2d, StridedConv2d) if strided else (Conv2d,):
            if m.weight.dtype == torch.float32 and _reason(new._ssg_stride, m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding,
                                                           m.dilation, m.groups, m.bias is not None, m.padding_mode) is None:
                return _train.adopt(new(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, device="meta"), m, ("weight",))
        return None

    if type(model) is nn.Conv2d:
        raise ValueError("use_device_conv: pass the model that holds the convolution, not the convolution itself")
    return _train.swap_modules(model, "_ssg_conv_skipped", nn.Conv2d, (nn.Conv2d,), lambda m: isinstance(m, _DeviceConv), swap)
