"""Train-mode Conv2d of the fine-tune phase on the GPU: forward, data gradient and weight gradient.

The reference trains torch's ResNet (reid/trainers.py), so its convolutions are the vendor library's.  For the class

    groups 1, dilation 1, no bias, stride 1;  1x1 with padding 0, or 3x3 with padding 1;  Cin % 64 == 0 and Cout % 64 == 0

(46 of ResNet-50's 53 convolutions, all of layer1 of resnet18/34) this module runs them on the project's kernels, float32 NHWC:

    y  = ssg_conv2d_nhwc_f32(x,  w_fwd)      the embedder's fp32-MFMA convolution (zero bias, no residual, no ReLU)
    dX = ssg_conv2d_nhwc_f32(dY, w_dgrad)    the same kernel: the weight transposed in (Cout, Cin), rotated by 180 degrees in (r, s)
    dW = ssg_conv_wgrad_f32(dY, x)           csrc/conv_train.hip: fp32-MFMA partial sums over fixed pixel slices, added in float64

`ssg_conv_pack_train_f32` writes the two packings from the weight in one launch per pass.  The weight gradient has no float atomics
and its slice cut depends on the shape alone, so a forward + backward gives the same bits run to run.

    y = conv2d_train(x, weight, stride=1, padding=0)
    Conv2d                          nn.Conv2d with that forward (train and eval: the convolution has no mode)
    use_device_conv(model)          swaps every nn.Conv2d of the class in a built model (strided=True: also the stride-2 classes and
                                    the 7x7 stem of ssg_amd/conv_strided.py)

There is no CPU fallback: without a GPU the forward raises SSGError."""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import SSGError, check, ptr, stream

__all__ = ["conv2d_train", "Conv2d", "use_device_conv", "unsupported_reason"]

CL = torch.channels_last


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def unsupported_reason(cin, cout, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=False, padding_mode="zeros"):
    """None when a convolution with these hyper-parameters is in the device class, else the rule it breaks (one line)"""
    k, s, d = _pair(kernel_size), _pair(stride), _pair(dilation)
    if groups != 1:
        return "groups must be 1 (got %d)" % groups
    if d != (1, 1):
        return "dilation must be 1 (got %r)" % (d,)
    if bias:
        return "the convolution must have no bias"
    if padding_mode != "zeros":
        return "padding_mode must be 'zeros' (got %r)" % (padding_mode,)
    if s != (1, 1):
        return "stride must be 1 (got %r)" % (s,)
    if k not in ((1, 1), (3, 3)):
        return "the kernel must be 1x1 or 3x3 (got %dx%d)" % k
    if isinstance(padding, str) or _pair(padding) != (k[0] // 2, k[0] // 2):
        return "padding must be %d for a %dx%d kernel (got %r)" % (k[0] // 2, k[0], k[1], padding)
    if cin % 64 or cout % 64 or cin <= 0 or cout <= 0:
        return "Cin %% 64 == 0 and Cout %% 64 == 0 are required (got Cin=%d, Cout=%d)" % (cin, cout)
    return None


def _device():
    if not torch.cuda.is_available():
        raise SSGError("ssg_amd.conv needs a GPU (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _zeros(dev, n):
    """the zero bias vector the convolution kernel reads (it dereferences `bias` unconditionally)"""
    return torch.zeros(n, dtype=torch.float32, device=dev)


def _pack(L, w, want_fwd, want_dgrad):
    cout, cin, kh, kw = w.shape
    wf = torch.empty((cout, kh * kw * cin), dtype=torch.float32, device=w.device) if want_fwd else None
    wd = torch.empty((cin, kh * kw * cout), dtype=torch.float32, device=w.device) if want_dgrad else None
    s = w.stride()
    check(L.ssg_conv_pack_train_f32(ptr(w), s[0], s[1], s[2], s[3], cout, cin, kh, kw, ptr(wf), ptr(wd), stream()), "ssg_conv_pack_train_f32")
    return wf, wd


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        dev = _device()
        L = _lib.lib()
        xd = x.detach().to(dev, torch.float32).contiguous(memory_format=CL)
        w = weight.detach().to(dev, torch.float32)
        B, cin, H, W = xd.shape
        cout, _, kh, kw = w.shape
        wf, _ = _pack(L, w, True, False)
        y = torch.empty((B, cout, H, W), dtype=torch.float32, device=dev, memory_format=CL)
        check(L.ssg_conv2d_nhwc_f32(ptr(xd), ptr(wf), ptr(_zeros(dev, cout)), None, ptr(y), B, H, W, cin, cout, kh, kw, 1, kh // 2, 0, stream()),
              "ssg_conv2d_nhwc_f32 (forward)")
        ctx.save_for_backward(xd, w)
        ctx.src = tuple((t.device, t.dtype) for t in (x, weight))
        return y

    @staticmethod
    @once_differentiable                              # a double backward raises
    def backward(ctx, gy):
        xd, w = ctx.saved_tensors
        dev = xd.device
        L = _lib.lib()
        B, cin, H, W = xd.shape
        cout, _, kh, kw = w.shape
        g = gy.to(dev, torch.float32).contiguous(memory_format=CL)
        (xdev, xdt), (wdev, wdt) = ctx.src
        dx = dw = None
        if ctx.needs_input_grad[0]:
            _, wd = _pack(L, w, False, True)
            dx = torch.empty((B, cin, H, W), dtype=torch.float32, device=dev, memory_format=CL)
            check(L.ssg_conv2d_nhwc_f32(ptr(g), ptr(wd), ptr(_zeros(dev, cin)), None, ptr(dx), B, H, W, cout, cin, kh, kw, 1, kh // 2, 0, stream()),
                  "ssg_conv2d_nhwc_f32 (data gradient)")
            dx = dx.to(device=xdev, dtype=xdt)
        if ctx.needs_input_grad[1]:
            nws = L.ssg_conv_wgrad_workspace_bytes(B * H * W, cout, kh, kw, cin)
            if nws == 0:
                raise ValueError("conv2d_train: %s" % L.ssg_last_error().decode("utf-8", "replace"))
            ws = torch.empty(nws // 4, dtype=torch.float32, device=dev)
            dw = torch.empty_like(w)                  # preserve_format: the weight's strides (contiguous or channels_last)
            s = dw.stride()
            check(L.ssg_conv_wgrad_f32(ptr(g), ptr(xd), B, H, W, cin, cout, kh, kw, ptr(dw), s[0], s[1], s[2], s[3], ptr(ws), nws, 3, stream()),
                  "ssg_conv_wgrad_f32")
            dw = dw.to(device=wdev, dtype=wdt)
        return dx, dw


def conv2d_train(x, weight, stride=1, padding=0, dilation=1, groups=1, bias=None):
    """`F.conv2d(x, weight, None, stride, padding)` for the device class (see the module docstring) as one differentiable function on the
    current GPU.  x [B, Cin, H, W] and weight [Cout, Cin, KH, KW] float32; a `channels_last` x is used as it is, anything else is made
    `channels_last` first.  y and dX come back `channels_last`, dW in the weight's shape and memory format.  When x does not require
    grad the data gradient is skipped, when weight does not the weight gradient is.  A shape outside the class raises ValueError
    naming the rule; a double backward raises.  No host read, no synchronisation."""
    if x.dim() != 4 or weight.dim() != 4:
        raise ValueError("conv2d_train: x must be [B, Cin, H, W] and weight [Cout, Cin, KH, KW] (got %r, %r)" % (tuple(x.shape), tuple(weight.shape)))
    cout, cin_w, kh, kw = weight.shape
    why = unsupported_reason(x.shape[1] if groups == 1 else cin_w * groups, cout, (kh, kw), stride, padding, dilation, groups, bias is not None)
    if why is None and x.shape[1] != cin_w:
        why = "x has %d channels, the weight takes %d" % (x.shape[1], cin_w)
    if why is None and (x.shape[0] < 1 or x.shape[2] < 1 or x.shape[3] < 1):
        why = "the input is empty %r" % (tuple(x.shape),)
    if why is None and (x.dtype != torch.float32 or weight.dtype != torch.float32):
        why = "x and weight must be float32 (got %s, %s)" % (x.dtype, weight.dtype)
    if why is not None:
        raise ValueError("conv2d_train: " + why)
    return _Conv2dFn.apply(x, weight)


class Conv2d(nn.Conv2d):
    """nn.Conv2d (same parameter and state-dict key) whose forward, data gradient and weight gradient run on the HIP kernels, in train
    and in eval mode.  Only the device class can be built; the output is `channels_last`."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=False, padding_mode="zeros", **kw):
        why = unsupported_reason(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode)
        if why is not None:
            raise ValueError("ssg_amd.Conv2d: " + why)
        super(Conv2d, self).__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, **kw)

    def forward(self, input):
        return conv2d_train(input, self.weight, self.stride, self.padding)


def _module_reason(m):
    return unsupported_reason(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, m.dilation, m.groups, m.bias is not None, m.padding_mode)


def _adopt(old):
    """the device module in place of `old`, holding the same Parameter object"""
    new = Conv2d(old.in_channels, old.out_channels, old.kernel_size, old.stride, old.padding, device="meta")
    new._parameters["weight"] = old._parameters["weight"]
    new.training = old.training
    return new


def _adopt_strided(old):
    from .conv_strided import StridedConv2d
    new = StridedConv2d(old.in_channels, old.out_channels, old.kernel_size, old.stride, old.padding, device="meta")
    new._parameters["weight"] = old._parameters["weight"]
    new.training = old.training
    return new


def use_device_conv(model, strided=False):
    """Replace every `nn.Conv2d` of the device class in `model` (also under nn.DataParallel: the walk goes through `.module`) by
    `ssg_amd.Conv2d`.  The Parameter objects are kept, so optimiser groups built before the call and the state-dict keys stay valid.
    The qualified names of the convolutions left alone (strided, 7x7, with a bias, ..., and other subclasses of nn.Conv2d) are listed
    in `model._ssg_conv_skipped`.  `strided=True` also swaps the stride-2 1x1 / 3x3 convolutions and the 7x7 stem for
    `ssg_amd.StridedConv2d` (ssg_amd/conv_strided.py), which leaves none of a ResNet's convolutions on the skipped list; a later call
    without the keyword leaves those modules where they are and does not list them.  Run the model
    on `channels_last` input (`model.to(memory_format=torch.channels_last)`) so that no layout copy is made between the layers.
    Returns the model."""
    skipped = []
    if strided:
        from .conv_strided import strided_unsupported_reason

        def strided_ok(m):
            return strided_unsupported_reason(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, m.dilation, m.groups,
                                              m.bias is not None, m.padding_mode) is None

    def walk(parent, prefix):
        for name, child in list(parent._modules.items()):
            if child is None:
                continue
            full = prefix + name
            if isinstance(child, Conv2d) or getattr(child, "_ssg_device_conv", False):     # already on the device path (either class)
                continue
            if isinstance(child, nn.Conv2d):
                if type(child) is nn.Conv2d and _module_reason(child) is None and child.weight.dtype == torch.float32:
                    parent._modules[name] = _adopt(child)
                elif strided and type(child) is nn.Conv2d and strided_ok(child) and child.weight.dtype == torch.float32:
                    parent._modules[name] = _adopt_strided(child)
                else:
                    skipped.append(full)
                continue
            walk(child, full + ".")

    if type(model) is nn.Conv2d:
        raise ValueError("use_device_conv: pass the model that holds the convolution, not the convolution itself")
    walk(model, "")
    model._ssg_conv_skipped = skipped
    return model
