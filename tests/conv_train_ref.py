"""Yardstick of the train-mode Conv2d tests (tests/test_conv_train_host.py, tests/test_gpu_conv_train.py): seeded cases, torch's
`F.conv2d` and its autograd in float64 on the CPU for y, dX and dW, the absolute-value companion A of each output (the same
convolution or gradient applied to |x|, |w| and |dY|), and a torch restatement of the two weight packings of csrc/conv_train.hip."""
from functools import lru_cache

import torch
import torch.nn.functional as Fn

from train_common import U, bound  # noqa: F401 (the unit roundoff and the (L + 2) 2^-24 A bound, under this module's names too)

# name -> (B, H, W, Cin, Cout, k, seed).  The multi-slice cases take their B from ssg_conv_wgrad_num_slices (see multi_slice_batch).
CASES = {
    "1x1_ragged": (2, 5, 3, 64, 64, 1, 201),        # M = 30: a ragged row tile
    "3x3_border": (2, 5, 3, 64, 64, 3, 202),        # every border tap on a non-square image
    "3x3_1px": (1, 1, 1, 64, 64, 3, 203),           # only the centre tap is in range
    "3x3_cout192": (2, 4, 4, 64, 192, 3, 204),      # Cout no multiple of 128, several Cout tiles
    "3x3_cin192": (2, 4, 4, 192, 64, 3, 205),       # the tile roles swapped for dgrad, six 32-channel chunks
}
MULTI = {"multi_1x1": (8, 4, 64, 64, 1, 206), "multi_3x3": (8, 4, 64, 64, 3, 207)}   # (H, W, Cin, Cout, k, seed)


def _real():
    """one case per distinct stride-1 (Cin, Cout, k) of torchvision's ResNet-50 at a 256 x 128 input: the real channel pair on the real
    row width W, with B and H chosen so that 512 < M = B H W < 768 and M is no multiple of 128 or of 3 -- three weight-gradient slices
    that cannot be equal, so the last is shorter, and a ragged last 128-row tile in the forward and the data gradient (asserted from the library's slice
    count in test_gpu_conv_train.py::test_real_cases_have_three_slices_and_ragged_tiles)"""
    rows = {32: (2, 11), 16: (5, 7), 8: (7, 11), 4: (19, 8)}                    # W -> (B, H): M = 704, 560, 616, 608, no multiple of 3
    layers = [(1, 32, [(64, 64), (64, 256), (256, 64), (256, 128)]), (1, 16, [(128, 512), (512, 128), (512, 256)]),
              (1, 8, [(256, 1024), (1024, 256), (1024, 512)]), (1, 4, [(512, 2048), (2048, 512)]),
              (3, 32, [(64, 64)]), (3, 16, [(128, 128)]), (3, 8, [(256, 256)]), (3, 4, [(512, 512)])]
    out, seed = {}, 220
    for k, W, pairs in layers:
        for cin, cout in pairs:
            out["real_%dx%d_%d_%d" % (k, k, cin, cout)] = rows[W] + (W, cin, cout, k, seed)
            seed += 1
    return out


REAL = _real()

# layer1's two 1x1 shapes at the trainer's own batch: name -> (B, H, W, Cin, Cout, seed), M = 131072
TRAINER = {"trainer_256_64": (64, 64, 32, 256, 64, 251), "trainer_64_256": (64, 64, 32, 64, 256, 252)}


def make_case(B, H, W, cin, cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float32)
    w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float32) * (1.0 / (cin * k * k) ** 0.5)
    gy = torch.randn(B, cout, H, W, generator=g, dtype=torch.float32)
    return dict(x=x, w=w, gy=gy, k=k, pad=k // 2)


def outputs(x, w, gy, pad, dtype):
    """{y, dx, dw} of F.conv2d(stride 1) and its autograd in `dtype` on the CPU"""
    x = x.to(dtype).clone().requires_grad_(True)
    w = w.to(dtype).clone().requires_grad_(True)
    y = Fn.conv2d(x, w, None, 1, pad)
    dx, dw = torch.autograd.grad(y, (x, w), gy.to(dtype))
    return dict(y=y.detach(), dx=dx, dw=dw)


@lru_cache(maxsize=None)
def reference(B, H, W, cin, cout, k, seed):
    """(case, ref64 {y, dx, dw}, A {y, dx, dw}, L {y, dx, dw}) -- computed once, never modified"""
    d = make_case(B, H, W, cin, cout, k, seed)
    ref = outputs(d["x"], d["w"], d["gy"], d["pad"], torch.float64)
    A = outputs(d["x"].abs(), d["w"].abs(), d["gy"].abs(), d["pad"], torch.float64)
    L = dict(y=k * k * cin, dx=k * k * cout, dw=B * H * W)
    return d, ref, A, L


def pack_fwd(w):
    """[Cout,Cin,KH,KW] -> w_fwd [Cout][KH*KW*Cin], k = ((ci/32)*KH*KW + r*KW + s)*32 + ci%32"""
    cout, cin, kh, kw = w.shape
    return w.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin // 32, 32).permute(0, 2, 1, 3).reshape(cout, kh * kw * cin).contiguous()


def pack_dgrad(w):
    """[Cout,Cin,KH,KW] -> w_dgrad [Cin][KH*KW*Cout]: transposed in (Cout, Cin), taps (KH-1-r, KW-1-s), the same K order over Cout"""
    return pack_fwd(w.flip(2, 3).transpose(0, 1))


def im2col_packed(x, k):
    """x [B,C,H,W] -> [B*H*W, k*k*C] in the packed K order, stride 1, pad k//2 (zeros outside the image)"""
    B, C, H, W = x.shape
    p = k // 2
    xp = Fn.pad(x, (p, p, p, p))
    taps = [xp[:, :, r:r + H, s:s + W] for r in range(k) for s in range(k)]          # each [B,C,H,W]
    t = torch.stack(taps, 0).permute(1, 3, 4, 0, 2)                                    # [B,H,W,tap,C]
    return t.reshape(B * H * W, k * k, C // 32, 32).permute(0, 2, 1, 3).reshape(B * H * W, k * k * C)


def multi_slice_batch(L, H, W, cin, cout, k):
    """smallest B <= 64 at which the weight gradient is cut into at least three slices (None: there is none)"""
    for B in range(1, 65):
        if L.ssg_conv_wgrad_num_slices(B * H * W, cout, k, k, cin) >= 3:
            return B
    return None


@lru_cache(maxsize=1)
def gemm_reference(name):
    """(case, ref64 {y, dx, dw}, A {y, dx, dw}) of a TRAINER case.  A 1x1 convolution is a GEMM over the M = B H W pixels, so the
    reference is three float64 matmuls (three more on absolute values for A) on the NHWC pixel matrices: x [M, Cin], w [Cout, Cin],
    gy [M, Cout] -> y [M, Cout] = x w^T, dx [M, Cin] = gy w, dw [Cout, Cin] = gy^T x.  Only the last one is kept (hundreds of MB).

    The data are what these layers see: x = max(N(0, 1), 0), the output of the ReLU in front of the layer, and gy = N(0, 1) with
    half of its elements zeroed, a gradient that came back through a ReLU.  Dense N(0, 1) data would leave the slice-aware dW bound
    too blunt at 256 -> 64 (a missing 32-pixel stage seen on 0.64 of dW; tests/test_conv_train_host.py asks for 3/4): the terms of a
    sparse sum are larger against their mean absolute value, which is what A measures."""
    B, H, W, cin, cout, seed = TRAINER[name]
    M = B * H * W
    g = torch.Generator().manual_seed(seed)
    d = dict(x=torch.randn(M, cin, generator=g).clamp_(min=0), w=torch.randn(cout, cin, generator=g) * (1.0 / cin ** 0.5),
             gy=torch.randn(M, cout, generator=g) * (torch.rand(M, cout, generator=g) < 0.5))

    def gemms(x, w, gy):
        return dict(y=x @ w.t(), dx=gy @ w, dw=gy.t() @ x)
    return (d, gemms(d["x"].double(), d["w"].double(), d["gy"].double()),
            gemms(d["x"].double().abs(), d["w"].double().abs(), d["gy"].double().abs()))


def slice_length_bound(M, n):
    """an upper bound on the length of the weight gradient's slices, from the public slice count n alone: n - 1 full slices of equal
    length leave at least one pixel to the last, (n - 1) len < M, hence len <= ceil(M / (n - 1)); one slice is all of M"""
    return M if n <= 1 else -(-M // (n - 1))


class Bottleneck(torch.nn.Module):
    """a block with the attribute shape of torchvision's Bottleneck (torchvision is not installed)"""

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        nn = torch.nn
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        residual = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + residual)


def downsample(inplanes, outplanes, stride):
    nn = torch.nn
    return nn.Sequential(nn.Conv2d(inplanes, outplanes, 1, stride=stride, bias=False), nn.BatchNorm2d(outplanes))
