"""Yardstick of the strided train-mode Conv2d and max-pool tests (tests/test_conv_strided_host.py, tests/test_gpu_conv_strided.py,
tests/test_gpu_maxpool_train.py): seeded cases, torch's `F.conv2d` / `F.max_pool2d` and their autograd in float64 on the CPU, and the
absolute-value companion A of each output.  The bound, the unit roundoff and the model blocks come from tests/conv_train_ref.py."""
from functools import lru_cache

import torch
import torch.nn.functional as Fn

from conv_train_ref import Bottleneck, downsample  # noqa: F401
from train_common import U, bound  # noqa: F401

# name -> (B, H, W, Cin, Cout, k, seed); stride 2, pad k // 2.  The smallest shapes at which each thing can go wrong.
CASES = {
    "1x1_odd": (2, 5, 3, 64, 64, 1, 301),           # odd sides
    "1x1_even": (2, 4, 6, 64, 128, 1, 302),         # even sides: the last row / column of dX and the three empty classes are exactly 0
    "1x1_1px": (1, 1, 1, 64, 64, 1, 303),           # smallest
    "3x3_odd": (2, 5, 3, 64, 64, 3, 304),           # odd sides
    "3x3_even": (2, 4, 6, 64, 64, 3, 305),          # even: the r = 2 tap of the last output row reads the padding
    "3x3_1px": (1, 1, 1, 64, 64, 3, 306),           # centre tap only
    "3x3_2rows": (1, 2, 1, 64, 64, 3, 307),         # minimal with a second row
    "3x3_cout192": (2, 4, 4, 64, 192, 3, 308),      # several Cout tiles
    "3x3_cin192": (2, 4, 4, 192, 64, 3, 309),       # Cin chunking
    "stem_odd": (2, 9, 5, 3, 64, 7, 310),           # odd sides
    "stem_even": (1, 8, 4, 3, 64, 7, 311),          # even sides
    "stem_clipped": (1, 3, 3, 3, 64, 7, 312),       # image smaller than the kernel: every window is clipped
}
# one multi-slice case per weight-gradient kernel (H, W, Cin, Cout, k, seed); B comes from ssg_conv_wgrad_strided_num_slices.
# 8 x 8 input -> 16 output pixels per image, so that a ragged third slice appears at a B <= 64 with the 256-pixel slice floor
MULTI = {"multi_1x1": (8, 8, 64, 64, 1, 313), "multi_3x3": (8, 8, 64, 128, 3, 314), "multi_stem": (8, 8, 3, 64, 7, 315)}
# one case per distinct stride-2 (Cin, Cout, k) of torchvision's ResNet-50 at a 256 x 128 input: the real channel pair on the real
# input row width, even sides (the real parity), B and H chosen so that the output pixels M = B OH OW give 512 < M < 768 with M no
# multiple of 64: three weight-gradient slices of which the last is shorter, a ragged last 128-row tile in the forward, and in each
# parity class of dX (M pixels each) a ragged last 64-pixel tile (test_gpu_conv_strided.py::test_real_cases_have_three_slices_and_ragged_tiles)
REAL = {
    "real_3x3_128_128": (5, 14, 32, 128, 128, 3, 320),       # M = 5 * 7 * 16 = 560
    "real_3x3_256_256": (11, 14, 16, 256, 256, 3, 321),      # M = 11 * 7 * 8 = 616
    "real_3x3_512_512": (19, 16, 8, 512, 512, 3, 322),       # M = 19 * 8 * 4 = 608
    "real_1x1_256_512": (5, 14, 32, 256, 512, 1, 323),
    "real_1x1_512_1024": (11, 14, 16, 512, 1024, 1, 324),
    "real_1x1_1024_2048": (19, 16, 8, 1024, 2048, 1, 325),
}
DOWNSAMPLE = ("real_1x1_256_512", "real_1x1_512_1024", "real_1x1_1024_2048")


def out_hw(H, W, k):
    p = k // 2
    return (H + 2 * p - k) // 2 + 1, (W + 2 * p - k) // 2 + 1


def make_case(B, H, W, cin, cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    OH, OW = out_hw(H, W, k)
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float32)
    w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float32) * (1.0 / (cin * k * k) ** 0.5)
    gy = torch.randn(B, cout, OH, OW, generator=g, dtype=torch.float32)
    return dict(x=x, w=w, gy=gy, k=k, pad=k // 2)


def outputs(x, w, gy, pad, dtype):
    """{y, dx, dw} of F.conv2d(stride 2) and its autograd in `dtype` on the CPU"""
    x = x.to(dtype).clone().requires_grad_(True)
    w = w.to(dtype).clone().requires_grad_(True)
    y = Fn.conv2d(x, w, None, 2, pad)
    dx, dw = torch.autograd.grad(y, (x, w), gy.to(dtype))
    return dict(y=y.detach(), dx=dx, dw=dw)


@lru_cache(maxsize=None)
def reference(B, H, W, cin, cout, k, seed):
    """(case, ref64 {y, dx, dw}, A {y, dx, dw}, L {y, dx, dw}) -- computed once, never modified"""
    d = make_case(B, H, W, cin, cout, k, seed)
    ref = outputs(d["x"], d["w"], d["gy"], d["pad"], torch.float64)
    A = outputs(d["x"].abs(), d["w"].abs(), d["gy"].abs(), d["pad"], torch.float64)
    OH, OW = out_hw(H, W, k)
    L = dict(y=k * k * cin, dx=k * k * cout, dw=B * OH * OW)
    return d, ref, A, L


def pack_dgrad_s2(w):
    """[Cout,Cin,KH,KW] -> the strided data gradient's packing [KH*KW][Cout][Cin] (tap r*KW + s outermost, Cin contiguous)"""
    cout, cin, kh, kw = w.shape
    return w.permute(2, 3, 0, 1).reshape(kh * kw, cout, cin).contiguous()


def multi_slice_batch(L, H, W, cin, cout, k):
    """smallest B <= 64 at which the strided weight gradient is cut into at least three slices that cannot be equal (None: none)"""
    OH, OW = out_hw(H, W, k)
    for B in range(1, 65):
        n = L.ssg_conv_wgrad_strided_num_slices(B * OH * OW, cout, k, k, cin, 2)
        if n >= 3 and (B * OH * OW) % n != 0:
            return B
    return None


# ---- max-pool ------------------------------------------------------------------------------------------------------------------------------

def pool_input(name):
    """x [B, C, H, W] float32 of a named max-pool case"""
    g = torch.Generator().manual_seed({"odd": 401, "even": 402, "1px": 403, "relu": 404, "dup": 405}[name])
    if name == "odd":
        return torch.randn(2, 64, 5, 3, generator=g)
    if name == "even":
        return torch.randn(2, 64, 4, 6, generator=g)
    if name == "1px":
        return torch.randn(1, 4, 1, 1, generator=g)
    if name == "relu":                                   # whole windows tie at 0
        return torch.relu(torch.randn(2, 64, 6, 5, generator=g))
    # "dup": few distinct positive values, so that a maximum repeats inside one window and across overlapping windows
    return torch.randint(1, 4, (2, 8, 7, 6), generator=g).float()


POOL_CASES = ("odd", "even", "1px", "relu", "dup")


@lru_cache(maxsize=None)
def pool_reference(name):
    """(x, gy, y32 of F.max_pool2d in float32, dx64 of the float64 autograd, A = the same gather of |gy|)"""
    x = pool_input(name)
    y32 = Fn.max_pool2d(x, 3, 2, 1)
    gy = torch.randn(y32.shape, generator=torch.Generator().manual_seed(499))
    outs = []
    for g in (gy.double(), gy.double().abs()):
        xd = x.double().clone().requires_grad_(True)
        (dx,) = torch.autograd.grad(Fn.max_pool2d(xd, 3, 2, 1), xd, g)
        outs.append(dx)
    return x, gy, y32, outs[0], outs[1]
