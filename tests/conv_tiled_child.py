"""Child process of tests/test_conv_tiled_weights.py: every kernel case through ssg_conv2d_nhwc_xt / ssg_conv1x1_dual_nhwc_xt, once with
the tiled weight copy and once with wt = NULL, under the routing knobs of the parent's environment (the library caches them per process).
Prints one JSON object: case -> {out: same bits, flag: same range flag, flag_value, nonzero: the output is not all zero}."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ssg_amd import _lib, resnet            # noqa: E402
from ssg_amd._lib import check, ptr, stream  # noqa: E402

B = 3       # layer3 shapes: M = 3 * 16 * 8 = 384, one full 256-row tile and a ragged one (three 128-row tiles)
# name: (H, W, Cin, Cout, k, stride, pad, residual, second input (H2, W2, Cin2, stride2) or None, bias spike)
CASES = {
    "1x1_1024_256": (16, 8, 1024, 256, 1, 1, 0, False, None, 0.0),
    "3x3_256_256_pad1": (16, 8, 256, 256, 3, 1, 1, False, None, 0.0),
    "3x3_s2_128_128": (32, 16, 128, 128, 3, 2, 1, False, None, 0.0),
    "1x1_256_1024_res": (16, 8, 256, 1024, 1, 1, 0, True, None, 0.0),
    "dual_256_512_1024_s2": (16, 8, 256, 1024, 1, 1, 0, False, (32, 16, 512, 2), 0.0),
    "1x1_64_256_short": (16, 8, 64, 256, 1, 1, 0, False, None, 0.0),
    "1x1_1024_256_out_of_range": (16, 8, 1024, 256, 1, 1, 0, False, None, 1.0e5),      # the range flag goes up on both paths
}


def h8l8(t):
    return resnet._h8l8(t.reshape(-1, t.shape[-1])).reshape(t.shape)


def run(L, dev, g, spec):
    H, W, Cin, Cout, k, stride, pad, use_res, second, spike = spec
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x = h8l8(torch.randn(B, H, W, Cin, generator=g)).to(dev)
    kp = k * k * Cin + (second[2] if second else 0)
    wf = torch.randn(Cout, kp, generator=g) * (2.0 / kp) ** 0.5
    sc = resnet._row_scales(wf)
    w = h8l8(wf * sc.view(-1, 1)).to(dev).contiguous()
    cs = (1.0 / sc).contiguous().to(dev)
    bias = torch.randn(Cout, generator=g) * 0.1
    bias[3] += spike
    bias = bias.to(dev)
    res = h8l8(torch.randn(B, OH, OW, Cout, generator=g)).to(dev) if use_res else None
    x2 = h8l8(torch.randn(B, second[0], second[1], second[2], generator=g)).to(dev) if second else None
    wt = torch.empty_like(w)
    assert L.ssg_conv_weights_tile(ptr(w), Cout, kp, ptr(wt), stream()) == 1
    got = []
    for t in (wt, None):
        out = torch.full((B, OH, OW, Cout), float("nan"), device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        if second:
            check(L.ssg_conv1x1_dual_nhwc_xt(ptr(x), ptr(x2), ptr(w), ptr(t), ptr(bias), ptr(out), B, H, W, Cin, second[0], second[1], second[2], second[3],
                                             Cout, 1, 3, 1.0, ptr(cs), ptr(flag), stream()), "ssg_conv1x1_dual_nhwc_xt")
        else:
            check(L.ssg_conv2d_nhwc_xt(ptr(x), ptr(w), ptr(t), ptr(bias), ptr(res), ptr(out), B, H, W, Cin, Cout, k, k, stride, pad, 1, 3, 1.0,
                                       ptr(cs), ptr(flag), stream()), "ssg_conv2d_nhwc_xt")
        got.append((out.view(torch.int32), flag))
    (o1, f1), (o0, f0) = got
    return {"out": bool(torch.equal(o1, o0)), "flag": bool(torch.equal(f1, f0)), "flag_value": int(f1.item()), "nonzero": bool((o1 != 0).any().item())}


def main():
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    g = torch.Generator().manual_seed(7)
    print(json.dumps({name: run(L, dev, g, spec) for name, spec in CASES.items()}))


if __name__ == "__main__":
    main()
