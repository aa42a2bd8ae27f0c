"""Child process of tests/test_conv_line_fetch.py.  `kernels`: every case through ssg_conv2d_nhwc_xt / ssg_conv1x1_dual_nhwc_xt under the
routing knobs and the SSG_CONV_LINE of the parent's environment (the library caches them per process); `embed`: the ResNet-50 embedder
before and after refresh().  Prints one JSON object: case -> {sha: digest of the output bits, flag: range flag, nonzero}."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ssg_amd                               # noqa: E402
from ssg_amd import _lib, resnet            # noqa: E402
from ssg_amd._lib import check, ptr, stream  # noqa: E402

# name: (B, H, W, Cin, Cout, k, stride, pad, residual, second input (H2, W2, Cin2, stride2) or None, bias spike); M = 384 unless the name says so
CASES = {
    "c1_1x1_32_256": (3, 16, 8, 32, 256, 1, 1, 0, False, None, 0.0),                    # nk = 2: one pair, shorter than every ring
    "c2_1x1_96_256": (3, 16, 8, 96, 256, 1, 1, 0, False, None, 0.0),                    # nk = 6: leftovers for four stages, two trips for three
    "c3_1x1_1024_256_m300": (3, 10, 10, 1024, 256, 1, 1, 0, False, None, 0.0),          # ragged last tile, rows behind M
    "c3_1x1_1024_256_m300_out_of_range": (3, 10, 10, 1024, 256, 1, 1, 0, False, None, 1.0e5),   # hi halves beyond the half range: the flag
    "c4_3x3_32_256_pad1_4x4": (24, 4, 4, 32, 256, 3, 1, 1, False, None, 0.0),           # nk = 18; padding taps are zero in both halves of a pair
    "c5_3x3_s2_64_128": (24, 8, 8, 64, 128, 3, 2, 1, False, None, 0.0),                 # strided taps
    "c6_1x1_64_256_res": (3, 16, 8, 64, 256, 1, 1, 0, True, None, 0.0),                 # straight-line epilogue with a residual
    "c7_dual_64_32_s2_256": (3, 16, 8, 64, 256, 1, 1, 0, False, (32, 16, 32, 2), 0.0),  # input boundary at an even k-tile
    # K >= 128, so that the wide / tall routing puts these two on the 128 x 256 and 256 x 256 instances (K < 128 runs on 128 x 128 tiles)
    "x1_1x1_128_256_res": (3, 16, 8, 128, 256, 1, 1, 0, True, None, 0.0),
    "x2_dual_96_32_s2_256": (3, 16, 8, 96, 256, 1, 1, 0, False, (32, 16, 32, 2), 0.0),  # nk = 8, the second input starts at k-tile 6
    "x3_3x3_64_256_pad1_4x4": (24, 4, 4, 64, 256, 3, 1, 1, False, None, 0.0),           # nk = 36: six full trips of three stages, nine of four
    "x4_1x1_160_256": (3, 16, 8, 160, 256, 1, 1, 0, False, None, 0.0),                  # nk = 10: four left-over steps behind one six-step trip
}


def h8l8(t):
    return resnet._h8l8(t.reshape(-1, t.shape[-1])).reshape(t.shape)


def digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def run(L, dev, spec, seed):
    g = torch.Generator().manual_seed(seed)
    B, H, W, Cin, Cout, k, stride, pad, use_res, second, spike = spec
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
    out = torch.full((B, OH, OW, Cout), float("nan"), device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if second:
        check(L.ssg_conv1x1_dual_nhwc_xt(ptr(x), ptr(x2), ptr(w), ptr(wt), ptr(bias), ptr(out), B, H, W, Cin, second[0], second[1], second[2], second[3],
                                         Cout, 1, 3, 1.0, ptr(cs), ptr(flag), stream()), "ssg_conv1x1_dual_nhwc_xt")
    else:
        check(L.ssg_conv2d_nhwc_xt(ptr(x), ptr(w), ptr(wt), ptr(bias), ptr(res), ptr(out), B, H, W, Cin, Cout, k, k, stride, pad, 1, 3, 1.0,
                                   ptr(cs), ptr(flag), stream()), "ssg_conv2d_nhwc_xt")
    bits = out.view(torch.int32)
    return {"sha": digest(bits), "flag": int(flag.item()), "nonzero": bool((bits != 0).any().item())}


def embed():
    model = ssg_amd.create("resnet50", num_classes=0, num_split=1, cluster=False, seed=1, pretrained=False, precision="split").cuda().eval()
    imgs = torch.randn(3, 3, 64, 32, generator=torch.Generator().manual_seed(5))
    first = model.embed_with_flip(imgs)
    model.refresh(ssg_amd.synthetic_state_dict(seed=2))
    second = model.embed_with_flip(imgs)
    fin = bool(torch.isfinite(first).all().item() and torch.isfinite(second).all().item())
    return {"before": {"sha": digest(first.view(torch.int32)), "finite": fin}, "after": {"sha": digest(second.view(torch.int32)), "finite": fin}}


def main():
    if sys.argv[1:] == ["embed"]:
        print(json.dumps(embed()))
        return
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    print(json.dumps({name: run(L, dev, spec, 11 + i) for i, (name, spec) in enumerate(CASES.items())}))


if __name__ == "__main__":
    main()
