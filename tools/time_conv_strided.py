#!/usr/bin/env python3
"""Write profiles/conv_strided_times.txt (run on the MI355X, e.g. `timeout -k 10 900 python tools/time_conv_strided.py`): forward +
backward of the seven strided convolutions of ResNet-50 and of its max-pool at B = 128 images of 256 x 128, two implementations in one
process on channels_last float32 input, run alternately:

  (a) torch    nn.Conv2d / nn.MaxPool2d (the vendor library's kernels; torch's own pool)
  (b) device   ssg_amd.StridedConv2d / ssg_amd.MaxPool2d (csrc/conv_strided.hip)

One call = forward, then torch.autograd.grad of y with a fixed upstream gradient towards x (not for the stem: the images do not require
grad) and the weight.  Every call is timed on its own with events; a round takes the median of CALLS calls of each implementation in
turn, ROUNDS rounds; the table shows the median of the round medians and their min-max (the spread).  A side wins a shape when its
median is lower by more than the larger of the two spreads, else the line says "tie"."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from _timing import CELL, rounds, verdict  # noqa: E402 (tools/ is the script's own directory)

B = 128
CALLS, ROUNDS, WARMUP = 5, 7, 3
# (Cin, Cout, k, H, W, where) -- the stride-2 convolutions of torchvision's ResNet-50 at 256 x 128 input (H x W: the layer's input)
SHAPES = [
    (3, 64, 7, 256, 128, "conv1"),
    (128, 128, 3, 64, 32, "layer2.0.conv2"),
    (256, 256, 3, 32, 16, "layer3.0.conv2"),
    (512, 512, 3, 16, 8, "layer4.0.conv2"),
    (256, 512, 1, 64, 32, "layer2.0.downsample.0"),
    (512, 1024, 1, 32, 16, "layer3.0.downsample.0"),
    (1024, 2048, 1, 16, 8, "layer4.0.downsample.0"),
]
POOL = (64, 128, 64, "maxpool")


def main():
    import torch
    from torch import nn
    import ssg_amd
    from ssg_amd import _lib
    L = _lib.lib()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "conv_strided_times.txt")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    CL = torch.channels_last
    lines = ["strided train-mode Conv2d / MaxPool2d(3, 2, 1) forward + backward per call at B = %d, %s, float32 channels_last; median (min-max) over %d "
             "rounds of the median of %d calls, implementations interleaved" % (B, torch.cuda.get_device_name(0), ROUNDS, CALLS),
             "(a) torch nn.Conv2d / nn.MaxPool2d  (b) ssg_amd.StridedConv2d / ssg_amd.MaxPool2d;  slices = cuts of the weight gradient's pixel range",
             "%-24s %-22s %26s %26s %6s %-7s %6s" % ("where", "Cin>Cout k HxW", "(a) ms", "(b) ms", "a / b", "winner", "slices")]
    wins = {"torch": 0, "device": 0, "tie": 0}

    def report(where, what, a, b, n):
        winner = verdict(a, b, "torch", "device")
        wins[winner] += 1
        lines.append("%-24s %-22s %26s %26s %6.2f %-7s %6s" % (where, what, CELL % a, CELL % b, a[0] / b[0], winner, n))
        print(lines[-1], flush=True)

    for cin, cout, k, H, W, where in SHAPES:
        stem = k == 7
        x = torch.randn((B, cin, H, W), device=dev, generator=g).contiguous(memory_format=CL).requires_grad_(not stem)
        ref = nn.Conv2d(cin, cout, k, 2, k // 2, bias=False).to(dev).to(memory_format=CL)
        mine = ssg_amd.StridedConv2d(cin, cout, k, 2, k // 2).to(dev).to(memory_format=CL)
        with torch.no_grad():
            mine.weight.copy_(ref.weight)
            OH, OW = ref(x).shape[2:]
        gy = torch.randn((B, cout, OH, OW), device=dev, generator=g).contiguous(memory_format=CL)
        a, b = rounds([lambda: torch.autograd.grad(ref(x), [ref.weight] if stem else [x, ref.weight], gy),
                       lambda: torch.autograd.grad(mine(x), [mine.weight] if stem else [x, mine.weight], gy)], CALLS, ROUNDS, WARMUP)
        report(where, "%d>%d %dx%d %dx%d" % (cin, cout, k, k, H, W), a, b, L.ssg_conv_wgrad_strided_num_slices(B * OH * OW, cout, k, k, cin, 2))
        del x, gy, ref, mine
        torch.cuda.empty_cache()
    C, H, W, where = POOL
    x = torch.randn((B, C, H, W), device=dev, generator=g).contiguous(memory_format=CL).requires_grad_(True)
    gy = torch.randn((B, C, H // 2, W // 2), device=dev, generator=g).contiguous(memory_format=CL)
    ref, mine = nn.MaxPool2d(3, 2, 1), ssg_amd.MaxPool2d()
    a, b = rounds([lambda: torch.autograd.grad(ref(x), [x], gy), lambda: torch.autograd.grad(mine(x), [x], gy)], CALLS, ROUNDS, WARMUP)
    report(where, "%d 3x3 %dx%d" % (C, H, W), a, b, "-")
    lines.append("of %d shapes: torch faster on %d, the device path faster on %d, within the spread on %d.  The feature is opt-in whatever this says."
                 % (len(SHAPES) + 1, wins["torch"], wins["device"], wins["tie"]))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])


if __name__ == "__main__":
    main()
