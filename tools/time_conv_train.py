#!/usr/bin/env python3
"""Write profiles/conv_train_times.txt (run on the MI355X, e.g. `timeout -k 10 900 python tools/time_conv_train.py`): forward + backward
of every distinct convolution shape of ResNet-50 that ssg_amd.Conv2d takes, at B = 128 images of 256 x 128 (last stride 2), two
implementations in one process on channels_last float32 input, run alternately:

  (a) torch    nn.Conv2d (the vendor library's forward, data gradient and weight gradient)
  (b) device   ssg_amd.Conv2d (pack + ssg_conv2d_nhwc_f32 forward, pack + ssg_conv2d_nhwc_f32 data gradient, ssg_conv_wgrad_f32)

One call = forward, then torch.autograd.grad of y with a fixed upstream gradient towards x and the weight.  Every call is timed on its
own with events; a round takes the median of CALLS calls of each implementation in turn, ROUNDS rounds; the table shows the median of
the round medians and their min-max (the spread).  A side wins a shape when its median is lower by more than the larger of the two
spreads, else the line says "tie".  The two stages of the weight gradient (partial tiles on the matrix cores; float64 slice sum) are
timed the same way through the entry point's `stages` argument, with the number of slices."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from _timing import CELL, rounds, verdict  # noqa: E402 (tools/ is the script's own directory)

B = 128
CALLS, ROUNDS, WARMUP = 5, 7, 3
# (Cin, Cout, k, H, W, where) -- stride-1 1x1 / 3x3 convolutions of torchvision's ResNet-50 at 256 x 128 input
SHAPES = [
    (64, 64, 1, 64, 32, "layer1.0.conv1"),
    (64, 64, 3, 64, 32, "layer1.*.conv2"),
    (64, 256, 1, 64, 32, "layer1.*.conv3, downsample"),
    (256, 64, 1, 64, 32, "layer1.1-2.conv1"),
    (256, 128, 1, 64, 32, "layer2.0.conv1"),
    (128, 512, 1, 32, 16, "layer2.*.conv3"),
    (512, 128, 1, 32, 16, "layer2.1-3.conv1"),
    (128, 128, 3, 32, 16, "layer2.1-3.conv2"),
    (512, 256, 1, 32, 16, "layer3.0.conv1"),
    (256, 1024, 1, 16, 8, "layer3.*.conv3"),
    (1024, 256, 1, 16, 8, "layer3.1-5.conv1"),
    (256, 256, 3, 16, 8, "layer3.1-5.conv2"),
    (1024, 512, 1, 16, 8, "layer4.0.conv1"),
    (512, 2048, 1, 8, 4, "layer4.*.conv3"),
    (2048, 512, 1, 8, 4, "layer4.1-2.conv1"),
    (512, 512, 3, 8, 4, "layer4.1-2.conv2"),
]


def main():
    import torch
    from torch import nn
    import ssg_amd
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "conv_train_times.txt")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    CL = torch.channels_last
    lines = ["train-mode Conv2d forward + backward (dX and dW) per call at B = %d, %s, float32 channels_last; median (min-max) over %d rounds of the "
             "median of %d calls, implementations interleaved" % (B, torch.cuda.get_device_name(0), ROUNDS, CALLS),
             "(a) torch nn.Conv2d  (b) ssg_amd.Conv2d;  wgrad stage 1 = fp32-MFMA partial tiles per slice, stage 2 = float64 slice sum",
             "%-30s %-18s %26s %26s %6s %-7s %6s %22s %22s" % ("where", "Cin>Cout k HxW", "(a) ms", "(b) ms", "a / b", "winner", "slices", "stage 1 ms",
                                                          "stage 2 ms")]
    wins = {"torch": 0, "device": 0, "tie": 0}

    for cin, cout, k, H, W, where in SHAPES:
        x = torch.randn((B, cin, H, W), device=dev, generator=g).contiguous(memory_format=CL).requires_grad_(True)
        gy = torch.randn((B, cout, H, W), device=dev, generator=g).contiguous(memory_format=CL)
        ref = nn.Conv2d(cin, cout, k, 1, k // 2, bias=False).to(dev).to(memory_format=CL)
        mine = ssg_amd.Conv2d(cin, cout, k, 1, k // 2).to(dev).to(memory_format=CL)
        with torch.no_grad():
            mine.weight.copy_(ref.weight)
        a, b = rounds([lambda: torch.autograd.grad(ref(x), [x, ref.weight], gy), lambda: torch.autograd.grad(mine(x), [x, mine.weight], gy)], CALLS, ROUNDS,
                      WARMUP)
        M = B * H * W
        n = L.ssg_conv_wgrad_num_slices(M, cout, k, k, cin)
        nws = L.ssg_conv_wgrad_workspace_bytes(M, cout, k, k, cin)
        ws = torch.empty(nws // 4, dtype=torch.float32, device=dev)
        dw = torch.empty_like(mine.weight)
        s = dw.stride()
        xd = x.detach()

        def stage(which):
            return lambda: check(L.ssg_conv_wgrad_f32(ptr(gy), ptr(xd), B, H, W, cin, cout, k, k, ptr(dw), s[0], s[1], s[2], s[3], ptr(ws), nws,
                                                      which, stream()), "ssg_conv_wgrad_f32")
        s1, s2 = rounds([stage(1), stage(2)], CALLS, ROUNDS, WARMUP)
        winner = verdict(a, b, "torch", "device")
        wins[winner] += 1
        lines.append("%-30s %-18s %26s %26s %6.2f %-7s %6d %22s %22s" % (
            where, "%d>%d %dx%d %dx%d" % (cin, cout, k, k, H, W), CELL % a, CELL % b, a[0] / b[0], winner, n,
            "%8.4f (%.4f-%.4f)" % s1, "%7.4f (%.4f-%.4f)" % s2))
        print(lines[-1], flush=True)
        del x, gy, ws, ref, mine
        torch.cuda.empty_cache()
    lines.append("of %d shapes: torch faster on %d, ssg_amd.Conv2d faster on %d, within the spread on %d.  The feature is opt-in whatever this says."
                 % (len(SHAPES), wins["torch"], wins["device"], wins["tie"]))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])


if __name__ == "__main__":
    main()
