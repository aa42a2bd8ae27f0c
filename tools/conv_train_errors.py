#!/usr/bin/env python3
"""Write profiles/conv_train_errors.txt (run on the MI355X): for every case of tests/test_gpu_conv_train.py, through conv2d_train and
through the raw entry points, and for each of y, dX and dW: max |device - ref64|, the same measure for torch's float32 CPU convolution,
and the worst ratio of the device error to the asserted bound (L + 2) 2^-24 A.  Then the composed bottleneck block (use_device_conv +
use_device_batchnorm): per parameter gradient err = max |v - ref64| / max |ref64| of the device and of the float32 CPU run, and their
ratio; the test's factor F_COMP is the next power of two above the worst ratio (at most 4).  Recorded, not asserted."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    from train_common import composition_table
    import test_gpu_conv_train as t
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "conv_train_errors.txt")
    lines = ["train-mode Conv2d (csrc/conv_train.hip, ssg_conv2d_nhwc_f32) on %s: error against torch's F.conv2d autograd in float64 on the CPU"
             % torch.cuda.get_device_name(0),
             "err = max |v - ref64| (absolute); err / bound = worst element of |dev - ref64| / ((L + 2) 2^-24 A), asserted <= 1",
             "trainer_* (M = 131072, reference: float64 matmuls): dw against (L_s + 2) 2^-24 A, L_s = ceil(M / (slices - 1)) >= the slice length",
             "%-18s %-28s %-13s %-3s %11s %11s %12s" % ("case", "(B, H, W, Cin, Cout, k)", "via", "out", "err_dev", "err_f32cpu", "err / bound")]
    worst = worst_new = 0.0
    for name, case, path, o, e_dev, e_f32, frac in t.measure():
        worst = max(worst, frac)
        if name.startswith(("real_", "trainer_")):
            worst_new = max(worst_new, frac)
        lines.append("%-18s %-28s %-13s %-3s %11.3e %11.3e %12.3g" % (name, case, path, o, e_dev, e_f32, frac))
    lines.append("worst err / bound: %.3g" % worst)
    lines.append("")
    lines.append("composition: Bottleneck(64 -> 256) with use_device_conv + use_device_batchnorm, x %r, parameter gradients" % (t.COMP_SHAPE,))
    lines.append("err = max |v - ref64| / max |ref64|; ratio = err_dev / err_f32 (float32 CPU run of the same block)")
    lines += composition_table(t.measure_composition(), t.F_COMP, 24)
    lines.append("")
    lines.append("worst err / bound of the real-width (real_*) and trainer-batch (trainer_*) cases: %.3g" % worst_new)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
