#!/usr/bin/env python3
"""Write profiles/conv_strided_errors.txt (run on the MI355X): for every case of tests/test_gpu_conv_strided.py, through
conv2d_train_strided and through the raw entry points, and for each of y, dX and dW: max |device - ref64|, the same measure for torch's
float32 CPU convolution, and the worst ratio of the device error to the asserted bound (L + 2) 2^-24 A.  Then the max-pool backward of
tests/test_gpu_maxpool_train.py against its bound, and the composed stride-2 bottleneck (use_device_conv(strided=True) +
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
    import conv_strided_ref as ref
    import test_gpu_conv_strided as t
    import test_gpu_maxpool_train as tp
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "conv_strided_errors.txt")
    lines = ["strided train-mode Conv2d, 7x7 stem and MaxPool2d(3, 2, 1) (csrc/conv_strided.hip) on %s: error against torch's autograd in float64 "
             "on the CPU" % torch.cuda.get_device_name(0),
             "err = max |v - ref64| (absolute); err / bound = worst element of |dev - ref64| / ((L + 2) 2^-24 A), asserted <= 1",
             "%-18s %-28s %-21s %-3s %11s %11s %12s" % ("case", "(B, H, W, Cin, Cout, k)", "via", "out", "err_dev", "err_f32cpu", "err / bound")]
    worst = worst_new = 0.0
    for name, case, path, o, e_dev, e_f32, frac in t.measure():
        worst = max(worst, frac)
        if name.startswith("real_"):
            worst_new = max(worst_new, frac)
        lines.append("%-18s %-28s %-21s %-3s %11.3e %11.3e %12.3g" % (name, case, path, o, e_dev, e_f32, frac))
    lines.append("worst err / bound: %.3g" % worst)
    lines.append("")
    lines.append("max-pool backward: err / bound = worst element of |dX - ref64| / ((4 + 2) 2^-24 A); the forward is bit-equal (asserted)")
    for name in ref.POOL_CASES:
        x, gy, y32, dx64, A = ref.pool_reference(name)
        for route in (tp._api, tp._abi):
            y, dx = route(name)
            err = (dx.cpu().double() - dx64).abs()
            frac = float((err / ((4 + 2) * ref.U * A).clamp_min(1e-300)).max())
            lines.append("%-18s %-28s %-21s %-3s %11.3e %11s %12.3g" % (name, tuple(x.shape), route.__name__.strip("_"), "dx", float(err.max()), "-", frac))
    lines.append("")
    lines.append("composition: Bottleneck(256 -> 512, stride 2) with use_device_conv(strided=True) + use_device_batchnorm, x %r, parameter gradients"
                 % (t.COMP_SHAPE,))
    lines.append("err = max |v - ref64| / max |ref64|; ratio = err_dev / err_f32 (float32 CPU run of the same block)")
    lines += composition_table(t.measure_composition(), t.F_COMP, 24)
    lines.append("")
    lines.append("worst err / bound of the real-width cases (real_*): %.3g" % worst_new)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
