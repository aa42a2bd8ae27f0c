#!/usr/bin/env python3
"""Write profiles/head_errors.txt (run on the MI355X): for every case of tests/test_gpu_head.py, through stripe_pool_train /
linear_train and through the raw entry points, and for each output: max |device - ref64| and the worst ratio of the device error to the
asserted bound ((L + 2) 2^-24 A; 4 * 2^-24 A for the pool's dX).  Then the composed look-alike model (use_device_conv(strided=True) +
use_device_maxpool + use_device_batchnorm + use_device_head): per parameter gradient err = max |v - ref64| / max |ref64| of the device
and of the float32 CPU run, and their ratio; the test's factor F_COMP is the next power of two above the worst ratio (at most 4).
Recorded, not asserted."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    from train_common import composition_table
    import test_gpu_head as t
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "head_errors.txt")
    lines = ["train-mode head: stripe pooling and Linear (csrc/head_train.hip) on %s: error against torch's autograd in float64 on the CPU"
             % torch.cuda.get_device_name(0),
             "err = max |v - ref64| (absolute); err / bound = worst element of |dev - ref64| / bound, asserted <= 1; bound = (L + 2) 2^-24 A, "
             "for the pool's dx 4 * 2^-24 A; dx/<which sets received a gradient>",
             "%-11s %-24s %-18s %-8s %11s %12s" % ("case", "shape", "via", "out", "err_dev", "err / bound")]
    worst = 0.0
    for name, case, path, o, e_dev, frac in t.measure():
        worst = max(worst, frac)
        lines.append("%-11s %-24s %-18s %-8s %11.3e %12.3g" % (name, case, path, o, e_dev, frac))
    lines.append("shapes: pool (B, h, w, C, S), Linear (B, K, N, bias).  worst err / bound: %.3g" % worst)
    lines.append("")
    lines.append("composition: the look-alike model of tests/head_ref.py (7x7 stem, max-pool, one stride-2 bottleneck, num_split 2, feat, feat_bn) with "
                 "use_device_conv(strided=True) + use_device_maxpool + use_device_batchnorm + use_device_head, images %r, parameter gradients" % (t.COMP_SHAPE,))
    lines.append("err = max |v - ref64| / max |ref64|; ratio = err_dev / err_f32 (float32 CPU run of the unswapped model)")
    lines += composition_table(t.measure_composition(), t.F_COMP, 34)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
