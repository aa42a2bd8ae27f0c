#!/usr/bin/env python3
"""Write profiles/batchnorm_errors.txt (run on the MI355X): for every case and variant of tests/test_gpu_batchnorm.py and every output
of the four batch-norm entry points ("abi" rows) and of the autograd function batch_norm_train ("fn" rows), err_dev = max |device -
ref64| / max |ref64|, err_f32 = the same measure for tests/batchnorm_ref.py run in float32 on the CPU, and their ratio.  The test's
factor F is the next power of two above the worst ratio (at most 4).  Where err_dev <= 2^-24 -- the rounding of the float32 output,
which the criterion allows by itself -- the ratio is shown but does not count.  The last column is the share of the asserted bound
F err_f32 + 2^-24 that err_dev uses; the last line gives its worst value at the real channels_last widths (the real_* cases)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    import test_gpu_batchnorm as t
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "batchnorm_errors.txt")
    lines = ["batch-norm entry points (csrc/batchnorm.hip) on %s: error against tests/batchnorm_ref.py in float64, next to the float32 torch chain's"
             % torch.cuda.get_device_name(0),
             "err = max|v - ref64| / max|ref64|; ratio = err_dev / err_f32; '*': err_dev > 2^-24 = %.3e, the ratio counts" % t.FLOOR,
             "err / bound = err_dev / (F err_f32cpu + 2^-24) with the test's F = %g, asserted <= 1; cl: channels_last" % t.F,
             "%-14s %-20s %-9s %-4s %-13s %11s %11s %9s %12s" % ("case", "shape", "variant", "via", "output", "err_dev", "err_f32cpu", "ratio", "err / bound")]
    worst = worst_all = worst_real = 0.0
    for name in t.CASES:
        shape = "%s%s" % ("x".join(str(s) for s in t.CASES[name][0]), " cl" if t.CASES[name][1] else "")
        for variant in t.VARIANTS:
            for via, run in (("abi", None), ("fn", t._function)):
                for k, e_dev, e_f32 in t.measure(name, variant, run):
                    ratio = e_dev / e_f32 if e_f32 > 0 else float("inf") if e_dev > 0 else 0.0
                    frac = e_dev / (t.F * e_f32 + t.FLOOR)
                    counts = e_dev > t.FLOOR
                    if counts:
                        worst = max(worst, ratio)
                    if e_f32 > 0:
                        worst_all = max(worst_all, ratio)
                    if name.startswith("real_"):
                        worst_real = max(worst_real, frac)
                    lines.append("%-14s %-20s %-9s %-4s %-13s %11.3e %11.3e %9.3g %12.3g%s"
                                 % (name, shape, variant, via, k, e_dev, e_f32, ratio, frac, " *" if counts else ""))
    lines.append("worst counting ratio: %.3g; worst ratio among all outputs with err_f32 > 0: %.3g" % (worst, worst_all))
    lines.append("worst err / bound of the real-width cases (real_*): %.3g" % worst_real)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-3:]))


if __name__ == "__main__":
    main()
