#!/usr/bin/env python3
"""Write profiles/loss_errors.txt (run on the MI355X): for every case of tests/test_gpu_loss.py and each output, the worst ratio of the
device error against float64 (tests/loss_ref.py) to the asserted bound

    2^-23 |ref64| + 1e-12 (1 + A) max(1, |factor|)          (the OIM table: 2^-22 / (1 - m) absolute)

per case and per (mode, C) over the batch sizes.  Recorded, not asserted; a ratio above 1 is a bug."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    import test_gpu_loss as t
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "loss_errors.txt")
    lines = ["classification losses (csrc/softmax_ce.hip) on %s: error against the float64 restatement of tests/loss_ref.py" % torch.cuda.get_device_name(0),
             "err / bound = worst element of |dev - ref64| / bound, asserted <= 1; bound = 2^-23 |ref64| + 1e-12 (1 + A) max(1, |factor|); the OIM table "
             "2^-22 / (1 - m); row staging capacity %d floats" % t.cap(),
             "%-32s %-14s %-20s %-18s %12s" % ("case", "shape", "via", "out", "err / bound")]
    worst, shapes = 0.0, {}
    for name, shape, via, o, q in t.measure():
        worst = max(worst, q)
        if via == "cross_entropy_train" and name in [m[0] for m in t.ref.MODES]:      # the shape sweep: one line per (mode, C), the worst over B
            key = (name, shape[1], o)
            shapes[key] = max(shapes.get(key, 0.0), q)
            continue
        lines.append("%-32s %-14s %-20s %-18s %12.3g" % (name, "%dx%d" % tuple(shape[:2]) + ("x%d" % shape[2] if len(shape) > 2 else ""), via, o, q))
    for (name, C, o), q in shapes.items():
        lines.append("%-32s %-14s %-20s %-18s %12.3g" % (name, "B*x%d" % C, "cross_entropy_train", o, q))
    lines.append("B* = the worst over B in %r.  worst err / bound over all lines: %.3g" % (t.ref.SHAPE_B, worst))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
