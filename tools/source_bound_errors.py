#!/usr/bin/env python3
"""Write profiles/source_bound_errors.txt (run on the MI355X): for every case of tests/source_bound_ref.py and every bound path of
tests/test_gpu_source_bound.py, the worst entry of the bound table against the float64 granule minimum, as a share of the contract

    |table - min over the granule's real sources of sum_k (x_k - y_k)^2| <= tol / 2,     tol = rerank.source_bound_params(...)

and the share of the granules the refine pass re-evaluates in float64.  Recorded, not asserted; a ratio above 1 is a bug."""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    import test_gpu_source_bound as t
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "source_bound_errors.txt")
    lines = ["source term bound tables (csrc/source_bound.hip, csrc/source_term.hip, conv.hip epi 3) on %s against the float64 restatement of "
             "tests/source_bound_ref.py" % torch.cuda.get_device_name(0),
             "err / (tol / 2) = worst entry of |table - float64 granule minimum| over every row and granule with a real source, asserted <= 1; "
             "refined = share of those granules within tol of the row's smallest bound",
             "%-26s %-12s %-8s %2s %16s %12s" % ("case", "shape", "path", "G", "err / (tol / 2)", "refined")]
    worst = 0.0
    with tempfile.TemporaryDirectory() as tmp:
        for name, path, G, q, share, bad in t.measure(tmp):
            c = t.ref.case(name)
            worst = max(worst, q)
            lines.append("%-26s %-12s %-8s %2d %16.3g %12.3g%s" % (name, "%dx%dx%d" % (c.tgt.shape[0], c.src.shape[0], c.tgt.shape[1]), path, G, q, share,
                                                                  "   FAILED " + "; ".join(bad) if bad else ""))
    lines.append("worst err / (tol / 2) over all lines: %.3g" % worst)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
