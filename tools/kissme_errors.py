"""Writes profiles/kissme_errors.txt: for every case of tests/kissme_ref.py the share of its bound that the device uses, measured on the
GPU -- the figures behind the assertions of tests/test_gpu_kissme.py (nothing is asserted here):

    C1, C0        worst |dev - ref64| / ((P + 2) 2^-53 A) over the elements
    M before validation
                  ||M_dev - M_64||_F / (2 (||C1^-1||_2^2 ||B1||_F + ||C0^-1||_2^2 ||B0||_F)), with cond(C) and ||C^-1||_2 ||B||_F
    transform     worst |dev - X64 G64| / ((d + 2) 2^-24 |X| |G|)

    python tools/kissme_errors.py [--out FILE]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "kissme_errors.txt")


def main():
    import torch
    import kissme_ref as kr
    from train_common import bound
    from ssg_amd.metric_learning import KISSME
    lines = ["KISSME on %s against the float64 restatement (tests/kissme_ref.py); numpy %s" % (torch.cuda.get_device_name(0), np.__version__),
             "%-4s %5s %4s %5s | %-23s | %-23s | %9s %9s %11s %11s | %9s | %9s" %
             ("case", "n", "d", "P", "C1 max err   err/bound", "C0 max err   err/bound", "cond C1", "cond C0", "|C1^-1||B1|", "|C0^-1||B0|", "M share", "transform")]
    for name in sorted(kr.CASES):
        X, y = kr.make_case(name)
        st = {}
        k = KISSME().fit(X, y, rng=kr.FIT_SEED[name], stages=st)
        r = kr.fit64(X, y, st["p"])
        cells, lim, small = [], 0.0, []
        for c, b in (("C1", "B1"), ("C0", "B0")):
            err = np.abs(st[c] - r[c])
            cells.append("%10.3e %10.3e" % (err.max(), (err / r[b]).max()))
            inv2, bf = np.linalg.norm(np.linalg.inv(r[c]), 2), np.linalg.norm(r[b], "fro")
            lim += 2.0 * inv2 * inv2 * bf; small.append(inv2 * bf)
        G = k.transformer()
        X64 = X.astype(np.float64)
        terr = np.abs(k.transform(X).astype(np.float64) - X64.dot(G)) / bound(X.shape[1], np.abs(X64).dot(np.abs(G)))
        lines.append("%-4s %5d %4d %5d | %s  | %s  | %9.3g %9.3g %11.3e %11.3e | %9.3e | %9.3e" %
                     (name, X.shape[0], X.shape[1], r["P"], cells[0], cells[1], np.linalg.cond(r["C1"]), np.linalg.cond(r["C0"]), small[0], small[1],
                      np.linalg.norm(st["M_raw"] - r["M_raw"], "fro") / lim, terr.max()))
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
