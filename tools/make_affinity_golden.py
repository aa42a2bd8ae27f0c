"""tests/golden/affinity_cases.npz: for every case of tests/affinity_ref.py, sklearn's AffinityPropagation(affinity='precomputed') on the
CPU -- cluster_centers_indices_, labels_, n_iter_ -- and the sha256 of the numpy restatement's final A, R and S.  Needs sklearn
(written with 1.7.2); the restatement must agree with sklearn on every case or nothing is written.

    python tools/make_affinity_golden.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import affinity_ref as ref  # noqa: E402


def main():
    import sklearn
    from sklearn.cluster import AffinityPropagation
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name in ref.CASES:
        X = ref.case_input(ref.CASES[name][0])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sk = AffinityPropagation(affinity="precomputed", **ref.case_kwargs(name)).fit(X.copy())
        r = ref.case_result(name)
        cen = np.asarray(sk.cluster_centers_indices_, dtype=np.int64)
        assert np.array_equal(cen, r["centers"]) and np.array_equal(sk.labels_, r["labels"]) and sk.n_iter_ == r["n_iter"], name
        out[name + "_centers"], out[name + "_labels"], out[name + "_n_iter"] = cen, np.asarray(sk.labels_, dtype=np.int64), np.array(sk.n_iter_)
        out[name + "_sha"] = np.array([ref.sha(r["A"]), ref.sha(r["R"]), ref.sha(r["S"])])
        print("%-8s N %4d n_iter %3d K %3d converged %s" % (name, X.shape[0], sk.n_iter_, len(cen), r["converged"]))
    path = os.path.join(ROOT, "tests", "golden", "affinity_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
