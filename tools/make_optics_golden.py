"""Writes tests/golden/optics_cases.npz: what sklearn's OPTICS(metric='precomputed') gives for every case of tests/optics_ref.py --
ordering_, core_distances_, reachability_, predecessor_, and the labels (and cluster hierarchy) of every cut -- plus a sha256 of
every rebuilt matrix.  Needs scikit-learn (the golden was written with 1.7.2); the package and the tests do not.

    python tools/make_optics_golden.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import optics_ref as ref  # noqa: E402


def main():
    import sklearn
    from sklearn.cluster import OPTICS, cluster_optics_dbscan, cluster_optics_xi
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for case in ref.CASES:
        name = case["name"]
        D = ref.matrix(case)
        X = np.asarray(D, dtype=np.float64)              # sklearn widens first: the golden of a half matrix is that of its float64 copy
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            est = OPTICS(metric="precomputed", min_samples=case["min_samples"], max_eps=case["max_eps"]).fit(X)
        out[name + "/sha256"] = np.array(ref.sha(D))
        out[name + "/warned"] = np.array(any("All reachability values are inf" in str(w.message) for w in caught))
        out[name + "/ordering"], out[name + "/core"] = est.ordering_, est.core_distances_
        out[name + "/reach"], out[name + "/pred"] = est.reachability_, est.predecessor_
        for i, cut in enumerate(case["cuts"]):
            if cut["method"] == "xi":
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    labels, hier = cluster_optics_xi(reachability=est.reachability_, predecessor=est.predecessor_, ordering=est.ordering_,
                                                     min_samples=case["min_samples"], min_cluster_size=cut["min_cluster_size"], xi=cut["xi"],
                                                     predecessor_correction=cut["predecessor_correction"])
                out["%s/cut%d/hier" % (name, i)] = hier
            else:
                labels = cluster_optics_dbscan(reachability=est.reachability_, core_distances=est.core_distances_, ordering=est.ordering_,
                                               eps=case["max_eps"] if cut["eps"] is None else cut["eps"])
            out["%s/cut%d/labels" % (name, i)] = labels
            print("%-12s cut %d %-6s clusters %3d noise %4d" % (name, i, cut["method"], labels.max() + 1, int((labels < 0).sum())))
        print("%-12s N %4d inf core %4d inf reach %4d around15 changed %4d core distances" % (
            name, case["N"], int(np.isinf(est.core_distances_).sum()), int(np.isinf(est.reachability_).sum()),
            int((np.sort(X, axis=1)[:, ref.resolve_size(case["min_samples"], case["N"]) - 1] != est.core_distances_).sum())))
    os.makedirs(os.path.dirname(ref.GOLDEN), exist_ok=True)
    np.savez_compressed(ref.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (ref.GOLDEN, os.path.getsize(ref.GOLDEN)))


if __name__ == "__main__":
    main()
