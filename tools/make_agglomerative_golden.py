#!/usr/bin/env python3
"""Write tests/golden/agglomerative_cases.npz: what scipy's `linkage` and sklearn's `AgglomerativeClustering(metric='precomputed')` give
for every case of tests/agglomerative_ref.py and every linkage.  Needs scipy and sklearn (written with 1.15.3 and 1.7.2); no GPU.

Per case: the sha256 of the rebuilt matrix.  Per case and linkage: scipy's Z on the condensed upper triangle; the merges in merge
order (the restatement's: scipy does not hand them out before its sort); the thresholds the tests cut at; and for every n_clusters in
{1, 2, 7, N} and every threshold sklearn's `n_clusters_` and `labels_` (`children_` and `distances_` are columns of Z, asserted here).

Nothing is written unless, on every case, the restatement of tests/agglomerative_ref.py reproduces scipy's Z and sklearn's labels bit
for bit -- the numpy form everywhere, the entry-by-entry form up to N = 130 -- and unless the case built for it shows chain[-2] keeping
a tie against a lower-indexed slot."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import agglomerative_ref as ref  # noqa: E402


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.astype(a.dtype).tobytes()


def main():
    import scipy
    import sklearn
    from scipy.cluster.hierarchy import linkage
    from sklearn.cluster import AgglomerativeClustering
    out = {"sklearn_version": np.array(sklearn.__version__), "scipy_version": np.array(scipy.__version__)}
    for case in ref.CASES:
        name, N = case["name"], case["N"]
        D = ref.matrix(case)
        X64 = np.array(D, dtype=np.float64)
        out[name + "/sha256"] = np.array(ref.sha(D))
        for method in ref.LINKAGES:
            key = "%s/%s" % (name, method)
            Z = linkage(ref.condensed(D), method=method)
            stats = {}
            x, y, d, s = ref.merges(D, method, stats=stats)
            assert same_bits(ref.label(x, y, d), Z), (key, "restatement")
            if N <= ref.LITERAL_MAX_N:
                for a, b in zip(ref.merges(D, method, literal=True), (x, y, d, s)):
                    assert (a is None and b is None) or same_bits(a, b), (key, "entry-by-entry restatement")
            if case["kind"] == "prevtie" and method != "single":
                assert stats["prev_kept"] >= 1, key
            out[key + "/Z"] = Z
            out[key + "/x"], out[key + "/y"], out[key + "/d"] = x, y, d
            if s is not None:
                out[key + "/size"] = s
            ths = ref.thresholds(Z)
            out[key + "/thresholds"] = np.array(ths)
            fits = [("k%d" % k, dict(n_clusters=k)) for k in ref.n_clusters_options(N)] + [("t%d" % i, dict(n_clusters=None, distance_threshold=t)) for i, t in enumerate(ths)]
            counts = []
            for tag, kw in fits:
                est = AgglomerativeClustering(metric="precomputed", linkage=method, compute_distances=True, **kw).fit(X64)
                assert same_bits(est.children_.astype(np.float64), Z[:, :2]) and same_bits(est.distances_, Z[:, 2]), (key, tag)
                assert (est.n_leaves_, est.n_connected_components_, est.n_features_in_) == (N, 1, N)
                children, k, labels = ref.fit(Z, kw.get("n_clusters"), kw.get("distance_threshold"))
                assert k == est.n_clusters_ and np.array_equal(labels, est.labels_), (key, tag)
                out["%s/%s/labels" % (key, tag)] = est.labels_.astype(np.int64)
                out["%s/%s/n_clusters" % (key, tag)] = np.array(int(est.n_clusters_))
                counts.append(int(est.n_clusters_))
            ties = len(Z) - len(np.unique(Z[:, 2]))
            print("%-14s %-8s N %5d  scans %5s  chain[-2] kept a tie %4s  tied heights %4d  clusters at the cuts %s" % (
                name, method, N, stats.get("scans", "-"), stats.get("prev_kept", "-"), ties, counts))
    np.savez_compressed(ref.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (ref.GOLDEN, os.path.getsize(ref.GOLDEN)))


if __name__ == "__main__":
    main()
