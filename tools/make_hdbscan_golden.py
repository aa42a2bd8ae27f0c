#!/usr/bin/env python3
"""Write tests/golden/hdbscan_cases.npz: what sklearn's `HDBSCAN(metric='precomputed')` gives for every case of tests/hdbscan_ref.py.
Needs sklearn (written with 1.7.2); no GPU.

Per case: the sha256 of the rebuilt matrix, the core distances, the spanning tree in Prim order (sklearn's own
`mutual_reachability_graph` + `mst_from_mutual_reachability`), the `row_order` this machine's `np.argsort` gave for its weights, the
single-linkage tree, `labels_`, `probabilities_`, the labels of `dbscan_clustering` at the case's two cuts, and whether sklearn warned
about infinite edges.  Every array is N long.

Nothing is written unless, on every case, the numpy restatement of tests/hdbscan_ref.py reproduces sklearn bit for bit: the core
distances and the three fields of every edge from the matrix, and -- fed the stored row_order -- the tree, the labels, the
probabilities and the cut labels; and unless the cases marked `full` show at least 2 clusters and at least one noise point."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hdbscan_ref as ref  # noqa: E402


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.astype(a.dtype).tobytes()


def main():
    import sklearn
    from sklearn.cluster import HDBSCAN
    from sklearn.cluster._hdbscan._linkage import make_single_linkage, mst_from_mutual_reachability
    from sklearn.cluster._hdbscan._reachability import mutual_reachability_graph
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for case in ref.CASES:
        name = case["name"]
        D = ref.matrix(case)
        ms, alpha = ref.min_samples_of(case), case["alpha"]
        X = np.array(D, dtype=np.float64)
        X /= alpha
        core = np.partition(X, ms - 1, axis=1)[:, ms - 1].copy()
        mst = mst_from_mutual_reachability(mutual_reachability_graph(X, min_samples=ms))
        row_order = np.argsort(mst["distance"])
        slt = make_single_linkage(mst[row_order])
        est = HDBSCAN(metric="precomputed", min_cluster_size=case["min_cluster_size"], min_samples=case["min_samples"], alpha=alpha,
                      cluster_selection_method=case["method"], allow_single_cluster=case["allow_single_cluster"],
                      cluster_selection_epsilon=case["epsilon"], max_cluster_size=case["max_cluster_size"], copy=True)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            est.fit(np.array(D, dtype=np.float64))
        warned = any("edge weights with value infinity" in str(w.message) for w in caught)
        assert est._single_linkage_tree_.tobytes() == slt.tobytes(), name
        got = dict(core=core, mst_current=mst["current_node"].copy(), mst_next=mst["next_node"].copy(), mst_distance=mst["distance"].copy(),
                   row_order=row_order.astype(np.int64), slt_left=slt["left_node"].astype(np.int64), slt_right=slt["right_node"].astype(np.int64),
                   slt_value=slt["value"].copy(), slt_size=slt["cluster_size"].astype(np.int64), labels=est.labels_.astype(np.int64),
                   probs=est.probabilities_.copy(), warned=np.array(warned))
        for i, cut in enumerate(case["cuts"]):
            got["cut%d" % i] = est.dbscan_clustering(cut, min_cluster_size=case["min_cluster_size"]).astype(np.int64)
        # the restatement against sklearn
        rcore = ref.core_distances(D, ms, alpha)
        assert same_bits(rcore, core), (name, "core")
        for g, key in zip(ref.prim(D, rcore, alpha), ("mst_current", "mst_next", "mst_distance")):
            assert same_bits(g, got[key]), (name, key)
        assert warned == bool(np.isinf(got["mst_distance"]).any()), name
        for key, val in ref.run_case(case, got["mst_current"], got["mst_next"], got["mst_distance"], row_order).items():
            assert same_bits(val, got[key]), (name, key)
        n_clusters, n_noise = int(est.labels_.max()) + 1, int((est.labels_ < 0).sum())
        if case["full"]:
            assert n_clusters >= 2 and n_noise >= 1, (name, n_clusters, n_noise)
        ties = len(got["mst_distance"]) - len(np.unique(got["mst_distance"]))
        print("%-20s N %5d  clusters %3d  noise %4d  tied edges %4d  cut labels %s%s" % (
            name, case["N"], n_clusters, n_noise, ties, [int(got["cut%d" % i].max()) + 1 for i in range(len(case["cuts"]))], "  (warned)" if warned else ""))
        out[name + "/sha256"] = np.array(ref.sha(D))
        for key, val in got.items():
            out["%s/%s" % (name, key)] = val
    assert sum(bool(out[c["name"] + "/warned"]) for c in ref.CASES) == 1
    np.savez_compressed(ref.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (ref.GOLDEN, os.path.getsize(ref.GOLDEN)))


if __name__ == "__main__":
    main()
