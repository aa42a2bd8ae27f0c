#!/usr/bin/env python3
"""Write tests/golden/silhouette_cases.npz: what sklearn's `silhouette_samples` and `silhouette_score` give for `metric='precomputed'`
on every case of tests/silhouette_ref.py.  Needs sklearn (written with 1.7.2); no GPU.

Per case: the labels and sklearn's per-sample result on the float64 copy of the matrix (for the 'noise' cases: on the sub-matrix of
the samples not labelled -1, NaN at the dropped positions; for the 're-rank' cases: on the matrix with its diagonal zeroed) and their
mean.  Per case marked `sample`: `silhouette_score(sample_size=N // 2, random_state=3)` and the next draw of that stream after the call.
The matrices are not stored: tests/silhouette_ref.py rebuilds them from seeds.

Nothing is written unless, on every case, the sequential restatement of tests/silhouette_ref.py reproduces sklearn bit for bit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import silhouette_ref as ref  # noqa: E402


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def main():
    import sklearn
    from sklearn.metrics import silhouette_samples, silhouette_score
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for case in ref.CASES:
        name, N = case["name"], case["N"]
        X, lab = ref.expected_input(case), ref.labels(case)
        if case["kind"] == "neg":
            # sklearn refuses a negative precomputed distance (pairwise_distances), after all its other checks: the message is stored, and
            # the tests hold the kernel's sums on this matrix to the restatement instead
            assert (X < 0).any()
            try:
                silhouette_samples(X, lab, metric="precomputed")
                raise AssertionError("sklearn accepted a negative distance")
            except ValueError as e:
                out[name + "/labels"], out[name + "/error"] = lab.astype(np.int64), np.array(str(e))
            print("%-20s N %5d  %-6s %-10s refused: %s" % (name, N, case["kind"], case["labeling"], out[name + "/error"]))
            continue
        if ref.ignore_noise(case):
            keep = lab != -1
            sil = np.full(N, np.nan)
            sil[keep] = silhouette_samples(X[keep][:, keep], lab[keep], metric="precomputed")
            score = silhouette_score(X[keep][:, keep], lab[keep], metric="precomputed")
        else:
            sil = silhouette_samples(X, lab, metric="precomputed")
            score = silhouette_score(X, lab, metric="precomputed")
        assert sil.dtype == np.float64 and same_bits(ref.expected(case), sil), (name, "restatement")
        out[name + "/labels"], out[name + "/sil"], out[name + "/score"] = lab.astype(np.int64), sil, np.array(score)
        extra = ""
        if case.get("sample"):
            rs = np.random.RandomState(ref.SAMPLE_SEED)
            sampled = silhouette_score(X, lab, metric="precomputed", sample_size=N // 2, random_state=rs)
            nxt = rs.random_sample()
            rs2 = np.random.RandomState(ref.SAMPLE_SEED)
            assert same_bits(ref.sampled_score(X, lab, N // 2, rs2), sampled) and rs2.random_sample() == nxt, (name, "sampled restatement")
            assert sampled == silhouette_score(X, lab, metric="precomputed", sample_size=N // 2, random_state=ref.SAMPLE_SEED)
            out[name + "/sampled_score"], out[name + "/next_draw"] = np.array(sampled), np.array(nxt)
            extra = "  sampled %.6f" % sampled
        print("%-20s N %5d  %-6s %-10s clusters %4d  score %+.6f%s" % (name, N, case["kind"], case["labeling"], len(np.unique(lab[lab != -1] if ref.ignore_noise(case) else lab)),
                                                                      score, extra))
    np.savez_compressed(ref.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (ref.GOLDEN, os.path.getsize(ref.GOLDEN)))


if __name__ == "__main__":
    main()
