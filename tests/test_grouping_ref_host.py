"""CPU suite: the independent grouping reference of tests/grouping_ref.py (used by tests/test_gpu_grouping_large.py at N = 30 000 and
128 000) against the reference's own results -- the committed goldens of reid/rerank.py + selftraining.py:289-306 + sklearn, and
sklearn's dense DBSCAN -- so that the checker is trusted before it meets the GPU."""
import numpy as np
import pytest
import torch

import grouping_ref as gr

GOLDENS = ["rerank_n256_l01_ref.npz", "rerank_n256_l01_stable.npz", "rerank_n256_l03_ref.npz", "rerank_n256_l03_stable.npz",
           "rerank_n1024_l01_ref.npz", "rerank_n1024_l01_stable.npz", "rerank_n1024_l03_ref.npz", "rerank_n1024_l03_stable.npz"]


def _stages(g, ora):
    mode = "stable" if bool(g["stable"]) else "introsort"
    _, f, st = ora.re_ranking(g["src"], g["tgt"], k1=int(g["k1"]), k2=int(g["k2"]), lambda_value=float(g["lambda_value"]), rank_mode=mode, stages=True)
    return f, torch.from_numpy(st["jaccard_scaled"].copy()), torch.from_numpy(st["v"].copy())


@pytest.mark.parametrize("name", GOLDENS)
def test_final_rows_bit_equal_to_the_reference(name, golden, ora):
    """final_dist rebuilt from J' and v with torch element-wise ops == the reference's final_dist (the golden's own matrix at N = 256,
    the oracle's, which reproduces the golden's sha256, at N = 1024), in every row block split"""
    g = golden(name)
    f, Jp, v = _stages(g, ora)
    if "final" in g.files:
        assert np.array_equal(f, g["final"])
    lam = float(g["lambda_value"])
    N = f.shape[0]
    assert np.array_equal(gr.final_rows(Jp, v, lam, 0, N).numpy(), f)
    for block in (1, 7, 100):
        got = np.concatenate([F.numpy() for _, F in gr.FinalDist(Jp, v, lam, block_rows=block).blocks()])
        assert np.array_equal(got, f)
    # the numpy restatement of tests/test_gpu_fullsize.py::_check_sampled_rows, on a few rows
    vn, jn = v.numpy(), Jp.numpy()
    for r in (0, 1, N // 2, N - 1):
        ref = jn[r].astype(np.float64) + (vn + vn[r]).astype(np.float64) * lam
        assert np.array_equal(gr.final_rows(Jp, v, lam, r, r + 1).numpy()[0], ref)


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("hint", ["none", "low", "exact", "high"])
def test_eps_and_labels_vs_golden(name, hint, golden, ora):
    """(eps, count, top_num) bit for bit and sklearn's labels exactly, whatever the cap hint (a hint far below the answer makes the
    cap double until `top` entries are collected)"""
    g = golden(name)
    f, Jp, v = _stages(g, ora)
    mat = gr.FinalDist(Jp, v, float(g["lambda_value"]), block_rows=97)
    ge = float(g["eps"])
    h = {"none": None, "low": ge / 64, "exact": ge, "high": 4 * ge}[hint]
    e = gr.eps_rule(mat, float(g["rho"]), hint=h)
    assert (e.eps, e.count, e.top) == (ge, int(g["count"]), int(g["top_num"]))
    assert e.ncand >= e.top
    gg = gr.region_graph(mat, e.eps)
    lab, core = gr.dbscan(gg, e.eps, 4)
    assert np.array_equal(lab, g["labels"])
    assert np.array_equal(gg.counts, (f <= e.eps).sum(axis=1))
    assert np.array_equal(core, np.nonzero(gg.counts >= 4)[0])
    assert np.array_equal(gr.hit_keys(gg, e.eps), np.sort(np.flatnonzero(f <= e.eps)))
    # and the same with the explicit matrix
    e2 = gr.eps_rule(gr.Dense(f, block_rows=300), float(g["rho"]), hint=h)
    assert e2[:3] == e[:3]


def test_sparse_graph_dbscan_vs_sklearn_dense_cases(golden, ora):
    """the sparse-graph DBSCAN reproduces tests/golden/dbscan_cases.npz, written by sklearn from dense matrices.  Their diagonals are
    not zero (one case has eps below the whole diagonal: every point is noise), so a graph without its stored diagonal would fail."""
    g = golden("dbscan_cases.npz")
    for D, eps, lab in zip(g["D"], g["eps"], g["labels"]):
        gg = gr.region_graph(gr.Dense(D, block_rows=50), float(eps))
        assert np.array_equal(gr.dbscan(gg, float(eps), 4)[0], lab)
        assert np.array_equal(gg.counts, (D <= eps).sum(axis=1))
        assert np.array_equal(gr.dbscan(gg, float(eps), 4)[0], ora.dbscan(D, float(eps), 4))


def test_sparse_graph_dbscan_with_duplicate_points():
    """duplicate points: off-diagonal distances of exactly 0 (and a zero diagonal) must stay stored neighbours, and zeros are not
    counted by the eps rule's non-zero triangle"""
    from sklearn.cluster import DBSCAN
    rng = np.random.default_rng(4)
    base = rng.standard_normal((40, 3))
    X = np.concatenate([base, base[:12], base[:5], base[30:33] + 1e-3])           # 12 duplicated points, 5 of them three times
    X = X[rng.permutation(len(X))]
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    N = D.shape[0]
    assert ((D == 0).sum() - N) >= 2 * 12
    for eps in (1e-9, 2e-3, 0.3, 0.6, 1.0):
        gg = gr.region_graph(gr.Dense(D, block_rows=13), eps)
        ref = DBSCAN(eps=eps, min_samples=4, metric="precomputed").fit(D)
        lab, core = gr.dbscan(gg, eps, 4)
        assert np.array_equal(lab, ref.labels_) and np.array_equal(core, ref.core_sample_indices_)
        assert np.array_equal(gg.counts, (D <= eps).sum(axis=1))
        assert gg.csr.nnz >= gg.nhits
    # eps 1e-9: only the exact duplicates are neighbours -- the points present three times (plus themselves) are core
    assert gr.dbscan(gr.region_graph(gr.Dense(D), 1e-9), 1e-9, 3)[0].max() >= 0
    e = gr.eps_rule(gr.Dense(D), 0.05, hint=0.1)
    tri = np.triu(D, 1)
    tri = np.sort(tri[np.nonzero(tri)])
    top = int(np.round(0.05 * tri.size))
    assert (e.eps, e.count, e.top) == (tri[:top].mean(), tri.size, top)


@pytest.mark.parametrize("top", [8191, 8192, 8193, 16385, 40000, 179700])
def test_eps_mean_above_numpy_reduction_buffer(top, ora):
    """np.mean reduces in chunks of numpy's buffer size (8192 elements), pairwise inside each chunk: above 8192 summands one pairwise
    tree over all of them is 1-2 ulp off.  The oracle, the reference and numpy's own code agree for float64 and float16 matrices."""
    rng = np.random.default_rng(top)
    N = 600
    A = rng.random((N, N)) * 1.3 + 0.05
    D = np.triu(A, 1) + np.triu(A, 1).T
    count = N * (N - 1) // 2
    rho = top / count
    ref = gr.numpy_eps_rule(D, rho)
    assert ref[2] == top
    assert ora.eps_rule(D, rho) == ref
    e = gr.eps_rule(gr.Dense(D, block_rows=64), rho, hint=float(ref[0]))
    assert (e.eps, e.count, e.top) == ref
    H = D.astype(np.float16)
    href = gr.numpy_eps_rule(H, rho)
    he, hc, ht = ora.eps_rule(H, rho)
    assert (hc, ht) == href[1:] and np.float16(he).view(np.uint16) == np.float16(href[0]).view(np.uint16)
    s = np.sort(rng.random(top))
    assert ora.reduce_sum(s) == np.sum(s) and ora.reduce_sum(s.astype(np.float32)) == np.sum(s.astype(np.float32))
