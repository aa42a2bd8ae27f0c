"""GPU suite (-m gpu): `cluster.DBSCAN` and `cluster.eps_rule_dbscan` over the whole min_samples / eps / dtype / container / N range they
accept -- the case table of tests/dbscan_grid_ref.py -- against tests/golden/dbscan_grid.npz (sklearn 1.7.2 on the arrays as the cases
pass them) and against the visiting-order restatement of that file; re-rank handles (mode 0: the sparse copy, the packed-half
pre-filter, the generic path) against the restatement on their materialised final_dist; sklearn's refusals of NaN, infinity and
negative values.  Every assertion is an equality: each quantity is defined exactly by the reference."""
import numpy as np
import pytest

import dbscan_grid_ref as grid
from conftest import hard_clustered

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ENVS = [{}, {"SSG_EPS_PATH": "radix"}, {"SSG_EPS_FUSED": "0"}]
ENV_IDS = ["default", "radix", "unfused"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def g(golden):
    return golden(grid.FIXTURE)


_REFS = {}


def _ref(c):
    """the restatement's answers on a case (`grid.check_claims`), once per process; the matrices come from `grid.matrix`, which keeps the
    4096-point ones shared between the cases built on them"""
    if c.name not in _REFS:
        _REFS[c.name] = grid.check_claims(c)
    return _REFS[c.name]


def _region(h, eps, cap):
    """per-row neighbour counts, the sorted hit keys i * N + k and the counted hits, from the region query DBSCAN.fit launches"""
    from ssg_amd import cluster
    from ssg_amd._lib import lib, stream
    cnt = torch.zeros(h.nrows, dtype=torch.int32, device=h.device)
    edges = torch.empty((cap, 2), dtype=torch.int32, device=h.device)
    cursor = torch.zeros(2, dtype=torch.int64, device=h.device)
    cluster._region_query(lib(), h, float(eps), cnt, edges, cap, cursor, stream())
    ne = int(cursor[0].item())
    e = edges[:min(ne, cap)].cpu().numpy().astype(np.int64)
    return cnt.cpu().numpy().astype(np.int64), np.sort(e[:, 0] * h.N + e[:, 1]), ne


# ------------------------------------------------------------------ plain matrices: every case of the table
@pytest.mark.parametrize("name", [c.name for c in grid.PLAIN])
def test_plain_case_vs_sklearn_and_restatement(name, g, dev):
    from ssg_amd import cluster
    c = grid.BY_NAME[name]
    assert grid.sha(grid.matrix(c)) == str(g[name + "__sha"])
    ref = _ref(c)
    want, core = g[name + "__labels"].astype(np.int64), g[name + "__core"].astype(np.int64)
    assert np.array_equal(ref["labels"], want) and np.array_equal(ref["core"], core)              # (the CPU suite's statement, on this machine)
    X = grid.as_passed(c, dev)
    est = cluster.DBSCAN(eps=c.eps, min_samples=c.ms, metric="precomputed")
    assert est.fit(X) is est
    lab1, core1 = est.labels_.copy(), est.core_sample_indices_.copy()
    print("%s: hits %d, clusters %d (device %d), noise %d (device %d), core %d (device %d)" % (
        name, ref["nhits"], ref["n_clusters"], int(lab1.max()) + 1, ref["n_noise"], int((lab1 < 0).sum()), len(core), len(core1)), flush=True)
    assert np.array_equal(core1, core), "core_sample_indices_"
    assert np.array_equal(lab1, want), "labels_: %d differ, first at %s" % ((lab1 != want).sum(), np.nonzero(lab1 != want)[0][:8])
    assert lab1.dtype == np.int64 and est.n_features_in_ == c.N
    # the region query itself: every row's neighbour count, every hit pair
    h = cluster.as_handle(X)
    assert h.mode == (1 if c.dtype == "float16" else 2) and h.eps_f32 == (c.dtype == "float32")
    cnt, keys, ne = _region(h, cluster.compare_eps(h, c.eps), max(ref["nhits"], 1))
    assert ne == ref["nhits"] and np.array_equal(cnt, ref["counts"]), "neighbour counts: rows %s" % np.nonzero(cnt != ref["counts"])[0][:8]
    assert np.array_equal(keys, grid.hit_keys(ref["neigh"])), "hit pairs"
    # a second fit on the same estimator, and fit_predict on a fresh one
    est.fit(X)
    assert np.array_equal(est.labels_, lab1) and np.array_equal(est.core_sample_indices_, core1), "second fit"
    assert np.array_equal(cluster.DBSCAN(eps=c.eps, min_samples=c.ms, metric="precomputed", n_jobs=8).fit_predict(X), want), "fit_predict"


def test_float32_example_gives_sklearn_s_answer(dev):
    """the 2 x 2 example: float32(0.1) <= 0.1 holds where sklearn evaluates it, in float32, and fails on the float64 copy; a half matrix
    is compared in float64 like sklearn's widened copy"""
    from ssg_amd import cluster
    x = np.float32(0.1)
    D = np.array([[0, x], [x, 0]], np.float32)
    fit = lambda X, eps: cluster.DBSCAN(eps=eps, min_samples=2, metric="precomputed").fit_predict(X).tolist()   # noqa: E731
    assert fit(D, 0.1) == [0, 0] and fit(torch.from_numpy(D), 0.1) == [0, 0] and fit(torch.from_numpy(D).to(dev), 0.1) == [0, 0]
    assert fit(D.astype(np.float64), 0.1) == [-1, -1] and fit(torch.from_numpy(D).double().to(dev), 0.1) == [-1, -1]
    H = np.array([[0, 0.3], [0.3, 0]], np.float16)
    assert fit(H, 0.3) == [-1, -1] and fit(H, float(np.float16(0.3))) == [0, 0]
    assert fit(np.array([[.7, .1], [.1, .7]]), 0.5) == [-1, -1]
    assert fit(D, 1e39) == [0, 0]                                                          # float32(eps) overflows to infinity: every entry hits


# ------------------------------------------------------------------ the one-read chain on plain matrices
@pytest.mark.parametrize("env", ENVS, ids=ENV_IDS)
@pytest.mark.parametrize("name", [c.name for c in grid.CHAIN])
def test_chain_equals_two_calls_and_reference(name, env, g, dev, monkeypatch):
    """eps_rule_dbscan(X, rho, ms) == eps_rule(X, rho) then DBSCAN(eps, ms).fit(X) == the reference (selftraining.py's eps rule in numpy,
    sklearn's labels at that radius from the fixture, the restatement's core set), at min_samples 1, 3 and 10, under the eps rule's
    call-time switches"""
    from ssg_amd import cluster
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = grid.BY_NAME[name]
    D = grid.matrix(c)
    X = grid.as_passed(c, dev)
    want = (float(g[name + "__chain_eps"]), int(g[name + "__chain_count"]), int(g[name + "__chain_top"]))
    rule = cluster.eps_rule(X, c.rho)
    assert (float(rule[0]), rule[1], rule[2]) == want, "eps_rule"
    assert isinstance(rule[0], np.float16) == (c.dtype == "float16")
    neigh = grid.neighbourhoods(D, float(rule[0]))
    for ms in grid.CHAIN_MS:
        lab, core = grid.dbscan_ref(D, float(rule[0]), ms, neigh)
        assert np.array_equal(lab, g[name + "__chain_labels%d" % ms])
        eps, cnt, top, lab1, core1 = cluster.eps_rule_dbscan(X, c.rho, min_samples=ms)
        assert (float(eps), cnt, top) == want and type(eps) is type(rule[0]), "eps_rule_dbscan: eps rule (min_samples %d)" % ms
        est = cluster.DBSCAN(eps=rule[0], min_samples=ms, metric="precomputed").fit(X)
        assert np.array_equal(est.labels_, lab) and np.array_equal(est.core_sample_indices_, core), "two calls vs reference (min_samples %d)" % ms
        assert np.array_equal(lab1, lab) and np.array_equal(core1, core), "eps_rule_dbscan vs reference (min_samples %d)" % ms


# ------------------------------------------------------------------ re-rank handles (mode 0)
HANDLES = [(1000, 0.1), (1003, 0.1), (1000, 0.9), (1003, 0.9)]
RADII = ["eps_rule", "floor", "above_jp0", "four"]
HANDLE_MS = (1, 2, 3, 8, 20)
_HANDLES = {}


def _handle(N, lam, dev):
    """(handle, final_dist as numpy float64, {radius name: eps}) once per process"""
    if (N, lam) not in _HANDLES:
        from ssg_amd import cluster, rerank
        from test_gpu_grouping_large import _floor_radius, _pin_helper
        tgt = torch.from_numpy(hard_clustered(N, 256, 61)).to(dev); src = torch.from_numpy(hard_clustered(500, 256, 62, intra=0.7)).to(dev)
        h = rerank.re_ranking_device(src, tgt, lambda_value=lam)
        assert h.mode == 0 and h.sparse is not None and h.sparse_complete()
        _pin_helper(h, [0, N // 2, N - 1])
        final = h.final_dist().cpu().numpy()
        jp0 = float(np.uint16(h.sparse["jp0"]).view(np.float16))
        v = h.v.float()
        floors = jp0 + (v + v.min()).half().double() * h.lambda_value
        # above J'(0): at least the largest floor (no row can use the sparse copy), and the value J'(0) + lambda * half(2 q) of the entries
        # outside the copy whose two source terms are both the upper quartile q of v -- most of the matrix lies at or below it
        q = torch.sort(v).values[3 * N // 4]
        above = max(float(floors.max()), float(jp0 + (q + q).half().double() * h.lambda_value))
        radii = dict(eps_rule=cluster.eps_rule(h, 1.6e-3)[0], floor=_floor_radius(h), above_jp0=above, four=4.0)
        assert radii["floor"] <= radii["above_jp0"] < 4.0 and radii["above_jp0"] >= jp0 and final.max() < 4.0
        _HANDLES[(N, lam)] = (h, final, radii)
    return _HANDLES[(N, lam)]


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("N,lam", HANDLES)
def test_rerank_handle_vs_restatement(N, lam, radius, dev):
    """N = 1000 takes the dense region query's packed-half pre-filter, N = 1003 its generic path; lambda = 0.9 widens the pre-filter's
    band.  The eps rule's radius walks the sparse copy, the floor radius splits the rows between the sparse copy and the dense pass, at
    the largest floor no row can use the copy and most entries hit, at 4.0 every entry hits and the pre-filter flags everything.
    Per-row neighbour counts, hit pairs, and labels / core set at min_samples 1, 2, 3, 8 and 20, against the restatement on final_dist"""
    from ssg_amd import cluster
    h, final, radii = _handle(N, lam, dev)
    eps = radii[radius]
    neigh = grid.neighbourhoods(final, eps)
    counts = np.array([len(n) for n in neigh])
    nhits = int(counts.sum())
    print("N=%d lambda=%g %s radius %.6f: %d hits (%.1f per row)" % (N, lam, radius, eps, nhits, nhits / N), flush=True)
    rows_sparse, rows_dense = cluster.sparse_row_split(h, 1.6e-3, eps)["region"]
    assert rows_sparse + rows_dense == N
    if radius == "eps_rule":
        assert rows_sparse > 0
    if radius == "floor":
        assert rows_sparse > 0 and rows_dense > 0, "the floor radius splits the rows"
    if radius == "four":
        assert nhits == N * N and rows_sparse == 0
    if radius == "above_jp0":
        assert nhits > N * N // 2 and rows_sparse == 0
    cnt, keys, ne = _region(h, eps, max(nhits, 1))
    assert ne == nhits and np.array_equal(cnt, counts), "neighbour counts: rows %s" % np.nonzero(cnt != counts)[0][:8]
    assert np.array_equal(keys, grid.hit_keys(neigh)), "hit pairs"
    for ms in HANDLE_MS:
        lab, core = grid.dbscan_ref(final, eps, ms, neigh)
        est = cluster.DBSCAN(eps=eps, min_samples=ms, metric="precomputed").fit(h)
        assert np.array_equal(est.core_sample_indices_, core), "core samples (min_samples %d)" % ms
        assert np.array_equal(est.labels_, lab), "labels (min_samples %d)" % ms
    if radius == "eps_rule":
        for ms in HANDLE_MS:
            e, _, _, lab1, core1 = cluster.eps_rule_dbscan(h, 1.6e-3, min_samples=ms)
            lab, core = grid.dbscan_ref(final, eps, ms, neigh)
            assert e == eps and np.array_equal(lab1, lab) and np.array_equal(core1, core), "eps_rule_dbscan (min_samples %d)" % ms


# ------------------------------------------------------------------ what sklearn refuses
@pytest.mark.parametrize("bad,match", [(float("nan"), "Input X contains NaN"), (float("inf"), "Input X contains infinity"),
                                       (-float("inf"), "Input X contains infinity"), (-0.25, "Negative values in data passed to X")])
def test_nan_infinity_and_negative_values_are_refused(bad, match, dev):
    from ssg_amd import cluster
    D = np.array(grid.matrix(grid.BY_NAME["d20_plane_n120_f64_ms4"]))
    D[3, 77] = D[77, 3] = bad
    for X in (D, D.astype(np.float32), D.astype(np.float16), torch.from_numpy(D), torch.from_numpy(D).to(dev), torch.from_numpy(D).to(dev).half()):
        with pytest.raises(ValueError, match=match):
            cluster.DBSCAN(eps=0.1, min_samples=4, metric="precomputed").fit(X)
        with pytest.raises(ValueError, match=match):
            cluster.eps_rule_dbscan(X, 0.02, min_samples=4)
    D[3, 77] = D[77, 3] = -0.0                                       # a negative zero is no negative value
    assert cluster.DBSCAN(eps=0.1, min_samples=4, metric="precomputed").fit(D).labels_.shape == (120,)
