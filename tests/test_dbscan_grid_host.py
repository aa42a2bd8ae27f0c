"""CPU suite: tests/golden/dbscan_grid.npz (sklearn 1.7.2's DBSCAN(metric='precomputed') over the min_samples / eps / dtype / N range
`ssg_amd.cluster.DBSCAN` accepts, tools/make_golden.py --only-dbscan-grid) against the visiting-order restatement of
tests/dbscan_grid_ref.py and against the C oracle, and the case table against what it claims to cover.
tests/test_gpu_dbscan_grid.py runs the same cases through the HIP path."""
import numpy as np
import pytest

import dbscan_grid_ref as grid

NAMES = [c.name for c in grid.CASES]


@pytest.fixture(scope="module")
def g(golden):
    return golden(grid.FIXTURE)


def test_fixture_holds_the_table(g):
    assert g["names"].tolist() == NAMES and len(grid.CASES) == 52
    for c in grid.CASES:
        if c.N > 1100:
            continue                             # (the 4096-point matrices are pinned where they are used, case by case, below)
        D = grid.matrix(c)
        assert D.shape == (c.N, c.N) and D.dtype == np.dtype(c.dtype) and D.flags.c_contiguous
        assert grid.sha(D) == str(g[c.name + "__sha"]), c.name
        assert (c.name + "__labels" in g.files) == (c.eps > 0) and (c.name + "__chain_eps" in g.files) == (c.rho is not None), c.name
        if c.container.startswith("numpy"):
            X = grid.as_passed(c)
            assert np.array_equal(X, D) and X.flags.c_contiguous == (c.container == "numpy"), c.name
    assert all(c.N >= 64 for c in grid.CHAIN) and max(c.N for c in grid.CASES) == 4096
    assert len(grid.PLAIN) == 51 and len(grid.CHAIN) == 9


@pytest.mark.parametrize("name", NAMES)
def test_restatement_and_oracle_reproduce_sklearn(name, g, ora):
    """the visiting-order restatement equals the recorded sklearn labels and core set on the matrix as the case passes it; so does the C
    oracle on the float64 cases; the case has the property it is in the table for, recomputed from the restatement"""
    c = grid.BY_NAME[name]
    D = grid.matrix(c)
    assert grid.sha(D) == str(g[name + "__sha"])
    m = grid.check_claims(c)
    if c.eps > 0:
        want, core = g[name + "__labels"], g[name + "__core"]
        assert want.dtype == np.int32 and np.array_equal(m["labels"], want), "restatement vs sklearn: labels"
        assert np.array_equal(m["core"], core), "restatement vs sklearn: core samples"
        assert np.array_equal(m["core"], np.nonzero(m["counts"] >= c.ms)[0])
        if c.dtype == "float64":
            assert np.array_equal(ora.dbscan(D, c.eps, c.ms), want), "oracle vs sklearn"
    if c.rho is not None:
        eps, cnt, top = grid.chain_reference(c)
        assert (float(eps), cnt, top) == (float(g[name + "__chain_eps"]), int(g[name + "__chain_count"]), int(g[name + "__chain_top"]))
        if c.dtype != "float32":
            oeps, ocnt, otop = ora.eps_rule(D, c.rho)
            assert (float(oeps), ocnt, otop) == (float(eps), cnt, top), "oracle eps rule"
        for ms in grid.CHAIN_MS:
            lab, _ = grid.dbscan_ref(D, float(eps), ms)
            assert np.array_equal(lab, g[name + "__chain_labels%d" % ms]), "restatement vs sklearn at the eps rule's radius, min_samples %d" % ms
            if c.dtype == "float64":
                assert np.array_equal(ora.dbscan(D, float(eps), ms), lab)


def test_float32_is_compared_in_float32_and_half_in_float64(g):
    """what the product's `compare_eps` rests on, read from the recorded sklearn answers: on the float32 cases where float32(eps) != eps
    changes a hit, sklearn's labels are those of the float32 comparison and not those of the widened matrix; on the half cases where
    float16(eps) would add hits, sklearn's labels are those of the float64 comparison"""
    seen32 = seen16 = 0
    for c in grid.PLAIN:
        D = grid.matrix(c)
        want = g[c.name + "__labels"]
        if c.claims.get("f32_eps_matters"):
            wide = grid.dbscan_ref(D.astype(np.float64), c.eps, c.ms)[0]
            assert not np.array_equal(wide, want) and np.array_equal(grid.dbscan_ref(D.astype(np.float64), float(np.float32(c.eps)), c.ms)[0], want)
            seen32 += 1
        if c.claims.get("f16_eps_would_matter"):
            inhalf = [np.nonzero(D[i] <= np.float16(c.eps))[0] for i in range(c.N)]
            assert not np.array_equal(grid.dbscan_ref(D, c.eps, c.ms, inhalf)[0], want)
            assert np.array_equal(grid.dbscan_ref(D.astype(np.float64), c.eps, c.ms)[0], want)
            seen16 += 1
    assert seen32 >= 2 and seen16 >= 2
    x = np.float32(0.1)
    assert grid.dbscan_ref(np.array([[0, x], [x, 0]], np.float32), 0.1, 2)[0].tolist() == [0, 0]
    assert grid.dbscan_ref(np.array([[0, x], [x, 0]], np.float64), 0.1, 2)[0].tolist() == [-1, -1]
    assert grid.dbscan_ref(np.array([[.7, .1], [.1, .7]]), 0.5, 2)[0].tolist() == [-1, -1]


def test_table_sits_on_both_sides_of_every_branch():
    """at least one case on each side of every branch of the issue's axes: the row streaming's size arithmetic (`grid.branches`, restated
    from csrc/matview.h), the three matrix modes, the containers, min_samples against the neighbour counts, eps against the entries"""
    cases = grid.PLAIN
    br = {c.name: grid.branches(c) for c in grid.CASES}

    def some(pred, among=cases):
        return [c.name for c in among if pred(c)]

    # N: the issue's list, all of it
    assert sorted(set(c.N for c in grid.CASES)) == [1, 2, 6, 7, 8, 9, 10, 17, 63, 64, 65, 120, 300, 511, 512, 513, 520, 1031, 4096]
    # rows that start on / off the 8-element boundary, in half (16-byte loads) and in double; fewer than 8 elements in all; one lane exactly
    for dt in ("float16", "float64"):
        assert some(lambda c: c.dtype == dt and br[c.name]["rows_aligned"]) and some(lambda c: c.dtype == dt and not br[c.name]["rows_aligned"] and c.N > 8)
    assert some(lambda c: br[c.name]["below_lane"] and c.N > 2) and some(lambda c: c.N == 8)
    # one chunk of 512: below, exactly, one element more, a partial second chunk on aligned rows, three chunks, eight
    assert some(lambda c: c.N == 511) and some(lambda c: br[c.name]["exact_chunks"] and br[c.name]["chunks"] == 1) and some(lambda c: c.N == 513)
    assert some(lambda c: br[c.name]["rows_aligned"] and not br[c.name]["exact_chunks"] and br[c.name]["chunks"] == 2)
    assert some(lambda c: br[c.name]["chunks"] == 3) and some(lambda c: br[c.name]["chunks"] == 8)
    # the last row's tail guard `off + 8 <= total`: the matrix ends inside / at the end of a lane's 8 elements
    for dt in ("float16", "float64"):
        assert some(lambda c: c.dtype == dt and br[c.name]["last_row_tail_inside_lane"]) and some(lambda c: c.dtype == dt and not br[c.name]["last_row_tail_inside_lane"])
    # dtypes and containers
    for dt in ("float64", "float32", "float16"):
        assert some(lambda c: c.dtype == dt and c.container == "numpy") and some(lambda c: c.dtype == dt and c.container == "gpu"), dt
    assert some(lambda c: c.container == "cpu") and some(lambda c: c.container == "numpy_T") and some(lambda c: c.container == "numpy_slice")
    assert some(lambda c: c.container == "cpu_T")
    # min_samples: every value of the issue's list, N and N + 1
    assert set((1, 2, 3, 4, 5, 10, 65, 200)) <= set(c.ms for c in cases)
    assert some(lambda c: c.ms == c.N and c.N > 2) and some(lambda c: c.ms == c.N + 1 and c.N > 2) and some(lambda c: c.ms == c.N + 1 and c.N == 1)
    assert some(lambda c: c.ms > grid.EDGES_PER_ROW and "counts_straddle" in c.claims)
    # eps: below every off-diagonal entry (noise / singletons), ordinary, equal to entries, above every entry, not representable
    assert some(lambda c: "none_hit" in c.claims and c.ms == 1) and some(lambda c: "none_hit" in c.claims and c.ms > 1)
    assert some(lambda c: "eps_equals_entries" in c.claims and c.dtype == "float16") and some(lambda c: "eps_equals_entries" in c.claims and c.dtype == "float32")
    assert some(lambda c: "all_hit" in c.claims) and some(lambda c: c.gen == "plane" and not c.claims)
    assert some(lambda c: c.claims.get("f32_eps_matters") is True and c.N > 2) and some(lambda c: c.claims.get("f32_eps_matters") is False and c.N > 2)
    assert some(lambda c: "f16_eps_would_matter" in c.claims and c.N > 2)
    # diagonal: zero, above eps, mixed
    assert some(lambda c: c.diag == "above" and c.N > 2) and some(lambda c: c.diag == "mixed" and c.ms == 1) and some(lambda c: c.diag == "zero")
    # structure
    assert some(lambda c: c.gen == "dups") and some(lambda c: c.gen == "paths" and c.arg == (1, False) and c.N == 4096 and c.ms == 3)
    assert some(lambda c: c.gen == "paths" and c.arg[0] == 2) and some(lambda c: c.gen == "paths" and c.arg[0] == 5)
    assert some(lambda c: c.gen == "paths" and c.claims.get("n_clusters") == 0) and some(lambda c: "cores_alternate" in c.claims)
    assert some(lambda c: c.claims.get("border_ties") == 2) and some(lambda c: c.claims.get("border_ties") == 3) and some(lambda c: "noise_next_to_border" in c.claims)
    # the edge list: a case within the first capacity and one above it, for fit and for the one-read chain
    assert some(lambda c: "hits_above_capacity" in c.claims) and some(lambda c: "chain_hits_above_capacity" in c.claims, grid.CHAIN)
    assert grid.edge_capacity(300) == 65536 < 300 * 300 and grid.edge_capacity(4096) == 64 * 4096
    # the one-read chain: every dtype, N on and off the boundary
    for dt in ("float64", "float32", "float16"):
        assert some(lambda c: c.dtype == dt, grid.CHAIN), dt
    assert some(lambda c: c.N % 8 == 0, grid.CHAIN) and some(lambda c: c.N % 8 != 0, grid.CHAIN)


def test_capacity_formula_is_the_library_s():
    """`grid.edge_capacity` is restated from cluster.py: both places that size the first edge list still read as the table assumes"""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "self-similarity-grouping_amd", "cluster.py")).read()
    assert "cap = max(64 * mx_rows, 1 << 16)" in src and "ecap = max(64 * h.nrows, 1 << 16)" in src
    assert grid.EDGES_PER_ROW == 64 and grid.MIN_EDGE_CAP == 1 << 16


def test_compare_eps_rounds_for_a_float32_matrix_only():
    """`cluster.compare_eps` (no GPU needed): float64(float32(eps)) for a handle that remembers a float32 matrix, eps itself otherwise;
    with it the float64 comparison the kernels make selects exactly the hits of sklearn's float32 comparison on every float32 case"""
    from types import SimpleNamespace
    from ssg_amd import cluster
    f32, other = SimpleNamespace(eps_f32=True), SimpleNamespace(eps_f32=False)
    assert cluster.compare_eps(f32, 0.1) == float(np.float32(0.1)) != 0.1 and cluster.compare_eps(other, 0.1) == 0.1
    assert cluster.compare_eps(f32, 1e39) == float("inf") and cluster.compare_eps(f32, np.float16(0.5)) == 0.5
    assert cluster.compare_eps(SimpleNamespace(), 0.3) == 0.3
    for c in grid.PLAIN:
        if c.dtype == "float32":
            D = grid.matrix(c)
            wide = [np.nonzero(D[i].astype(np.float64) <= cluster.compare_eps(f32, c.eps))[0] for i in range(c.N)]
            assert all(np.array_equal(a, b) for a, b in zip(wide, grid.neighbourhoods(D, c.eps))), c.name
