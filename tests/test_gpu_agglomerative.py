"""GPU half of the agglomerative tests: `ssg_amd.agglomerative` (csrc/agglomerative.hip) against what scipy 1.15.3 and sklearn 1.7.2 gave
for every case of tests/agglomerative_ref.py (tests/golden/agglomerative_cases.npz).

The three entry points are called by name: for every case, every linkage and both placements of the loop's state the merges in merge
order equal the restatement's bit for bit (the golden holds them).  Z, children_, distances_, n_clusters_ and labels_ equal scipy's and
sklearn's.  Also: float16 / float32 input against the float64 copy; a mode-0 re-rank handle read in place; the state beyond its LDS
placement; NaN and inf anywhere in the matrix; one blocking read per fit; the input unchanged; `generate_selflabel_agglomerative`."""
import numpy as np
import pytest
import torch

import agglomerative_ref as ref

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in ref.CASES]
METHOD = {"average": 0, "complete": 1, "single": 2}


@pytest.fixture(scope="module")
def gold():
    return ref.load_golden()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def rerank_handle(golden, dev):
    """the mode-0 handle re_ranking_device builds from the features of the re-rank golden whose final_dist the 'rerank' case uses"""
    from ssg_amd import rerank
    case = ref.BY_NAME["rerank_n256"]
    g = golden(case["file"])
    h = rerank.re_ranking_device(torch.from_numpy(g["src"]).to(dev), torch.from_numpy(g["tgt"]).to(dev), k1=int(g["k1"]), k2=int(g["k2"]),
                                 lambda_value=case["lambda_value"])
    assert h.mode == 0 and h.group is None
    assert np.array_equal(h.final_dist().cpu().numpy(), np.asarray(ref.matrix(case)))
    return h


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _input(case, rerank_handle):
    return rerank_handle if case["kind"] == "rerank" else ref.matrix(case)


def _device_loop(L, h, method, state, dev, ld=None):
    """the three entry points called by name on handle h -> (counts, flag, x, y, distance, size, W) as numpy; the outputs start at
    sentinels"""
    from ssg_amd._lib import check, ptr
    N = h.N
    ld = (N + 3) & ~3 if ld is None else ld
    counts = torch.full((2,), -7, dtype=torch.int64, device=dev)
    flag = torch.full((2,), -7, dtype=torch.int64, device=dev)
    W = torch.full((N, ld), -7.0, dtype=torch.float64, device=dev)
    x, y, size = (torch.full((N - 1,), -7, dtype=torch.int64, device=dev) for _ in range(3))
    dist = torch.full((N - 1,), -7.0, dtype=torch.float64, device=dev)
    ws = torch.empty(ld, dtype=torch.float64, device=dev)
    check(L.ssg_agglo_check(ptr(h.M), ptr(h.v), N, h.mode, h.lambda_value, ptr(counts), None), "ssg_agglo_check")
    check(L.ssg_agglo_expand(ptr(h.M), ptr(h.v), N, h.mode, h.lambda_value, ptr(W), ld, None), "ssg_agglo_expand")
    W0 = W.cpu().numpy()
    check(L.ssg_agglo_nn_chain(ptr(W), N, ld, method, state, ptr(counts), ptr(ws), ld * 8, ptr(x), ptr(y), ptr(dist), ptr(size), ptr(flag), None), "ssg_agglo_nn_chain")
    return counts.cpu().numpy(), flag.cpu().numpy(), x.cpu().numpy(), y.cpu().numpy(), dist.cpu().numpy(), size.cpu().numpy(), W0


@pytest.mark.parametrize("state", [1, 2], ids=["lds", "global"])
@pytest.mark.parametrize("name", NAMES)
def test_entry_points_give_the_merges_bit_for_bit(gold, dev, rerank_handle, name, state):
    """ssg_agglo_check, ssg_agglo_expand and ssg_agglo_nn_chain by name, every case, all three linkages, both placements of the loop's
    state: no NaN, no inf, the working square is the upper triangle on both sides, and both slots, the height and the size of every
    merge in merge order are the restatement's"""
    from ssg_amd import _lib, hdbscan
    case = ref.BY_NAME[name]
    N = case["N"]
    h = hdbscan._as_handle(_input(case, rerank_handle))
    assert h.mode == {"q16": 1, "rerank": 0}.get(case["kind"], 2)
    want_W = ref.square(ref.matrix(case))
    np.fill_diagonal(want_W, 0.0)
    for method in ref.LINKAGES:
        key = "%s/%s" % (name, method)
        counts, flag, x, y, d, s, W0 = _device_loop(_lib.lib(), h, METHOD[method], state, dev)
        assert counts.tolist() == [0, 0] and flag[0] == 0, key
        assert _same_bits(W0[:, :N], want_W) and (W0[:, N:] == -7.0).all(), key
        assert _same_bits(x, gold[key + "/x"]) and _same_bits(y, gold[key + "/y"]) and _same_bits(d, gold[key + "/d"]), key
        if method == "single":
            assert (s == -7).all() and flag[1] == N - 1
        else:
            assert _same_bits(s, gold[key + "/size"]) and 0 < flag[1] <= 3 * (N - 1), key


@pytest.mark.parametrize("method", ref.LINKAGES)
@pytest.mark.parametrize("name", NAMES)
def test_fit_is_sklearn(gold, dev, rerank_handle, name, method, monkeypatch):
    """linkage() gives scipy's Z; the estimator gives sklearn's children_, distances_, n_clusters_, n_leaves_, n_connected_components_,
    n_features_in_ and labels_ for n_clusters in {1, 2, 7, N} and for thresholds below the first merge, between two merges, equal to
    a merge height and above the last; one blocking read per fit; the input is unchanged"""
    from ssg_amd import AgglomerativeClustering, agglomerative
    case, key = ref.BY_NAME[name], "%s/%s" % (name, method)
    N = case["N"]
    X = _input(case, rerank_handle)
    keep = X.M.clone() if case["kind"] == "rerank" else np.array(X)
    reads = []
    real = agglomerative._read_back
    monkeypatch.setattr(agglomerative, "_read_back", lambda *t: reads.append(len(t)) or real(*t))
    Z = agglomerative.linkage(X, method)
    assert len(reads) == 1 and Z.dtype == np.float64 and _same_bits(Z, gold[key + "/Z"]), key
    fits = [("k%d" % k, k, None) for k in ref.n_clusters_options(N)] + [("t%d" % i, None, float(t)) for i, t in enumerate(gold[key + "/thresholds"])]
    for tag, k, t in fits:
        del reads[:]
        est = AgglomerativeClustering(n_clusters=k, distance_threshold=t, metric="precomputed", linkage=method, compute_distances=(tag == "k2"))
        assert est.fit(X) is est and len(reads) == 1, "one blocking read per fit"
        assert est.children_.dtype == np.int64 and _same_bits(est.children_.astype(np.float64), gold[key + "/Z"][:, :2]), (key, tag)
        if t is not None or tag == "k2":
            assert _same_bits(est.distances_, gold[key + "/Z"][:, 2]), (key, tag)
        else:
            assert not hasattr(est, "distances_")
        assert (est.n_leaves_, est.n_connected_components_, est.n_features_in_) == (N, 1, N)
        assert est.n_clusters_ == int(gold["%s/%s/n_clusters" % (key, tag)]) and type(est.n_clusters_) is int, (key, tag)
        assert est.labels_.dtype == np.int64 and np.array_equal(est.labels_, gold["%s/%s/labels" % (key, tag)]), (key, tag)
    assert torch.equal(X.M, keep) if case["kind"] == "rerank" else np.array_equal(np.array(X), keep)
    with pytest.raises(ValueError, match="Cannot extract more clusters than samples: %d clusters were given for a tree with %d leaves" % (N + 1, N)):
        AgglomerativeClustering(n_clusters=N + 1, metric="precomputed", linkage=method).fit(X)


@pytest.mark.parametrize("name", ["n65_q16", "n257_q16"])
def test_half_and_float32_matrices_give_the_float64_copy_s_result(gold, dev, name):
    """scipy widens a float16 / float32 condensed matrix to float64 before anything else: numpy and torch, host and device, float16
    (mode 1), float32 and float64 all give the golden Z of the float64 copy, and the caller's matrix is never modified"""
    from ssg_amd import agglomerative
    D = ref.matrix(ref.BY_NAME[name])
    assert D.dtype == np.float16
    inputs = {"numpy f16": D, "numpy f32": D.astype(np.float32), "numpy f64": D.astype(np.float64), "torch f16 cuda": torch.from_numpy(np.ascontiguousarray(D)).to(dev),
              "torch f32 cpu": torch.from_numpy(D.astype(np.float32)), "torch f64 cuda": torch.from_numpy(D.astype(np.float64)).to(dev)}
    for what, X in inputs.items():
        keep = X.clone() if torch.is_tensor(X) else X.copy()
        for method in ref.LINKAGES:
            assert _same_bits(agglomerative.linkage(X, method), gold["%s/%s/Z" % (name, method)]), (name, what, method)
        assert torch.equal(X, keep) if torch.is_tensor(X) else np.array_equal(X, keep), what


def test_rerank_handle_and_the_array_re_ranking_returns(gold, golden, dev, rerank_handle):
    """the mode-0 handle is read through its compact form and left as it is; a handle whose status words are still pending is validated
    first; the DeviceBackedArray re_ranking returns carries its handle"""
    from ssg_amd import AgglomerativeClustering, re_ranking, rerank
    case = ref.BY_NAME["rerank_n256"]
    g = golden(case["file"])
    want = gold["rerank_n256/average/t1/labels"]
    t = float(gold["rerank_n256/average/thresholds"][1])
    fit = lambda X: AgglomerativeClustering(n_clusters=None, distance_threshold=t, metric="precomputed", linkage="average").fit_predict(X)      # noqa: E731
    Mbits = rerank_handle.M.clone()
    assert np.array_equal(fit(rerank_handle), want) and torch.equal(rerank_handle.M, Mbits)
    src, tgt = torch.from_numpy(g["src"]).to(dev), torch.from_numpy(g["tgt"]).to(dev)
    h2 = rerank.re_ranking_device(src, tgt, k1=int(g["k1"]), k2=int(g["k2"]), lambda_value=case["lambda_value"], validate=False)
    assert np.array_equal(fit(h2), want)
    _, f = re_ranking(g["src"], g["tgt"], k1=int(g["k1"]), k2=int(g["k2"]), lambda_value=case["lambda_value"])
    assert np.array_equal(fit(f), want)


def test_state_beyond_the_lds_placement(dev):
    """N just above ssg_agglo_lds_max_n(): state 1 is refused, auto without a workspace is refused; the global placement runs (auto
    picks it).  The matrix is built so that the merges are known: points on a line with growing gaps merge left to right under every
    linkage, N - 1 merges in 2 (N - 1) scans."""
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr
    L = _lib.lib()
    N = L.ssg_agglo_lds_max_n() + 5
    ld = (N + 3) & ~3
    pos = torch.cumsum(1.0 + torch.arange(N, dtype=torch.float64, device=dev) / N, 0)       # gaps 1 + i / N: strictly growing
    M = (pos[None, :] - pos[:, None]).abs().to(torch.float16).contiguous()               # only nearest neighbours matter; half keeps their order
    M = torch.triu(M, 1)                                                                  # the lower triangle is not looked at
    gaps = M.diagonal(1).to(torch.float64).cpu().numpy()
    assert (np.diff(gaps) >= 0).all() and gaps[0] < gaps[-1]
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    W = torch.empty((N, ld), dtype=torch.float64, device=dev)
    x, y, size = (torch.full((N - 1,), -7, dtype=torch.int64, device=dev) for _ in range(3))
    dist = torch.full((N - 1,), -7.0, dtype=torch.float64, device=dev)
    flag = torch.full((2,), -7, dtype=torch.int64, device=dev)
    ws = torch.empty(ld, dtype=torch.float64, device=dev)
    loop = lambda method, state, wsp, nbytes: L.ssg_agglo_nn_chain(ptr(W), N, ld, method, state, ptr(counts), wsp, nbytes, ptr(x), ptr(y), ptr(dist), ptr(size), ptr(flag), None)   # noqa: E731
    assert loop(1, 1, ptr(ws), ld * 8) == -1 and loop(1, 0, None, 0) == -1
    for method, state in ((1, 0), (2, 2)):
        check(L.ssg_agglo_expand(ptr(M), None, N, 1, 0.0, ptr(W), ld, None), "ssg_agglo_expand")
        check(loop(method, state, ptr(ws), ld * 8), "ssg_agglo_nn_chain")
        f = flag.cpu().numpy()
        assert f[0] == 0
        if method == 2:
            # Prim from node 0 walks the line: (i, i + 1, gap i)
            assert np.array_equal(x.cpu().numpy(), np.arange(N - 1)) and np.array_equal(y.cpu().numpy(), np.arange(1, N)) and _same_bits(dist.cpu().numpy(), gaps)
        else:
            # complete linkage: the chain from slot 0 finds 1 and merges (gap 0 is the smallest of all); the merged slot 1 is then
            # farther from 2 than 2 is from 3 ... until the far end, where the walk turns: every merge joins two neighbours on the line
            xs, ys, sz = x.cpu().numpy(), y.cpu().numpy(), size.cpu().numpy()
            assert (xs >= 0).all() and (xs < ys).all() and (ys < N).all() and sz[-1] == N and len(set(xs.tolist())) == N - 1
            assert 0 < f[1] <= 3 * (N - 1)
            assert np.isfinite(dist.cpu().numpy()).all()


def test_nan_and_inf_anywhere(dev):
    """N = 130: three 64-wide tiles of which the last holds two rows and two columns.  A NaN or an infinity anywhere -- the upper or
    lower triangle, the diagonal, the ragged tile -- is counted by ssg_agglo_check, the loop returns before it writes anything (its
    outputs keep their sentinels, the flag stays clear) and fit raises sklearn's error, NaN first"""
    from ssg_amd import AgglomerativeClustering, _lib, hdbscan
    from ssg_amd.agglomerative import _NAN
    L = _lib.lib()
    base = np.array(ref.matrix(ref.BY_NAME["n130_asym"]))
    N = len(base)
    fit = lambda X, **kw: AgglomerativeClustering(metric="precomputed", linkage="complete", **kw).fit(X)      # noqa: E731
    fit(base)
    for (i, j) in ((3, 100), (100, 3), (7, 7), (129, 129), (129, 0), (0, 129), (128, 129), (64, 63)):
        for bad, col in ((np.nan, 0), (np.inf, 1), (-np.inf, 1)):
            X = base.copy()
            X[i, j] = bad
            for dt in (np.float64, np.float16):
                h = hdbscan._as_handle(X.astype(dt))
                counts, flag, x, y, d, s, _ = _device_loop(L, h, 1, 0, dev)
                assert counts[col] == 1 and counts[1 - col] == 0, (i, j, bad)
                assert flag.tolist() == [0, 0] and (x == -7).all() and (y == -7).all() and (s == -7).all() and (d == -7.0).all(), (i, j, bad)
            with pytest.raises(ValueError) as e:
                fit(X)
            assert str(e.value) == (_NAN if col == 0 else "Input X contains infinity or a value too large for dtype('float64')."), (i, j, bad)
    X = base.copy()
    X[5, 9], X[100, 2], X[129, 129] = np.inf, np.nan, np.nan
    with pytest.raises(ValueError) as e:
        fit(X.astype(np.float32))
    assert str(e.value) == _NAN
    X[100, 2] = X[129, 129] = -np.inf
    with pytest.raises(ValueError) as e:
        fit(X.astype(np.float32))
    assert str(e.value) == "Input X contains infinity or a value too large for dtype('float32')."
    # sklearn validates X before its _fit refuses the parameters
    with pytest.raises(ValueError, match="infinity"):
        fit(X, n_clusters=2, distance_threshold=1.0)
    with pytest.raises(ValueError, match="Exactly one of n_clusters and distance_threshold"):
        fit(base, n_clusters=2, distance_threshold=1.0)
    with pytest.raises(ValueError, match="compute_full_tree must be True if distance_threshold is set."):
        fit(base, n_clusters=None, distance_threshold=1.0, compute_full_tree=False)


def test_generate_selflabel_agglomerative(gold, dev, rerank_handle, capsys):
    """the grouping step over two iterations: estimator cached at iteration 0, the cut from the rho rule printed with the reference's
    line and frozen, clusters below agglo_min_cluster_size turned into -1, the rest renumbered; the args reach the estimator"""
    from types import SimpleNamespace
    from ssg_amd import AgglomerativeClustering, cluster, generate_selflabel_agglomerative
    h = rerank_handle
    rho = 2e-2                                                    # (a cut at which this matrix shows eight clusters of four or more samples)
    eps = float(cluster.eps_rule(h, rho)[0])
    raw = AgglomerativeClustering(n_clusters=None, distance_threshold=eps, metric="precomputed", linkage="average").fit_predict(h)
    want = ref.drop_small(raw, 4)
    assert (want == -1).any() and want.max() >= 1
    args = SimpleNamespace(no_rerank=False, rho=rho)
    labels, cl = generate_selflabel_agglomerative([[]], [h], 0, args, cluster_list=[])
    assert len(cl) == 1 and isinstance(cl[0], AgglomerativeClustering) and np.array_equal(labels[0], want)
    assert (cl[0].linkage, cl[0].distance_threshold, cl[0].n_clusters, cl[0].metric) == ("average", eps, None, "precomputed")
    out = capsys.readouterr().out
    assert 'eps in cluster: {:.3f}'.format(eps) in out and "Clustering and labeling..." in out and "Iteration 1 have %d training ids" % (want.max() + 1) in out
    args2 = SimpleNamespace(no_rerank=False, rho=0.5)             # the cut is frozen: another rho changes nothing
    labels2, cl2 = generate_selflabel_agglomerative([[]], [h], 1, args2, cluster_list=cl)
    out = capsys.readouterr().out
    assert cl2[0] is cl[0] and np.array_equal(labels2[0], want) and "Iteration 2 have %d training ids" % (want.max() + 1) in out and "eps in cluster" not in out
    t = float(gold["rerank_n256/complete/thresholds"][1])
    args = SimpleNamespace(no_rerank=False, rho=rho, agglo_linkage="complete", agglo_threshold=t, agglo_min_cluster_size=2)
    labels3, cl3 = generate_selflabel_agglomerative([[]], [h], 0, args, cluster_list=[])
    assert np.array_equal(labels3[0], ref.drop_small(gold["rerank_n256/complete/t1/labels"], 2)) and cl3[0].distance_threshold == t
    assert "eps in cluster" not in capsys.readouterr().out
    args = SimpleNamespace(no_rerank=False, rho=rho, agglo_linkage="single", agglo_n_clusters=7, agglo_min_cluster_size=1)
    labels4, cl4 = generate_selflabel_agglomerative([[]], [h], 0, args, cluster_list=[])
    assert np.array_equal(labels4[0], ref.drop_small(gold["rerank_n256/single/k7/labels"], 1)) and cl4[0].n_clusters == 7 and cl4[0].distance_threshold is None
