"""GPU half of the HDBSCAN tests: `ssg_amd.hdbscan.HDBSCAN` (csrc/hdbscan.hip) against what sklearn 1.7.2 gave for every case of
tests/hdbscan_ref.py (tests/golden/hdbscan_cases.npz).

What does not depend on a sort is compared bit for bit with the golden: the core distances and the three fields of every edge of the
spanning tree, from the entry points called by name, with the loop's state in LDS and in global memory.  What follows the sort of the tied
edge weights -- the single-linkage tree, the labels, the probabilities -- is compared with the restatement run on the golden spanning tree
with THIS machine's `np.argsort`, with the golden directly whenever this machine's order is the stored one (the test prints which held),
and with sklearn's live fit where sklearn imports.  Also: float16 / float32 input against the float64 copy; a mode-0 re-rank handle read
in place; the state beyond its LDS placement; the check pass on ragged tiles; one blocking read per fit; `generate_selflabel_hdbscan`."""
import warnings

import numpy as np
import pytest
import torch

import hdbscan_ref as ref

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in ref.CASES]
MST = ("mst_current", "mst_next", "mst_distance")
ASYM = "its values appear to be asymmetric"


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
    """the mode-0 handle re_ranking_device builds from the features of the re-rank golden whose final_dist the 'rerank' cases use"""
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


def _estimator(case, state=0):
    from ssg_amd import HDBSCAN
    est = HDBSCAN(metric="precomputed", min_cluster_size=case["min_cluster_size"], min_samples=case["min_samples"], alpha=case["alpha"],
                  cluster_selection_method=case["method"], allow_single_cluster=case["allow_single_cluster"], cluster_selection_epsilon=case["epsilon"],
                  max_cluster_size=case["max_cluster_size"])
    est.state = state
    return est


def _device_tree(L, h, k, alpha, state, dev):
    """the three entry points called by name on handle h -> (counts, core, current, next, distance) as numpy"""
    from ssg_amd._lib import check, ptr
    N = h.N
    counts = torch.full((2,), -7, dtype=torch.int64, device=dev)
    core = torch.full((N,), -1.0, dtype=torch.float64, device=dev)
    cur = torch.full((N - 1,), -7, dtype=torch.int64, device=dev)
    nxt = torch.full((N - 1,), -7, dtype=torch.int64, device=dev)
    dist = torch.full((N - 1,), -7.0, dtype=torch.float64, device=dev)
    ws = torch.empty(N + 2, dtype=torch.float64, device=dev)
    args = (ptr(h.M), ptr(h.v), N, h.mode, h.lambda_value)
    check(L.ssg_hdbscan_check(*args, ptr(counts), None), "ssg_hdbscan_check")
    check(L.ssg_hdbscan_core_dist(*args, k, alpha, ptr(core), None), "ssg_hdbscan_core_dist")
    check(L.ssg_hdbscan_mst(*args, ptr(core), alpha, state, ptr(ws), N * 8, ptr(cur), ptr(nxt), ptr(dist), None), "ssg_hdbscan_mst")
    return counts.cpu().numpy(), core.cpu().numpy(), cur.cpu().numpy(), nxt.cpu().numpy(), dist.cpu().numpy()


@pytest.mark.parametrize("state", [1, 2], ids=["lds", "global"])
@pytest.mark.parametrize("name", NAMES)
def test_entry_points_give_the_golden_tree_bit_for_bit(gold, dev, rerank_handle, name, state):
    """ssg_hdbscan_check, ssg_hdbscan_core_dist and ssg_hdbscan_mst by name, every case, both placements of the loop's state: no NaN, no
    asymmetric pair, sklearn's core distances and all three fields of every edge in Prim order -- the claim that depends on no sort"""
    from ssg_amd import _lib, hdbscan
    case = ref.BY_NAME[name]
    h = hdbscan._as_handle(_input(case, rerank_handle))
    assert h.mode == {"half": 1, "inf": 1, "rerank": 0}.get(case["kind"], 2)
    counts, core, cur, nxt, dist = _device_tree(_lib.lib(), h, ref.min_samples_of(case), case["alpha"], state, dev)
    assert counts.tolist() == [0, 0], name
    assert _same_bits(core, gold[name + "/core"]), name
    for got, key in zip((cur, nxt, dist), MST):
        assert _same_bits(got, gold["%s/%s" % (name, key)]), (name, key)


@pytest.mark.parametrize("name", NAMES)
def test_fit_is_sklearn(gold, dev, rerank_handle, name, monkeypatch):
    """the whole fit: tree, labels_, probabilities_ and the two cuts against the restatement on the golden spanning tree with this
    machine's np.argsort; against the golden itself when this machine sorts the ties as the golden's machine did; against sklearn's
    live fit where sklearn imports; one blocking read"""
    from ssg_amd import hdbscan
    case = ref.BY_NAME[name]
    reads = []
    real = hdbscan._read_back
    monkeypatch.setattr(hdbscan, "_read_back", lambda *t: reads.append(len(t)) or real(*t))
    est = _estimator(case)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        assert est.fit(_input(case, rerank_handle)) is est
    assert len(reads) == 1, "one blocking read per fit"
    warned = any("edge weights with value infinity" in str(w.message) for w in caught)
    assert warned == bool(gold[name + "/warned"]), name
    for got, key in zip(est._mst, MST):
        assert _same_bits(got, gold["%s/%s" % (name, key)]), (name, key)
    assert est.n_features_in_ == case["N"] and est._min_samples == ref.min_samples_of(case)
    tree = est._single_linkage_tree_
    assert tree.dtype.names == ("left_node", "right_node", "value", "cluster_size") and tree.shape == (case["N"] - 1,)
    assert est.labels_.dtype == np.int64 and est.probabilities_.dtype == np.float64
    cuts = [est.dbscan_clustering(cut, min_cluster_size=case["min_cluster_size"]) for cut in case["cuts"]]

    def compare(want, what):
        for field, key in (("left_node", "slt_left"), ("right_node", "slt_right"), ("value", "slt_value"), ("cluster_size", "slt_size")):
            assert _same_bits(tree[field].astype(want[key].dtype), want[key]), (name, what, field)
        assert np.array_equal(est.labels_, want["labels"]) and _same_bits(est.probabilities_, want["probs"]), (name, what)
        for i in range(len(cuts)):
            assert np.array_equal(cuts[i], want["cut%d" % i]), (name, what, i)

    here = np.argsort(gold[name + "/mst_distance"])
    compare(ref.run_case(case, *(gold["%s/%s" % (name, k)] for k in MST), here), "restatement with this machine's argsort")
    same_order = np.array_equal(here, gold[name + "/row_order"])
    print("%s: this machine sorts the tied edges %s" % (name, "as the golden's machine did" if same_order else "in another order than the golden's machine"))
    if same_order:
        compare({k: gold["%s/%s" % (name, k)] for k in ("slt_left", "slt_right", "slt_value", "slt_size", "labels", "probs", "cut0", "cut1")}, "golden")
    try:
        from sklearn.cluster import HDBSCAN as SkHDBSCAN
    except ImportError:
        return
    sk = SkHDBSCAN(metric="precomputed", min_cluster_size=case["min_cluster_size"], min_samples=case["min_samples"], alpha=case["alpha"],
                   cluster_selection_method=case["method"], allow_single_cluster=case["allow_single_cluster"], cluster_selection_epsilon=case["epsilon"],
                   max_cluster_size=case["max_cluster_size"], copy=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk.fit(np.array(ref.matrix(case), dtype=np.float64))
    st = sk._single_linkage_tree_
    live = dict(slt_left=st["left_node"].astype(np.int64), slt_right=st["right_node"].astype(np.int64), slt_value=st["value"].copy(),
                slt_size=st["cluster_size"].astype(np.int64), labels=sk.labels_, probs=sk.probabilities_)
    for i, cut in enumerate(case["cuts"]):
        live["cut%d" % i] = sk.dbscan_clustering(cut, min_cluster_size=case["min_cluster_size"])
    compare(live, "sklearn's live fit")


@pytest.mark.parametrize("name", ["n64_half", "n257_half_a15", "n257_inf", "n513_half_ms1"])
def test_half_and_float32_matrices_give_the_float64_copy_s_result(gold, dev, name):
    """sklearn widens a float16 / float32 matrix to float64 before anything else: numpy and torch, host and device, float16 (mode 1),
    float32 and float64 all give the golden tree of the float64 copy, and the same labels as each other"""
    case = ref.BY_NAME[name]
    D = ref.matrix(case)
    assert D.dtype == np.float16
    inputs = {"numpy f16": D, "numpy f32": D.astype(np.float32), "numpy f64": D.astype(np.float64), "torch f16 cuda": torch.from_numpy(np.ascontiguousarray(D)).to(dev),
              "torch f32 cpu": torch.from_numpy(D.astype(np.float32)), "torch f64 cuda": torch.from_numpy(D.astype(np.float64)).to(dev)}
    first = None
    for what, X in inputs.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            est = _estimator(case).fit(X)
        for got, key in zip(est._mst, MST):
            assert _same_bits(got, gold["%s/%s" % (name, key)]), (name, what, key)
        assert _same_bits(est._core_distances, gold[name + "/core"]), (name, what)
        if first is None:
            first = est
        assert np.array_equal(est.labels_, first.labels_) and _same_bits(est.probabilities_, first.probabilities_), (name, what)
        assert est._single_linkage_tree_.tobytes() == first._single_linkage_tree_.tobytes(), (name, what)


def test_rerank_handle_is_read_in_place(gold, golden, dev, rerank_handle):
    """the mode-0 handle is read through its compact form: a fit allocates nothing of the size of the float64 matrix (sklearn widens to
    8 N^2 bytes and overwrites them); a second fit gives identical bits; a handle whose status words are still pending is validated
    first; the DeviceBackedArray re_ranking returns carries its handle; the caller's matrix is never modified"""
    from ssg_amd import re_ranking, rerank
    case = ref.BY_NAME["rerank_n256"]
    N = case["N"]
    est = _estimator(case).fit(rerank_handle)                  # (warm: the pinned pool and the library are in place)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    Mbits = rerank_handle.M.clone()
    est2 = _estimator(case, state=2).fit(rerank_handle)
    assert torch.cuda.max_memory_allocated() - before < 8 * N * N // 4 + 2 * N * N, "a float64 N x N allocation during fit"
    assert torch.equal(rerank_handle.M, Mbits)
    for a in ("labels_", "probabilities_"):
        assert _same_bits(getattr(est, a), getattr(est2, a)), a
    assert est._single_linkage_tree_.tobytes() == est2._single_linkage_tree_.tobytes()
    for got, key in zip(est2._mst, MST):
        assert _same_bits(got, gold["rerank_n256/" + key]), key
    g = golden(case["file"])
    src, tgt = torch.from_numpy(g["src"]).to(dev), torch.from_numpy(g["tgt"]).to(dev)
    h2 = rerank.re_ranking_device(src, tgt, k1=int(g["k1"]), k2=int(g["k2"]), lambda_value=case["lambda_value"], validate=False)
    est3 = _estimator(case).fit(h2)
    assert np.array_equal(est3.labels_, est.labels_)
    _, f = re_ranking(g["src"], g["tgt"], k1=int(g["k1"]), k2=int(g["k2"]), lambda_value=case["lambda_value"])
    est4 = _estimator(case)
    assert np.array_equal(est4.fit_predict(f), est.labels_) and _same_bits(est4.probabilities_, est.probabilities_)
    # copy is accepted and changes nothing: the input is never written
    from ssg_amd import HDBSCAN
    X = np.array(ref.matrix(case))
    keep = X.copy()
    for copy in (False, True):
        e = HDBSCAN(metric="precomputed", min_cluster_size=4, copy=copy).fit(X)
        assert np.array_equal(X, keep) and np.array_equal(e.labels_, est.labels_)


def test_state_beyond_the_lds_placement(dev):
    """N just above ssg_hdbscan_lds_max_n() and not a multiple of 8: state 1 is refused, auto and global give the numpy restatement's
    spanning tree bit for bit (core distances: the device's, checked against torch.kthvalue)"""
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr
    L = _lib.lib()
    N = L.ssg_hdbscan_lds_max_n() + 5
    assert N % 8 != 0 and N % 2 == 1
    g = torch.Generator(device=dev).manual_seed(4)
    pts = torch.rand((N, 3), device=dev, generator=g)
    M = torch.cdist(pts, pts).to(torch.float16)
    M = torch.minimum(M, M.T).contiguous()
    core = torch.empty(N, dtype=torch.float64, device=dev)
    check(L.ssg_hdbscan_core_dist(ptr(M), None, N, 1, 0.0, 4, 1.0, ptr(core), None), "ssg_hdbscan_core_dist")
    assert torch.equal(core, torch.kthvalue(M.to(torch.float32), 4, dim=1).values.to(torch.float64))
    cur = torch.empty(N - 1, dtype=torch.int64, device=dev)
    nxt, dist, ws = torch.empty_like(cur), torch.empty(N - 1, dtype=torch.float64, device=dev), torch.empty(N + 1, dtype=torch.float64, device=dev)
    assert L.ssg_hdbscan_mst(ptr(M), None, N, 1, 0.0, ptr(core), 1.0, 1, ptr(ws), N * 8, ptr(cur), ptr(nxt), ptr(dist), None) == -1
    assert L.ssg_hdbscan_mst(ptr(M), None, N, 1, 0.0, ptr(core), 1.0, 0, None, 0, ptr(cur), ptr(nxt), ptr(dist), None) == -1
    res = []
    for state in (0, 2):
        cur.fill_(-7); nxt.fill_(-7); dist.fill_(-7.0)
        check(L.ssg_hdbscan_mst(ptr(M), None, N, 1, 0.0, ptr(core), 1.0, state, ptr(ws), N * 8, ptr(cur), ptr(nxt), ptr(dist), None), "ssg_hdbscan_mst")
        res.append((cur.cpu().numpy(), nxt.cpu().numpy(), dist.cpu().numpy()))
    want = ref.prim(M.cpu().numpy(), core.cpu().numpy())
    for got in res:
        for a, b, what in zip(got, want, MST):
            assert _same_bits(a, b), what
    assert len(np.unique(want[2])) < N // 2                    # tie-heavy: float16 distances


def _counts(L, X, dev):
    from ssg_amd._lib import check, ptr
    M = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
    counts = torch.full((2,), -7, dtype=torch.int64, device=dev)
    check(L.ssg_hdbscan_check(ptr(M), None, len(X), 1 if X.dtype == np.float16 else 2, 0.0, ptr(counts), None), "ssg_hdbscan_check")
    return counts.tolist()


def test_check_pass_on_ragged_tiles(dev):
    """N = 257: five 64-wide tiles of which the last holds one row and one column.  ssg_hdbscan_check counts every ordered pair that
    fails numpy's isclose rule and every NaN, wherever it lies; fit raises sklearn's errors from those counts, NaN first"""
    from ssg_amd import HDBSCAN, _lib
    L = _lib.lib()
    base = np.array(ref.matrix(ref.BY_NAME["n257_dup"]), dtype=np.float64)
    N = len(base)
    assert N == 257 and np.array_equal(base, base.T) and _counts(L, base, dev) == [0, 0]
    fit = lambda X: HDBSCAN(metric="precomputed", min_cluster_size=4).fit(X)      # noqa: E731
    want = fit(base).labels_
    for (i, j) in ((10, 20), (20, 10), (70, 5), (256, 3), (3, 256), (256, 200), (130, 129)):      # inside a tile, across tiles, the ragged row and column
        X = base.copy()
        X[i, j] += 1e-3
        assert _counts(L, X, dev) == [0, 2], (i, j)            # (i, j) against (j, i) and (j, i) against (i, j)
        with pytest.raises(ValueError, match=ASYM):
            fit(X)
        X = base.copy()
        X[i, j] += 1e-12
        assert _counts(L, X, dev) == [0, 0], (i, j)
        assert fit(X).labels_.shape == want.shape              # accepted (the labels may move: the weights are tied)
    # the bound is relative to the SECOND value: a pair of which only one direction violates it
    d = 0.1 + 0.5e-9
    for (i, j) in ((10, 20), (20, 10), (3, 256), (256, 3), (100, 101)):
        X = base.copy()
        X[i, j], X[j, i] = 1e6, 1e6 - d
        assert not np.isclose(X[i, j], X[j, i], rtol=1e-7, atol=1e-9) and np.isclose(X[j, i], X[i, j], rtol=1e-7, atol=1e-9)
        assert _counts(L, X, dev) == [0, 1], (i, j)
        assert not np.allclose(X, X.T, rtol=1e-7, atol=1e-9)
        with pytest.raises(ValueError, match=ASYM):
            fit(X)
    # the whole count against numpy on a matrix with many violations, float64 and float16
    rs = np.random.RandomState(1)
    X = base + np.where(rs.uniform(size=base.shape) < 0.01, 1e-4 * rs.standard_normal(base.shape), 0.0)
    assert _counts(L, X, dev) == [0, int((~np.isclose(X, X.T, rtol=1e-7, atol=1e-9)).sum())]
    H = np.array(ref.matrix(ref.BY_NAME["n257_half"]))
    H[rs.randint(0, N, 50), rs.randint(0, N, 50)] = np.float16(7.0)
    H64 = H.astype(np.float64)
    assert _counts(L, H, dev) == [0, int((~np.isclose(H64, H64.T, rtol=1e-7, atol=1e-9)).sum())]
    # one NaN anywhere: sklearn's NaN error, which wins over the asymmetry it also is
    for (i, j) in ((5, 7), (256, 256), (256, 0), (64, 63)):
        X = base.copy()
        X[i, j] = np.nan
        X[11, 12] += 1e-3
        c = _counts(L, X, dev)
        assert c[0] == 1 and c[1] >= 2, (i, j)
        with pytest.raises(ValueError, match="np.nan values found in precomputed-dense"):
            fit(X)
    # inf matched by inf passes (and warns only if an edge is infinite); inf against a finite value is asymmetric
    X = base.copy()
    X[4, 200] = X[200, 4] = np.inf
    X[256, 9] = X[9, 256] = np.inf
    assert _counts(L, X, dev) == [0, 0]
    fit(X)
    X[256, 9] = base[256, 9]
    assert _counts(L, X, dev) == [0, 2]
    with pytest.raises(ValueError, match=ASYM):
        fit(X)
    # min_samples larger than N: the NaN is reported first, as sklearn does
    X = base.copy()
    with pytest.raises(ValueError, match=r"min_samples \(300\) must be at most the number of samples in X \(257\)"):
        HDBSCAN(metric="precomputed", min_samples=300).fit(X)
    X[3, 3] = np.nan
    with pytest.raises(ValueError, match="np.nan values found in precomputed-dense"):
        HDBSCAN(metric="precomputed", min_samples=300).fit(X)


def test_generate_selflabel_hdbscan(gold, dev, rerank_handle, capsys):
    """the grouping step with HDBSCAN over two iterations: estimator cached at iteration 0, the reference's two printed lines, labels
    equal to HDBSCAN(...).fit_predict on the same handle; the args reach the estimator"""
    from types import SimpleNamespace
    from ssg_amd import HDBSCAN, generate_selflabel_hdbscan
    h = rerank_handle
    want = HDBSCAN(metric="precomputed", min_cluster_size=4).fit_predict(h)
    assert want.max() + 1 == 16 and _same_bits(HDBSCAN(metric="precomputed", min_cluster_size=4).fit(h)._mst[2], gold["rerank_n256/mst_distance"])
    args = SimpleNamespace(no_rerank=False)
    labels, cl = generate_selflabel_hdbscan([[]], [h], 0, args, cluster_list=[])
    assert len(cl) == 1 and isinstance(cl[0], HDBSCAN) and np.array_equal(labels[0], want)
    assert (cl[0].min_cluster_size, cl[0].min_samples, cl[0].cluster_selection_method, cl[0].cluster_selection_epsilon, cl[0].allow_single_cluster) == (4, None, "eom", 0.0, False)
    out = capsys.readouterr().out
    assert "Clustering and labeling..." in out and "Iteration 1 have 16 training ids" in out and "eps in cluster" not in out
    labels2, cl2 = generate_selflabel_hdbscan([[]], [h], 1, args, cluster_list=cl)
    assert cl2[0] is cl[0] and np.array_equal(labels2[0], want) and "Iteration 2 have 16 training ids" in capsys.readouterr().out
    assert cl[0].probabilities_.shape == (256,) and ((cl[0].probabilities_ > 0) == (want >= 0)).all()
    args = SimpleNamespace(no_rerank=False, hdbscan_min_cluster_size=10, hdbscan_min_samples=3, hdbscan_method="leaf", hdbscan_epsilon=0.6,
                           hdbscan_allow_single_cluster=True)
    labels3, cl3 = generate_selflabel_hdbscan([[]], [h], 0, args, cluster_list=[])
    e = HDBSCAN(metric="precomputed", min_cluster_size=10, min_samples=3, cluster_selection_method="leaf", cluster_selection_epsilon=0.6, allow_single_cluster=True)
    assert np.array_equal(labels3[0], e.fit_predict(h)) and cl3[0]._min_samples == 3
    assert "Iteration 1 have %d training ids" % len(set(labels3[0][labels3[0] >= 0].tolist())) in capsys.readouterr().out
