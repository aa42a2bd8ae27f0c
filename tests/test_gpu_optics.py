"""GPU half of the OPTICS tests: `ssg_amd.optics.OPTICS` (csrc/optics.hip) against what sklearn 1.7.2 gave for every case of
tests/optics_ref.py (tests/golden/optics_cases.npz), bit for bit, with the loop's state in LDS and in global memory; the two entry
points called by name over the whole min_samples range; float16 / float32 input against the golden of the float64 copy; a mode-0
re-rank handle read through its compact form; a second fit; one blocking read per fit; `generate_selflabel_optics`."""
import warnings

import numpy as np
import pytest
import torch

import optics_ref as ref

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in ref.CASES]
FIELDS = ("ordering", "core", "reach", "pred")


@pytest.fixture(scope="module")
def gold():
    return ref.load_golden()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _estimator(case, cut, state=0):
    from ssg_amd import OPTICS
    est = OPTICS(metric="precomputed", min_samples=case["min_samples"], max_eps=case["max_eps"], cluster_method=cut["method"], eps=cut["eps"],
                 xi=cut["xi"], min_cluster_size=cut["min_cluster_size"], predecessor_correction=cut["predecessor_correction"])
    est.state = state
    return est


def _check_graph(est, gold, name, what=""):
    for attr, key in zip(("ordering_", "core_distances_", "reachability_", "predecessor_"), FIELDS):
        want = gold["%s/%s" % (name, key)]
        got = getattr(est, attr)
        assert got.dtype == (np.float64 if key in ("core", "reach") else np.int64), (name, attr)
        assert _same_bits(got, want.astype(got.dtype)), (name, attr, what)


def _check_cut(est, gold, name, i, cut, what=""):
    want = gold["%s/cut%d/labels" % (name, i)]
    assert est.labels_.shape == want.shape and np.array_equal(est.labels_, want), (name, i, what)
    if cut["method"] == "xi":
        wh = gold["%s/cut%d/hier" % (name, i)]
        assert est.cluster_hierarchy_.shape == wh.shape and np.array_equal(est.cluster_hierarchy_, wh), (name, i, what)


@pytest.mark.parametrize("state", [1, 2], ids=["lds", "global"])
@pytest.mark.parametrize("name", NAMES)
def test_optics_is_sklearn_bit_for_bit(gold, dev, name, state):
    """every case, both placements of the loop's state: the four arrays, labels_ and cluster_hierarchy_ of every cut"""
    from ssg_amd import cluster
    case = ref.BY_NAME[name]
    h = cluster.as_handle(ref.matrix(case))                 # kind 'half': a float16 matrix (mode 1); else float64 (mode 2)
    assert h.mode == (1 if case["kind"] == "half" else 2)
    for i, cut in enumerate(case["cuts"]):
        est = _estimator(case, cut, state)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            assert est.fit(h) is est
        warned = any("All reachability values are inf" in str(w.message) for w in caught)
        assert warned == bool(gold[name + "/warned"]), name
        _check_graph(est, gold, name, "cut %d" % i)
        _check_cut(est, gold, name, i, cut)
        assert est.n_features_in_ == case["N"]


def test_entry_points_by_name_over_the_min_samples_range(gold, dev):
    """ssg_optics_core_dist for min_samples from 2 to N on a tie-heavy float16 matrix, its float64 copy and a genuine float64 matrix
    (N = 257: a row is not a multiple of the 8-entry load, most rows start off a 16-byte boundary), with and without a max_eps;
    ssg_optics_order on those core distances in both placements against the numpy restatement"""
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr
    L = _lib.lib()
    assert L.ssg_optics_lds_max_n() >= 16384
    for name in ("n257_half", "n257_dup"):
        D = ref.matrix(ref.BY_NAME[name])
        X = np.asarray(D, np.float64)
        N = len(X)
        srt = np.sort(X, axis=1)
        mats = [(2, torch.from_numpy(X).to(dev))] + ([(1, torch.from_numpy(np.ascontiguousarray(D)).to(dev))] if D.dtype == np.float16 else [])
        for mode, M in mats:
            for k in (2, 3, 4, 9, 64, 65, 128, 256, 257):
                for max_eps in (np.inf, 0.45):
                    core = torch.full((N,), -1.0, dtype=torch.float64, device=dev)
                    check(L.ssg_optics_core_dist(ptr(M), None, N, mode, 0.0, k, max_eps, ptr(core), None), "ssg_optics_core_dist")
                    want = srt[:, k - 1].copy()
                    want[want > max_eps] = np.inf
                    assert _same_bits(core.cpu().numpy(), np.around(want, 15)), (name, mode, k, max_eps)
            k, max_eps = 9, 0.6
            wo, wc, wr, wp = ref.optics_graph(X, k, max_eps)
            core = torch.from_numpy(wc).to(dev)
            for state in (0, 1, 2):
                o = torch.full((N,), -7, dtype=torch.int64, device=dev)
                p = torch.full((N,), -7, dtype=torch.int64, device=dev)
                r = torch.full((N,), -7.0, dtype=torch.float64, device=dev)
                ws = torch.empty(N, dtype=torch.float64, device=dev)
                check(L.ssg_optics_order(ptr(M), None, N, mode, 0.0, ptr(core), max_eps, state, ptr(ws), N * 8, ptr(o), ptr(r), ptr(p), None), "ssg_optics_order")
                assert np.array_equal(o.cpu().numpy(), wo) and _same_bits(r.cpu().numpy(), wr) and np.array_equal(p.cpu().numpy(), wp), (name, mode, state)
            assert np.isinf(wr).sum() >= 2 and np.isinf(wc).any()            # the ordering restarted; some points are never core
    # refused before any launch, also on a machine that has a device
    assert L.ssg_optics_order(ptr(M), None, N, 2, 0.0, ptr(core), 1.0, 2, None, 0, ptr(o), ptr(r), ptr(p), None) == -1
    assert L.ssg_optics_core_dist(ptr(M), None, N, 2, 0.0, N + 1, 1.0, ptr(core), None) == -1


def test_state_beyond_64_kb_of_lds(dev):
    """N = 8 200: the loop's state (65 600 bytes) needs more LDS than a kernel gets without asking.  Both placements give the same bits,
    the ordering is a permutation, and every finite reachability is around15(max(X[pred, j], core[pred])) of its predecessor"""
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr
    L = _lib.lib()
    N = 8200
    assert 8 * N > 64 * 1024 and N <= L.ssg_optics_lds_max_n()
    g = torch.Generator(device=dev).manual_seed(4)
    pts = torch.rand((N, 3), device=dev, generator=g)
    M = torch.cdist(pts, pts).to(torch.float16)
    M = torch.minimum(M, M.T).contiguous()
    core = torch.empty(N, dtype=torch.float64, device=dev)
    check(L.ssg_optics_core_dist(ptr(M), None, N, 1, 0.0, 4, 0.05, ptr(core), None), "ssg_optics_core_dist")
    res = []
    for state in (1, 2):
        o = torch.full((N,), -7, dtype=torch.int64, device=dev)
        p = torch.full((N,), -7, dtype=torch.int64, device=dev)
        r = torch.full((N,), -7.0, dtype=torch.float64, device=dev)
        ws = torch.empty(N, dtype=torch.float64, device=dev)
        check(L.ssg_optics_order(ptr(M), None, N, 1, 0.0, ptr(core), 0.05, state, ptr(ws), N * 8, ptr(o), ptr(r), ptr(p), None), "ssg_optics_order")
        res.append((o, r, p))
    (o, r, p), (o2, r2, p2) = res
    assert torch.equal(o, o2) and torch.equal(p, p2) and torch.equal(r.view(torch.int64), r2.view(torch.int64))
    assert torch.equal(torch.sort(o).values, torch.arange(N, device=dev))
    fin = torch.isfinite(r)
    assert torch.equal(fin, p >= 0) and 100 < int(fin.sum()) < N and int(torch.isinf(core).sum()) > 0
    j = torch.nonzero(fin).flatten()
    d = M[p[j], j].to(torch.float64)
    scaled = torch.round(torch.maximum(d, core[p[j]]) * 1e15)
    want = scaled / torch.full_like(scaled, 1e15)              # (a tensor divisor: torch multiplies by the reciprocal of a scalar one)
    assert torch.equal(r[j].view(torch.int64), want.view(torch.int64)) and bool((d <= 0.05).all())
    pos = torch.empty(N, dtype=torch.int64, device=dev)
    pos[o] = torch.arange(N, device=dev)
    assert bool((pos[p[j]] < pos[j]).all())                   # a predecessor is processed before its point


@pytest.mark.parametrize("name", ["n64_half", "n257_half", "n513_half2"])
def test_half_and_float32_matrices_give_the_float64_copy_s_result(gold, dev, name):
    """sklearn widens a float16 / float32 matrix to float64 before anything else (unlike DBSCAN, which compares a float32 matrix in
    float32): numpy and torch, host and device, float16 (mode 1), float32 and float64 all give the golden of the float64 copy"""
    case = ref.BY_NAME[name]
    D = ref.matrix(case)
    assert D.dtype == np.float16
    cut = case["cuts"][0]
    inputs = {"numpy f32": D.astype(np.float32), "numpy f64": D.astype(np.float64), "torch f16 cuda": torch.from_numpy(np.ascontiguousarray(D)).to(dev),
              "torch f32 cpu": torch.from_numpy(D.astype(np.float32)), "torch f64 cuda": torch.from_numpy(D.astype(np.float64)).to(dev)}
    for what, X in inputs.items():
        est = _estimator(case, cut).fit(X)
        _check_graph(est, gold, name, what)
        _check_cut(est, gold, name, 0, cut, what)


def test_rerank_handle_is_read_in_place(gold, golden, dev, monkeypatch):
    """a mode-0 handle (J' half + source vector, built by re_ranking_device on the inputs of an existing re-rank golden) gives the golden
    of its float64 final_dist(); so does the DeviceBackedArray re_ranking returns; a second fit gives identical bits; a fit reads once"""
    from ssg_amd import optics, rerank, re_ranking
    case = ref.BY_NAME["rerank_n256"]
    g = golden(case["file"])
    src, tgt = torch.from_numpy(g["src"]).to(dev), torch.from_numpy(g["tgt"]).to(dev)
    h = rerank.re_ranking_device(src, tgt, k1=int(g["k1"]), k2=int(g["k2"]), lambda_value=case["lambda_value"])
    assert h.mode == 0 and h.group is None
    assert np.array_equal(h.final_dist().cpu().numpy(), np.asarray(ref.matrix(case)))
    reads = []
    real = optics._read_back
    monkeypatch.setattr(optics, "_read_back", lambda *t: reads.append(len(t)) or real(*t))
    for state in (1, 2):
        for i, cut in enumerate(case["cuts"]):
            est = _estimator(case, cut, state).fit(h)
            _check_graph(est, gold, case["name"], "state %d" % state)
            _check_cut(est, gold, case["name"], i, cut)
    assert len(reads) == 2 * len(case["cuts"])               # one blocking read per fit, all four arrays in it
    first = {a: getattr(est, a).copy() for a in ("ordering_", "core_distances_", "reachability_", "predecessor_", "labels_")}
    est.fit(h)
    for a, v in first.items():
        assert _same_bits(getattr(est, a), v), a
    # a fresh handle with its status words still pending (validate=False): fit validates it first, as DBSCAN.fit does
    h2 = rerank.re_ranking_device(src, tgt, k1=int(g["k1"]), k2=int(g["k2"]), lambda_value=case["lambda_value"], validate=False)
    est2 = _estimator(case, case["cuts"][0]).fit(h2)
    _check_graph(est2, gold, case["name"], "pending handle")
    # the array re_ranking returns carries its handle
    _, f = re_ranking(g["src"], g["tgt"], k1=int(g["k1"]), k2=int(g["k2"]), lambda_value=case["lambda_value"])
    est3 = _estimator(case, case["cuts"][0])
    assert np.array_equal(est3.fit_predict(f), gold["rerank_n256/cut0/labels"])
    _check_graph(est3, gold, case["name"], "DeviceBackedArray")


def test_generate_selflabel_optics(gold, golden, dev, capsys):
    """the grouping step with OPTICS: estimator cached at iteration 0, xi labels with no eps, the eps cut at the rho rule's eps"""
    from types import SimpleNamespace
    from ssg_amd import generate_selflabel_optics, rerank
    case = ref.BY_NAME["rerank_n256"]
    g = golden(case["file"])
    X = np.asarray(ref.matrix(case))
    h = rerank.re_ranking_device(torch.from_numpy(g["src"]).to(dev), torch.from_numpy(g["tgt"]).to(dev), k1=int(g["k1"]), k2=int(g["k2"]),
                                 lambda_value=case["lambda_value"])
    o, c, r, p = (gold["rerank_n256/" + k] for k in FIELDS)          # min_samples = 4, max_eps = inf: the defaults of the grouping step
    args = SimpleNamespace(no_rerank=False, rho=float(g["rho"]), optics_xi=0.01)
    labels, cl = generate_selflabel_optics([[]], [h], 0, args, cluster_list=[])
    want = gold["rerank_n256/cut0/labels"]
    assert len(cl) == 1 and np.array_equal(labels[0], want)
    out = capsys.readouterr().out
    assert "Clustering and labeling..." in out and "Iteration 1 have %d training ids" % (want.max() + 1) in out and "eps in cluster" not in out
    labels2, cl2 = generate_selflabel_optics([[]], [h], 1, args, cluster_list=cl)
    assert cl2[0] is cl[0] and np.array_equal(labels2[0], want) and "Iteration 2 have" in capsys.readouterr().out
    args = SimpleNamespace(no_rerank=False, rho=float(g["rho"]), optics_method="dbscan")
    labels3, cl3 = generate_selflabel_optics([[]], [h], 0, args, cluster_list=[])
    assert cl3[0].eps == float(g["eps"]) and cl3[0].cluster_method == "dbscan"
    assert np.array_equal(labels3[0], ref.cut_dbscan(r, c, o, float(g["eps"])))
    assert "eps in cluster: {:.3f}".format(float(g["eps"])) in capsys.readouterr().out
    assert X.shape == (256, 256)
