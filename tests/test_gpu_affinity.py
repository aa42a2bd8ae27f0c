"""GPU suite of ssg_amd.cluster.AffinityPropagation (csrc/affinity.hip) against sklearn 1.7.2's recorded results
(tests/golden/affinity_cases.npz, written by tools/make_affinity_golden.py) and the numpy restatement tests/affinity_ref.py.

Everything is compared bit for bit: exemplars, labels and n_iter_ with sklearn's; S after the prepare step, A and R after iterations 1
and 2 and the final A and R with the restatement's arrays (and their sha256 with the recorded ones)."""
import math
import os
import sys
import warnings
from functools import lru_cache

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affinity_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "affinity_cases.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    bad = int((g != w).sum())
    assert bad == 0, "%s: %d of %d entries differ in their bits" % (what, bad, g.size)


def _fit(name, dev, stages=None, **over):
    from ssg_amd.cluster import AffinityPropagation
    kw = ref.case_kwargs(name)
    kw.update(over)
    est = AffinityPropagation(affinity="precomputed", **kw)
    X = torch.from_numpy(np.array(ref.case_input(ref.CASES[name][0]))).to(dev)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        est.fit(X, stages=stages)
    return est, [str(x.message) for x in w], [x.category for x in w]


def _check_against_golden(name, est):
    g = _golden()
    assert est.n_iter_ == int(g[name + "_n_iter"]), (est.n_iter_, int(g[name + "_n_iter"]))
    assert np.array_equal(np.asarray(est.cluster_centers_indices_, dtype=np.int64), g[name + "_centers"])
    assert np.array_equal(est.labels_, g[name + "_labels"])
    assert est.labels_.dtype == np.int64
    if ref.EXPECTED.get(name) is not None:
        assert (est.n_iter_, len(est.cluster_centers_indices_)) == ref.EXPECTED[name]


@pytest.mark.parametrize("name", list(ref.CASES))
def test_cases_bit_for_bit(dev, name):
    from ssg_amd.cluster import ConvergenceWarning
    stages = {"after": (1, 2)}
    est, msgs, cats = _fit(name, dev, stages=stages)
    r = ref.case_result(name)
    g = _golden()
    _same_bits(stages["S"], r["S"], "S after prepare")
    _same_bits(est.affinity_matrix_, r["S"], "affinity_matrix_")
    assert est.affinity_matrix_.is_cuda
    for cnt in (1, 2):
        if cnt in r["snaps"]:
            _same_bits(stages["A"][cnt], r["snaps"][cnt][0], "A after iteration %d" % cnt)
            _same_bits(stages["R"][cnt], r["snaps"][cnt][1], "R after iteration %d" % cnt)
    _same_bits(stages["A_final"], r["A"], "final A")
    _same_bits(stages["R_final"], r["R"], "final R")
    sha = [ref.sha(stages["A_final"].cpu().numpy()), ref.sha(stages["R_final"].cpu().numpy()), ref.sha(stages["S"].cpu().numpy())]
    assert sha == list(g[name + "_sha"])
    _check_against_golden(name, est)
    assert est.n_features_in_ == r["S"].shape[0]
    K = len(est.cluster_centers_indices_)
    if K == 0:
        assert est.cluster_centers_indices_ == [] and (est.labels_ == -1).all()
        assert msgs == ["Affinity propagation did not converge and this model will not have any cluster centers."]
        assert cats == [ConvergenceWarning]
    elif not r["converged"]:
        assert msgs == ["Affinity propagation did not converge, this model may return degenerate cluster centers and labels."]
        assert cats == [ConvergenceWarning]
    else:
        assert msgs == []


@pytest.mark.parametrize("poll", [1, 7, 16, 64])
def test_poll_every_launches_past_convergence_are_noops(dev, poll):
    stages = {}
    est, _, _ = _fit("a", dev, stages=stages, poll_every=poll)
    r = ref.case_result("a")
    assert est.n_iter_ == 22
    _same_bits(stages["A_final"], r["A"], "final A, poll_every=%d" % poll)
    _same_bits(stages["R_final"], r["R"], "final R, poll_every=%d" % poll)
    _check_against_golden("a", est)


@pytest.mark.parametrize("name", ["a", "b"])       # N*N odd / even
def test_default_preference_is_numpy_median(dev, name):
    stages = {}
    _fit(name, dev, stages=stages, max_iter=1)
    want = np.median(ref.case_input(ref.CASES[name][0]))
    _same_bits(stages["preference"], np.array([want]), "median")


def test_median_abi_mixed_signs_and_ties(dev):
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 4096, 100003):
        x = np.round(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n), 2)      # both signs, zeros, many ties
        X = torch.from_numpy(x).to(dev)
        out = torch.zeros(1, dtype=torch.float64, device=dev)
        wb = int(L.ssg_ap_median_workspace_bytes())
        ws = torch.empty(wb // 8, dtype=torch.int64, device=dev)
        check(L.ssg_ap_median_f64(ptr(X), n, ptr(ws), wb, ptr(out), stream()), "ssg_ap_median_f64")
        assert float(out.item()) == float(np.median(x)), n


def test_column_walk_order(dev):
    """cs = the rows added in ascending order, one running sum per column, on magnitudes spread over 16 decades"""
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    rng = np.random.default_rng(0)
    ctrl = torch.zeros(8, dtype=torch.int64, device=dev)
    for n in (1, 63, 130, 700):
        R = rng.standard_normal((n, n)) * 10.0 ** rng.integers(-8, 8, (n, n))
        Rp = np.maximum(R, 0); Rp.flat[::n + 1] = R.flat[::n + 1]
        want = ref.colsum_seq(Rp)
        Rd = torch.from_numpy(R).to(dev)
        for cfg in [-1] + list(range(int(L.ssg_ap_colsum_configs()))):          # every tile of the walk: the same bits
            cs = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
            check(L.ssg_ap_colsum_cfg_f64(ptr(Rd), n, ptr(cs), ptr(ctrl), cfg, stream()), "ssg_ap_colsum_cfg_f64")
            _same_bits(cs, want, "column sums, N=%d, tile %d" % (n, cfg))
    # the two sides of the automatic choice of the tile (512 workgroups of 16 columns)
    for n in (8192, 8208):
        Rd = torch.randn((n, n), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(n))
        Rd *= 10.0 ** torch.randint(-8, 8, (n, n), device=dev, generator=torch.Generator(device=dev).manual_seed(n + 1)).to(torch.float64)
        cs = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
        check(L.ssg_ap_colsum_f64(ptr(Rd), n, ptr(cs), ptr(ctrl), stream()), "ssg_ap_colsum_f64")
        Rp = Rd.clamp(min=0)
        Rp.diagonal().copy_(Rd.diagonal())
        want = ref.colsum_seq(Rp.cpu().numpy())
        _same_bits(cs, want, "column sums, N=%d" % n)
    with pytest.raises(ValueError):
        check(L.ssg_ap_colsum_cfg_f64(ptr(Rd), 8, ptr(cs), ptr(ctrl), 99, stream()), "ssg_ap_colsum_cfg_f64")


def test_loop_through_the_c_abi(dev):
    """case (f) driven through the C ABI alone: prepare, the iterations in chunks of 5 queued blindly up to 40 (the stopping rule fires at
    27 on the device), the closing row call, finish -- against the restatement's S, A, R, exemplars and labels"""
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    r = ref.case_result("f")
    X = np.array(ref.case_input("f"))
    n = X.shape[0]
    S = torch.from_numpy(X).to(dev)
    pref = torch.tensor([-3.0], dtype=torch.float64, device=dev)
    noise = torch.from_numpy(np.random.RandomState(0).standard_normal(size=(n, n))).to(dev)
    check(L.ssg_ap_prepare_f64(ptr(S), n, ptr(pref), 1, ptr(noise), stream()), "ssg_ap_prepare_f64")
    _same_bits(S, r["S"], "S")
    A, R = torch.zeros((n, n), dtype=torch.float64, device=dev), torch.zeros((n, n), dtype=torch.float64, device=dev)
    cs, E = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    win, ctrl = torch.zeros((n, 15), dtype=torch.uint8, device=dev), torch.zeros(8, dtype=torch.int64, device=dev)
    for it0 in range(0, 40, 5):
        check(L.ssg_ap_iterate_f64(ptr(S), ptr(A), ptr(R), ptr(cs), ptr(win), ptr(E), ptr(ctrl), n, 0.5, 15, it0, 5, stream()), "ssg_ap_iterate_f64")
    check(L.ssg_ap_row_f64(ptr(S), ptr(A), ptr(R), ptr(cs), n, 0.5, 40, 0, ptr(ctrl), stream()), "ssg_ap_row_f64")
    assert ctrl[:2].tolist() == [1, r["n_iter"]] and r["n_iter"] == 27
    _same_bits(A, r["A"], "final A")
    _same_bits(R, r["R"], "final R")
    fin = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    sums = torch.empty(n, dtype=torch.float64, device=dev)
    check(L.ssg_ap_finish_f64(ptr(S), ptr(E), n, ptr(fin[:n]), ptr(fin[n:]), ptr(sums), ptr(ctrl), stream()), "ssg_ap_finish_f64")
    K = int(ctrl[2].item())
    f = fin.cpu().numpy().astype(np.int64)
    labels = f[:K][f[n:]]
    cen = np.unique(labels)
    assert np.array_equal(cen, r["centers"]) and np.array_equal(np.searchsorted(cen, labels), r["labels"])
    # refused before any launch
    for call in (lambda: L.ssg_ap_iterate_f64(ptr(S), ptr(A), ptr(R), ptr(cs), ptr(win), ptr(E), ptr(ctrl), n, 0.4, 15, 0, 1, stream()),
                 lambda: L.ssg_ap_iterate_f64(ptr(S), ptr(A), ptr(R), ptr(cs), ptr(win), ptr(E), ptr(ctrl), n, 0.5, 0, 0, 1, stream()),
                 lambda: L.ssg_ap_row_f64(ptr(S), ptr(A), None, ptr(cs), n, 0.5, 1, 1, ptr(ctrl), stream()),
                 lambda: L.ssg_ap_prepare_f64(ptr(S), n, ptr(pref), 2, ptr(noise), stream()),
                 lambda: L.ssg_ap_finish_f64(ptr(S), ptr(E), 0, ptr(fin), ptr(fin), ptr(sums), ptr(ctrl), stream())):
        assert call() == -1
    _same_bits(A, r["A"], "A after the refused calls")


def test_indices_past_2_31(dev):
    """N = 46 342: N * N exceeds 2^31, so an element index kept in 32 bits would wrap.  One 17 GB matrix; the column walk is checked on
    64 columns spread over the width (the last ones included) against numpy's sequential accumulate, the input scan on a NaN planted in
    the last row and on the extrema of the off-diagonal entries."""
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    n = 46342
    assert n * n > 2 ** 31
    R = torch.randn((n, n), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    cs = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    ctrl = torch.zeros(8, dtype=torch.int64, device=dev)
    check(L.ssg_ap_colsum_f64(ptr(R), n, ptr(cs), ptr(ctrl), stream()), "ssg_ap_colsum_f64")
    cols = np.unique(np.concatenate([np.arange(8), np.arange(n - 8, n), np.linspace(0, n - 1, 48).astype(np.int64)]))
    sub = R[:, torch.from_numpy(cols).to(dev)].cpu().numpy()
    rp = np.maximum(sub, 0)
    rp[cols, np.arange(cols.size)] = sub[cols, np.arange(cols.size)]
    want = np.add.accumulate(rp, axis=0)[-1]                      # one running sum per column, rows in ascending order
    _same_bits(cs.cpu().numpy()[cols], want, "column sums at N=%d" % n)
    pref = torch.tensor([-1.0], dtype=torch.float64, device=dev)
    stats = torch.zeros(8, dtype=torch.int64, device=dev)
    R.fill_diagonal_(1e9)                                         # the diagonal is outside the extrema
    R[n - 1, n - 2] = float("nan")
    R[n - 1, 0], R[n - 2, n - 1] = -77.0, 99.0
    check(L.ssg_ap_stats_f64(ptr(R), n, ptr(pref), 1, ptr(stats), stream()), "ssg_ap_stats_f64")
    from ssg_amd.cluster import _unkey
    st = stats.cpu().numpy()
    assert int(st[0]) == 1 and (_unkey(st[1]), _unkey(st[2])) == (-77.0, 99.0)
    assert float(st[6:7].view(np.float64)[0]) == float(R[0, n - 1].item())


def _small(dev, X, **kw):
    from ssg_amd.cluster import AffinityPropagation
    est = AffinityPropagation(affinity="precomputed", random_state=0, **kw)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        est.fit(torch.from_numpy(np.asarray(X, dtype=np.float64)).to(dev))
    return est, [str(x.message) for x in w]


def test_special_cases(dev):
    equal_msg = "All samples have mutually equal similarities. Returning arbitrary cluster center(s)."
    # N = 1
    est, msgs = _small(dev, [[-1.0]])
    assert msgs == [equal_msg] and est.n_iter_ == 0
    assert np.array_equal(est.cluster_centers_indices_, [0]) and np.array_equal(est.labels_, [0])
    # all equal: preference below the similarities -> one cluster; above -> every sample its own
    X = np.full((5, 5), -2.0)
    est, msgs = _small(dev, X, preference=-3.0)
    assert msgs == [equal_msg] and est.n_iter_ == 0
    assert np.array_equal(est.cluster_centers_indices_, [0]) and np.array_equal(est.labels_, [0] * 5)
    est, msgs = _small(dev, X, preference=-1.0)
    assert msgs == [equal_msg] and est.n_iter_ == 0
    assert np.array_equal(est.cluster_centers_indices_, np.arange(5)) and np.array_equal(est.labels_, np.arange(5))
    # N = 2 runs the loop: the restatement's answer
    X2 = np.array([[0.0, -1.0], [-1.5, 0.0]])
    est, msgs = _small(dev, X2, preference=-0.5)
    r = ref.affinity_propagation(X2, preference=-0.5, seed=0)
    assert est.n_iter_ == r["n_iter"]
    assert np.array_equal(np.asarray(est.cluster_centers_indices_, dtype=np.int64), r["centers"]) and np.array_equal(est.labels_, r["labels"])


def test_nan_and_inf_raise(dev):
    from ssg_amd.cluster import AffinityPropagation
    for bad in (np.nan, np.inf):
        X = np.array(ref.case_input("f"))
        X[7, 7] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            AffinityPropagation(affinity="precomputed", random_state=0).fit(torch.from_numpy(X).to(dev))


def test_copy_flag_and_refit(dev):
    from ssg_amd.cluster import AffinityPropagation
    X0 = np.array(ref.case_input("f"))
    X = torch.from_numpy(X0).to(dev)
    est = AffinityPropagation(affinity="precomputed", preference=-3.0, random_state=0)            # copy=True
    st1 = {}
    est.fit(X, stages=st1)
    assert np.array_equal(_bits(X), _bits(X0))
    assert est.affinity_matrix_.data_ptr() != X.data_ptr()
    first = (est.n_iter_, est.cluster_centers_indices_.copy(), est.labels_.copy(), _bits(st1["A_final"]), _bits(st1["R_final"]))
    # a second fit on the same estimator: identical bits (the cached noise is sklearn's reseeded matrix)
    st2 = {}
    est.fit(X, stages=st2)
    assert est.n_iter_ == first[0] and np.array_equal(est.cluster_centers_indices_, first[1]) and np.array_equal(est.labels_, first[2])
    assert np.array_equal(_bits(st2["A_final"]), first[3]) and np.array_equal(_bits(st2["R_final"]), first[4])
    _check_against_golden("f", est)
    # copy=False works on the caller's tensor
    est2 = AffinityPropagation(affinity="precomputed", preference=-3.0, random_state=0, copy=False).fit(X)
    assert est2.affinity_matrix_.data_ptr() == X.data_ptr()
    _same_bits(X, ref.case_result("f")["S"], "the caller's tensor after copy=False")
    _check_against_golden("f", est2)
    # float32 input is widened first
    est3 = AffinityPropagation(affinity="precomputed", preference=-3.0, random_state=0).fit(torch.from_numpy(X0.astype(np.float32)).to(dev))
    r3 = ref.affinity_propagation(X0.astype(np.float32).astype(np.float64), preference=-3.0, seed=0)
    assert est3.n_iter_ == r3["n_iter"] and np.array_equal(est3.labels_, r3["labels"])


@pytest.mark.parametrize("poll", [1, 7, 16])
def test_blocking_reads(dev, poll, monkeypatch):
    from ssg_amd import cluster
    calls = []
    real = cluster._read_back
    monkeypatch.setattr(cluster, "_read_back", lambda *t: (calls.append(len(t)), real(*t))[1])
    est, _, _ = _fit("a", dev, poll_every=poll)
    assert est.n_iter_ == 22
    assert len(calls) <= math.ceil(est.n_iter_ / poll) + 2, (len(calls), poll)


def test_generate_selflabel_affinity(dev, capsys, ora):
    import types
    from ssg_amd import rerank, selftraining
    from ssg_amd.cluster import AffinityPropagation
    rng = np.random.default_rng(0)
    N, Ns, d, P = 512, 256, 128, 32
    c = rng.standard_normal((P, d)); c /= np.linalg.norm(c, axis=1, keepdims=True)
    tgt = c[np.arange(N) % P] + 0.044 * rng.standard_normal((N, d)); tgt /= np.linalg.norm(tgt, axis=1, keepdims=True)
    src = rng.standard_normal((Ns, d)); src /= np.linalg.norm(src, axis=1, keepdims=True)
    tgt = tgt.astype(np.float32); src = (0.6 * src + 0.4 * tgt[:Ns]).astype(np.float32)
    h = rerank.re_ranking_device(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), lambda_value=0.1)
    args = types.SimpleNamespace(no_rerank=False, rho=1.6e-3)
    want = AffinityPropagation(affinity="precomputed", random_state=0).fit_predict(-h.final_dist())
    cl = []
    labels, cl = selftraining.generate_selflabel_affinity([[]], [h], 0, args, cl)
    assert len(cl) == 1 and isinstance(cl[0], AffinityPropagation)
    assert np.array_equal(labels[0], want)
    first = cl[0]
    labels2, cl2 = selftraining.generate_selflabel_affinity([[]], [h], 1, args, cl)
    assert cl2[0] is first and len(cl2) == 1 and np.array_equal(labels2[0], want)
    out = capsys.readouterr().out
    assert "eps in cluster" not in out
    assert "Iteration 1 have %d training ids" % len(set(want.tolist())) in out and "Iteration 2 have" in out
    # the DBSCAN path on the same handle is untouched
    of = h.final_dist().cpu().numpy()
    oeps, _, _ = ora.eps_rule(of, 1.6e-3)
    lab_db, _ = selftraining.generate_selflabel([[]], [h], 0, args, [])
    assert np.array_equal(lab_db[0], ora.dbscan(of, oeps, 4))
    # the class takes no distance handle
    with pytest.raises(TypeError, match="final_dist"):
        AffinityPropagation(affinity="precomputed").fit(h)
