"""CPU half of the OPTICS tests.  The golden (tests/golden/optics_cases.npz) holds what sklearn 1.7.2 `OPTICS(metric='precomputed')` gave
for every case of tests/optics_ref.py; here, without a GPU: the rebuilt matrices are the ones the golden was made from (sha256), the
numpy restatement of the graph reproduces the golden bit for bit, the package's two label extractions (ssg_amd/optics.py, numpy on
four N-long arrays) reproduce the golden labels and hierarchies, the golden is not vacuous, the estimator's parameter errors and its
warning, the refusals of the entry points before any device call, and the scalar rules of csrc/optics.hip -- around15, the core-distance
finish, the reachability update, the arg-min tie rule, the radix key -- compiled for x86 from the SAME SOURCE TEXT
(tools/hostexec/optics_rules.cpp) and held to numpy.
"""
import ctypes
import os
import subprocess
import warnings

import numpy as np
import pytest

import optics_ref as ref
from ssg_amd import _lib, cluster, optics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
NAMES = [c["name"] for c in ref.CASES]


@pytest.fixture(scope="module")
def gold():
    return ref.load_golden()


def _graph(gold, name):
    return tuple(gold["%s/%s" % (name, k)] for k in ("ordering", "core", "reach", "pred"))


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ the golden and the restatement
@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_sklearn_bit_for_bit(gold, name):
    case = ref.BY_NAME[name]
    D = ref.matrix(case)
    assert ref.sha(D) == str(gold[name + "/sha256"]), "the matrix generator drifted: the golden was made from another matrix"
    got = ref.optics_graph(D, case["min_samples"], case["max_eps"])
    for g, w, what in zip(got, _graph(gold, name), ("ordering", "core_distances", "reachability", "predecessor")):
        assert _same_bits(g.astype(w.dtype), w), (name, what)
    assert sorted(got[0].tolist()) == list(range(case["N"]))


@pytest.mark.parametrize("name", NAMES)
def test_label_extractions_reproduce_the_golden(gold, name):
    """the package's cluster_optics_dbscan / cluster_optics_xi and the restatement's loops, fed the golden arrays"""
    case = ref.BY_NAME[name]
    o, c, r, p = _graph(gold, name)
    for i, cut in enumerate(case["cuts"]):
        want = gold["%s/cut%d/labels" % (name, i)]
        rl, rh = ref.run_cut(cut, o, c, r, p, case["min_samples"], case["max_eps"])
        if cut["method"] == "xi":
            labels, hier = optics.cluster_optics_xi(reachability=r, predecessor=p, ordering=o, min_samples=case["min_samples"],
                                                    min_cluster_size=cut["min_cluster_size"], xi=cut["xi"],
                                                    predecessor_correction=cut["predecessor_correction"])
            wh = gold["%s/cut%d/hier" % (name, i)]
            assert np.array_equal(hier, wh) and hier.shape == wh.shape, (name, i)
            assert np.array_equal(rh, wh) and rh.shape == wh.shape, (name, i)
        else:
            labels = optics.cluster_optics_dbscan(reachability=r, core_distances=c, ordering=o, eps=cut["eps"])
        assert np.array_equal(labels, want) and labels.shape == want.shape, (name, i)
        assert np.array_equal(rl, want), (name, i)


def test_golden_is_not_vacuous(gold):
    assert str(gold["sklearn_version"]) == "1.7.2"
    changed, restarts = 0, 0
    for case in ref.CASES:
        name = case["name"]
        o, c, r, p = _graph(gold, name)
        X = np.asarray(ref.matrix(case), np.float64)
        kth = np.sort(X, axis=1)[:, ref.resolve_size(case["min_samples"], case["N"]) - 1]
        if case["kind"] != "half" and np.any((kth != c) & np.isfinite(c)):
            changed += 1                                                   # around15 moved a float64 core distance
        if np.isinf(r).sum() >= 2 and not np.isinf(r).all():
            restarts += 1                                                  # the ordering restarted at the smallest unprocessed index
        if case["full"]:
            for i in range(len(case["cuts"])):
                lab = gold["%s/cut%d/labels" % (name, i)]
                assert lab.max() + 1 >= 2 and (lab < 0).any(), (name, i)
    assert changed >= 2 and restarts >= 1
    assert bool(gold["n64_tiny/warned"]) and np.isinf(gold["n64_tiny/reach"]).all() and (gold["n64_tiny/cut0/labels"] == -1).all()
    assert sum(bool(gold[n + "/warned"]) for n in NAMES) == 1
    # what the case table promises
    assert sorted({c["N"] for c in ref.CASES if c["kind"] != "rerank"}) == [2, 7, 64, 65, 257, 513, 3001]
    assert {2, 4, 9, 0.05} <= {c["min_samples"] for c in ref.CASES} and any(c["min_samples"] == c["N"] for c in ref.CASES)
    assert {c["kind"] for c in ref.CASES} == {"half", "dup", "f64", "rerank"}
    dup = np.asarray(ref.matrix(ref.BY_NAME["n257_dup"]))
    assert (dup[~np.eye(257, dtype=bool)] == 0).sum() > 0                  # duplicated points: zeros off the diagonal
    half = ref.matrix(ref.BY_NAME["n257_half"])
    assert half.dtype == np.float16 and (np.diag(half) != 0).all() and np.unique(half).size < half.size // 8      # tie-heavy, a non-zero diagonal
    cuts = [cut for c in ref.CASES for cut in c["cuts"] if cut["method"] == "xi"]
    assert {0.01, 0.05, 0.3} <= {cut["xi"] for cut in cuts} and {True, False} == {cut["predecessor_correction"] for cut in cuts}
    kinds = {type(cut["min_cluster_size"]) for cut in cuts}
    assert kinds == {type(None), int, float}


# ------------------------------------------------------------------ the estimator without a device
def test_surface():
    import ssg_amd
    from ssg_amd import selftraining
    for name in ("OPTICS", "compute_optics_graph", "cluster_optics_dbscan", "cluster_optics_xi"):
        assert getattr(cluster, name) is getattr(optics, name) is getattr(ssg_amd, name)
    assert callable(selftraining.generate_selflabel_optics) and ssg_amd.generate_selflabel_optics is selftraining.generate_selflabel_optics
    est = optics.OPTICS()
    assert (est.min_samples, est.max_eps, est.metric, est.p, est.cluster_method, est.eps, est.xi) == (5, np.inf, "minkowski", 2, "xi", None, 0.05)
    assert (est.predecessor_correction, est.min_cluster_size, est.algorithm, est.leaf_size, est.memory, est.n_jobs) == (True, None, "auto", 30, None, None)
    with pytest.raises(TypeError):
        optics.OPTICS(5)                                    # keyword-only, like sklearn
    import sys
    src = open(optics.__file__).read()
    assert "import sklearn" not in src and "from sklearn" not in src
    protos = _lib.parse_header()
    for name in ("ssg_optics_core_dist", "ssg_optics_order", "ssg_optics_lds_max_n"):
        assert name in protos, name
    assert sys.modules.get("ssg_amd.optics") is optics


def test_parameter_errors_come_before_any_device_call():
    X = np.zeros((4, 4))
    ok = dict(metric="precomputed")
    for bad in (dict(min_samples=1), dict(min_samples=0), dict(min_samples=1.5), dict(min_samples=-0.1), dict(min_samples="4"), dict(min_samples=True),
                dict(max_eps=-1.0), dict(max_eps=float("nan")), dict(max_eps="x"), dict(cluster_method="kmeans"), dict(eps=-0.5), dict(eps="x"),
                dict(xi=1.5), dict(xi=-0.1), dict(xi=None), dict(predecessor_correction=1), dict(min_cluster_size=1), dict(min_cluster_size=0.0),
                dict(min_cluster_size=1.5)):
        with pytest.raises(ValueError, match="parameter of OPTICS must be"):
            optics.OPTICS(**ok, **bad).fit(X)
    for metric in ("minkowski", "euclidean", "cosine"):
        with pytest.raises(ValueError, match="metric='precomputed' only"):
            optics.OPTICS(metric=metric).fit(X)
    with pytest.raises(ValueError, match=r"min_samples must be no greater than the number of samples \(4\)\. Got 5"):
        optics.OPTICS(min_samples=5, **ok).fit(X)
    with pytest.raises(ValueError, match=r"Specify an epsilon smaller than 0\.5\. Got 0\.7\."):
        optics.OPTICS(cluster_method="dbscan", eps=0.7, max_eps=0.5, **ok).fit(X)
    with pytest.raises(ValueError, match="state must be"):
        optics.compute_optics_graph(X, min_samples=2, max_eps=np.inf, state=3)
    # the module functions check their own arguments
    r, p, o = np.array([np.inf, 1.0, 1.0]), np.array([-1, 0, 0]), np.arange(3)
    with pytest.raises(ValueError, match="min_samples must be no greater"):
        optics.cluster_optics_xi(reachability=r, predecessor=p, ordering=o, min_samples=4)
    with pytest.raises(ValueError, match="min_cluster_size must be no greater"):
        optics.cluster_optics_xi(reachability=r, predecessor=p, ordering=o, min_samples=2, min_cluster_size=4)
    with pytest.raises(ValueError, match="'xi' parameter"):
        optics.cluster_optics_xi(reachability=r, predecessor=p, ordering=o, min_samples=2, xi=2.0)
    with pytest.raises(ValueError, match="'eps' parameter"):
        optics.cluster_optics_dbscan(reachability=r, core_distances=r, ordering=o, eps=-1.0)
    with pytest.raises(TypeError):
        optics.cluster_optics_dbscan(r, r, o, 0.5)          # keyword-only


class _FakeHandle:
    group, row0, mode, lambda_value = None, 0, 2, 0.0

    def __init__(self, n):
        self.N = self.nrows = n

    def validate(self):
        self.validated = True
        return self


def test_fit_plumbing_and_the_warning(gold, monkeypatch):
    """fit with the device part replaced by the golden arrays: the fraction and the state reach the device call, the handle is validated
    first, the labels and the hierarchy are the golden's, the all-inf warning is sklearn's, a sharded handle is refused"""
    seen = {}

    def fake_graph(name):
        def run(h, k, max_eps, state):
            seen.update(k=k, max_eps=max_eps, state=state, validated=getattr(h, "validated", False))
            return _graph(gold, name)
        return run

    case = ref.BY_NAME["n257_dup"]
    h = _FakeHandle(257)
    monkeypatch.setattr(cluster, "as_handle", lambda X, device=None: h)
    monkeypatch.setattr(optics, "_device_graph", fake_graph("n257_dup"))
    est = optics.OPTICS(metric="precomputed", min_samples=case["min_samples"], max_eps=case["max_eps"])
    est.state = 2
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert est.fit_predict(np.zeros((257, 257))) is est.labels_
    assert seen == dict(k=12, max_eps=np.inf, state=2, validated=True)              # max(2, int(0.05 * 257))
    assert np.array_equal(est.labels_, gold["n257_dup/cut0/labels"]) and np.array_equal(est.cluster_hierarchy_, gold["n257_dup/cut0/hier"])
    assert est.n_features_in_ == 257 and _same_bits(est.reachability_, gold["n257_dup/reach"])
    est = optics.OPTICS(metric="precomputed", min_samples=case["min_samples"], cluster_method="dbscan", eps=0.35).fit(np.zeros((257, 257)))
    assert np.array_equal(est.labels_, gold["n257_dup/cut2/labels"]) and not hasattr(est, "cluster_hierarchy_")
    # every reachability infinite: sklearn's warning, all noise
    h = _FakeHandle(64)
    monkeypatch.setattr(optics, "_device_graph", fake_graph("n64_tiny"))
    with pytest.warns(UserWarning, match="All reachability values are inf. Set a larger max_eps or all data will be considered outliers."):
        est = optics.OPTICS(metric="precomputed", min_samples=4, max_eps=1e-3).fit(np.zeros((64, 64)))
    assert (est.labels_ == -1).all() and est.cluster_hierarchy_.shape == (0,)
    # one GPU only
    h.group = object()
    with pytest.raises(ValueError, match="single GPU"):
        optics.OPTICS(metric="precomputed", min_samples=4).fit(np.zeros((64, 64)))


# ------------------------------------------------------------------ the entry points' refusals
def test_entry_points_refuse_before_any_device_call():
    """everything outside the rules returns -1 and names the entry point in ssg_last_error -- no device is touched (this box has none)"""
    L = _lib.lib()
    P = ctypes.c_void_p
    a = P(4096)
    cap = L.ssg_optics_lds_max_n()
    assert 16384 <= cap and cap * 8 + 256 <= 160 * 1024
    inf = float("inf")

    def core(M=a, v=None, N=8, mode=2, k=2, max_eps=inf, out=a):
        return L.ssg_optics_core_dist(M, v, N, mode, 0.0, k, max_eps, out, None)

    def order(M=a, v=None, N=8, mode=2, core_=a, max_eps=inf, state=0, ws=a, ws_bytes=1 << 30, o=a, r=a, p=a):
        return L.ssg_optics_order(M, v, N, mode, 0.0, core_, max_eps, state, ws, ws_bytes, o, r, p, None)

    for what, call in (("null matrix", lambda: core(M=None)), ("N = 1", lambda: core(N=1)), ("N = 0", lambda: core(N=0)), ("mode 3", lambda: core(mode=3)),
                       ("mode 0 without v", lambda: core(mode=0)), ("min_samples = 1", lambda: core(k=1)), ("min_samples = N + 1", lambda: core(k=9)),
                       ("null output", lambda: core(out=None)), ("negative max_eps", lambda: core(max_eps=-1.0)), ("NaN max_eps", lambda: core(max_eps=float("nan")))):
        assert call() == -1, what
        assert b"ssg_optics_core_dist" in L.ssg_last_error(), what
    for what, call in (("null matrix", lambda: order(M=None)), ("N = 1", lambda: order(N=1)), ("mode -1", lambda: order(mode=-1)),
                       ("mode 0 without v", lambda: order(mode=0)), ("null core", lambda: order(core_=None)), ("null ordering", lambda: order(o=None)),
                       ("null reachability", lambda: order(r=None)), ("null predecessor", lambda: order(p=None)), ("negative max_eps", lambda: order(max_eps=-0.5)),
                       ("state 3", lambda: order(state=3)), ("state -1", lambda: order(state=-1)), ("LDS state beyond its capacity", lambda: order(N=cap + 1, state=1)),
                       ("global state without a workspace", lambda: order(state=2, ws=None)), ("global state, short workspace", lambda: order(state=2, ws_bytes=63)),
                       ("auto beyond LDS without a workspace", lambda: order(N=cap + 1, ws=None)), ("unaligned workspace", lambda: order(state=2, ws=P(4100)))):
        assert call() == -1, what
        assert b"ssg_optics_order" in L.ssg_last_error(), what
    with pytest.raises(ValueError, match="ssg_optics_order"):
        _lib.check(order(state=3), "ssg_optics_order")


# ------------------------------------------------------------------ the scalar rules of optics.hip, compiled for x86
@pytest.fixture(scope="module")
def hx(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang++ not present")
    d = tmp_path_factory.mktemp("hx_optics")
    out, on = [], False
    for line in open(os.path.join(ROOT, "self-similarity-grouping_amd", "csrc", "optics.hip")):
        if line.startswith("__device__ __forceinline__ double optics_around15"):
            on = True
        if "end of the scalar rules" in line:
            break
        if on:
            out.append(line)
    text = "".join(out)
    for name in ("optics_around15", "optics_core_finish", "optics_update", "optics_better", "optics_key", "optics_unkey"):
        assert "__device__ __forceinline__" in text and name + "(" in text, name
    (d / "optics_cut.inc").write_text(text)
    so = str(d / "libhx_optics.so")
    r = subprocess.run([CLANG, "-x", "hip", "--offload-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I/opt/rocm/include", "-I" + str(d), "-o", so,
                        os.path.join(ROOT, "tools", "hostexec", "optics_rules.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _value_table():
    rng = np.random.RandomState(3)
    big = 2.0 ** 53 / 1e15                                   # x * 1e15 >= 2^53 from here on: the division still changes the value
    vals = [0.0, 5e-324, 1e-320, 2.2250738585072014e-308, 1e-300, 4.9e-16, 0.5e-15, 1.5e-15, 2.5e-15, 1e-15, 0.1, 0.2, 0.1 + 0.2, 1 / 3, 0.7, 1.0,
            9.0, big, np.nextafter(big, 0), np.nextafter(big, np.inf), 9.1, 12.3456789, 123.456, 1e3 + 1e-13, 1e10 / 3, 1e100, 1e292, 1.7e293, np.inf]
    vals += list(rng.uniform(0, 1, 4000)) + list(rng.uniform(0, 40, 2000)) + list(np.exp(rng.uniform(np.log(1e-20), np.log(1e20), 4000)))
    vals += list(np.float16(rng.uniform(0, 4, 1000)).astype(np.float64))
    vals += list((np.arange(1, 400) + 0.5) * 1e-15) + list(rng.randint(1, 1 << 20, 400) * 1e-15 + 0.5e-15)      # halfway cases: ties go to the even digit
    return np.array(vals, dtype=np.float64)


def test_around15_is_numpy_around(hx):
    x = _value_table()
    got = np.empty_like(x)
    hx.hx_optics_around15(_p(x), ctypes.c_long(x.size), _p(got))
    with np.errstate(over="ignore"):
        want = np.around(x, 15)
    assert _same_bits(got, want)
    assert got[x == np.inf][0] == np.inf and got[0] == 0.0
    past = x[(x * 1e15 >= 2.0 ** 53) & np.isfinite(x * 1e15)]
    assert past.size > 100 and (np.around(past, 15) != past).any()          # the division is applied there too, and it shows
    assert (want[x < 1] != x[x < 1]).sum() > 1000                           # the table is not made of fixed points
    # the core-distance finish: > max_eps -> inf, then around15
    for max_eps in (np.inf, 0.45, 0.0):
        fin = np.empty_like(x)
        hx.hx_optics_core_finish(_p(x), ctypes.c_long(x.size), ctypes.c_double(max_eps), _p(fin))
        c = x.copy()
        c[c > max_eps] = np.inf
        with np.errstate(over="ignore"):
            assert _same_bits(fin, np.around(c, 15)), max_eps


def test_key_preserves_the_order(hx):
    x = np.concatenate([_value_table(), -_value_table()[1:200], [-0.0]])
    key = np.empty(x.size, np.uint64)
    back = np.empty_like(x)
    hx.hx_optics_key(_p(x), ctypes.c_long(x.size), _p(key), _p(back))
    assert _same_bits(back, x)
    order = np.argsort(key, kind="stable")
    assert (np.diff(x[order]) >= 0).all()
    assert np.unique(key).size == np.unique(x.view(np.uint64)).size        # one key per bit pattern (-0.0 sorts just below +0.0)


def test_argmin_tie_rule(hx):
    rng = np.random.RandomState(5)
    hx.hx_optics_argmin.restype = ctypes.c_long
    for trial in range(200):
        n = int(rng.randint(1, 40))
        reach = rng.choice([0.25, 0.5, 0.5, 1.0, np.inf, np.inf], size=n)
        skip = (rng.uniform(size=n) < 0.4).astype(np.uint8)
        if trial % 5 == 0:
            reach[:] = np.inf                                # nothing reachable: the smallest unprocessed index
        idx = np.flatnonzero(skip == 0)
        want = int(idx[np.argmin(reach[idx])]) if idx.size else -1
        for desc in (0, 1):
            assert hx.hx_optics_argmin(_p(reach), _p(skip), ctypes.c_long(n), desc) == want, (trial, desc)


@pytest.mark.parametrize("name", ["n65_f64", "n257_half", "n257_dup", "n64_tiny"])
def test_compiled_rules_walk_the_golden_ordering(hx, gold, name):
    """the loop of optics.hip with its compiled rules (core finish, update, arg-min) and the data movement in numpy gives the golden"""
    case = ref.BY_NAME[name]
    X = np.ascontiguousarray(ref.matrix(case), dtype=np.float64)
    n, max_eps = case["N"], case["max_eps"]
    k = ref.resolve_size(case["min_samples"], n)
    kth = np.ascontiguousarray(np.sort(X, axis=1)[:, k - 1])
    core = np.empty(n)
    hx.hx_optics_core_finish(_p(kth), ctypes.c_long(n), ctypes.c_double(max_eps), _p(core))
    reach, pred, done = np.full(n, np.inf), np.full(n, -1, np.int64), np.zeros(n, np.uint8)
    ordering = np.empty(n, np.int64)
    hx.hx_optics_argmin.restype = ctypes.c_long
    for t in range(n):
        p = hx.hx_optics_argmin(_p(reach), _p(done), ctypes.c_long(n), t & 1)
        ordering[t], done[p] = p, 1
        if core[p] != np.inf:
            hx.hx_optics_update_row(_p(X[p]), _p(done), ctypes.c_long(n), ctypes.c_double(core[p]), ctypes.c_double(max_eps), ctypes.c_long(p), _p(reach), _p(pred))
    for g, w, what in zip((ordering, core, reach, pred), _graph(gold, name), ("ordering", "core_distances", "reachability", "predecessor")):
        assert _same_bits(g, w.astype(g.dtype)), (name, what)


def test_update_rule_is_numpy_at_the_margin(hx):
    """the reachability update against numpy on pairs (candidate, reach[j]) that lie a few ulps or a few 1e-15 apart: the shortcut that
    skips the rounding for a candidate far above reach[j] must never change the decision or the value"""
    rng = np.random.RandomState(9)
    base = np.concatenate([rng.uniform(0, 2, 3000), np.float16(rng.uniform(0, 2, 1000)).astype(np.float64), np.exp(rng.uniform(np.log(1e-18), np.log(1e6), 2000)),
                           [0.0, 1e-15, 2e-15, 0.5e-15, 1.0, 9.5, 100.0]])
    ds, ss = [], []
    for steps in (0, 1, -1, 2, -2, 3, -5):
        moved = base.copy()
        for _ in range(abs(steps)):
            moved = np.nextafter(moved, np.inf if steps > 0 else -np.inf)
        ds.append(base); ss.append(np.maximum(moved, 0.0))
        ds.append(base); ss.append(np.maximum(np.around(base, 15) + steps * 1e-15, 0.0))
        ds.append(base); ss.append(np.maximum(np.around(base, 15) + steps * 0.25e-15, 0.0))
    ds.append(base); ss.append(np.full(base.size, np.inf))
    ds.append(base); ss.append(rng.uniform(0, 2, base.size))
    d, s = np.ascontiguousarray(np.concatenate(ds)), np.ascontiguousarray(np.concatenate(ss))
    skip = np.zeros(d.size, np.uint8)
    for cp, max_eps in ((0.0, np.inf), (0.3, np.inf), (1e-15, np.inf), (0.3, 0.9), (0.75, 0.5)):
        reach, pred = s.copy(), np.full(d.size, -1, np.int64)
        hx.hx_optics_update_row(_p(d), _p(skip), ctypes.c_long(d.size), ctypes.c_double(cp), ctypes.c_double(max_eps), ctypes.c_long(7), _p(reach), _p(pred))
        r = np.around(np.maximum(d, cp), 15)
        better = (d <= max_eps) & (r < s)
        assert _same_bits(reach, np.where(better, r, s)) and np.array_equal(pred, np.where(better, 7, -1)), (cp, max_eps)
        assert better.sum() > 1000 and (~better).sum() > 1000          # both outcomes are well represented
