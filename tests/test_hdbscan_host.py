"""CPU half of the HDBSCAN tests.  The golden (tests/golden/hdbscan_cases.npz) holds what sklearn 1.7.2 `HDBSCAN(metric='precomputed')`
gave for every case of tests/hdbscan_ref.py, with the order in which the machine that made it sorted the tied edges.  Here, without a
GPU: the rebuilt matrices are the ones the golden was made from (sha256); the restatement reproduces the golden bit for bit (core
distances and spanning tree from the matrix; tree, labels, probabilities and cut labels from the stored edge order); the product's host
stage (ssg_amd/hdbscan.py), fed the golden spanning tree and the golden edge order, gives the golden tree, labels and probabilities bit
for bit; the golden is not vacuous; every validation message and their order; the refusals of the entry points before any device call;
and the scalar rules of csrc/hdbscan.hip -- the three-way max, the min-update, the better-than order, the allclose predicate -- compiled
for x86 from the SAME SOURCE TEXT (tools/hostexec/hdbscan_rules.cpp) and held to numpy.
"""
import ctypes
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import hdbscan_ref as ref
from ssg_amd import _lib, cluster, hdbscan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in ref.CASES]
MST = ("mst_current", "mst_next", "mst_distance")
TREE = (("left_node", "slt_left"), ("right_node", "slt_right"), ("value", "slt_value"), ("cluster_size", "slt_size"))


@pytest.fixture(scope="module")
def gold():
    return ref.load_golden()


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _mst(gold, name):
    return tuple(gold["%s/%s" % (name, k)] for k in MST)


# ------------------------------------------------------------------ the golden and the restatement
@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_sklearn_bit_for_bit(gold, name):
    case = ref.BY_NAME[name]
    D = ref.matrix(case)
    assert ref.sha(D) == str(gold[name + "/sha256"]), "the matrix generator drifted: the golden was made from another matrix"
    ms, alpha = ref.min_samples_of(case), case["alpha"]
    core = ref.core_distances(D, ms, alpha)
    assert _same_bits(core, gold[name + "/core"]), name
    for g, key in zip(ref.prim(D, core, alpha), MST):
        assert _same_bits(g, gold["%s/%s" % (name, key)]), (name, key)
    # the edges form a path that visits every node once: the first field is the node the step started from
    cur, nxt, _ = _mst(gold, name)
    assert cur[0] == 0 and np.array_equal(cur[1:], nxt[:-1]) and sorted([0] + nxt.tolist()) == list(range(case["N"]))
    for key, val in ref.run_case(case, *_mst(gold, name), gold[name + "/row_order"]).items():
        assert _same_bits(val, gold["%s/%s" % (name, key)]), (name, key)


@pytest.mark.parametrize("name", NAMES)
def test_product_host_stage_reproduces_the_golden(gold, name):
    """ssg_amd.hdbscan's argsort-free host stage on the golden spanning tree and the golden edge order: the single-linkage tree, the
    labels, the probabilities and the cut labels of sklearn, bit for bit"""
    case = ref.BY_NAME[name]
    tree, labels, probs = hdbscan._tree_from_mst(*_mst(gold, name), case["min_cluster_size"], case["method"], case["allow_single_cluster"], case["epsilon"],
                                                 case["max_cluster_size"], row_order=gold[name + "/row_order"])
    assert tree.dtype == hdbscan.HIERARCHY_dtype and tree.shape == (case["N"] - 1,)
    for field, key in TREE:
        assert _same_bits(tree[field].astype(gold["%s/%s" % (name, key)].dtype), gold["%s/%s" % (name, key)]), (name, field)
    assert labels.dtype == np.int64 and _same_bits(labels, gold[name + "/labels"]), name
    assert probs.dtype == np.float64 and _same_bits(probs, gold[name + "/probs"]), name
    est = hdbscan.HDBSCAN(metric="precomputed")
    est._single_linkage_tree_ = tree
    for i, cut in enumerate(case["cuts"]):
        got = est.dbscan_clustering(cut, min_cluster_size=case["min_cluster_size"])
        assert got.dtype == np.int64 and np.array_equal(got, gold["%s/cut%d" % (name, i)]), (name, i)
    # the default order is np.argsort's, and it is a permutation that sorts the weights
    tree2, labels2, _ = hdbscan._tree_from_mst(*_mst(gold, name), case["min_cluster_size"], case["method"], case["allow_single_cluster"], case["epsilon"],
                                               case["max_cluster_size"])
    assert _same_bits(tree2["value"], tree["value"])
    if np.array_equal(np.argsort(gold[name + "/mst_distance"]), gold[name + "/row_order"]):
        assert _same_bits(labels2, labels) and tree2.tobytes() == tree.tobytes()


def test_golden_is_not_vacuous(gold):
    assert str(gold["sklearn_version"]) == "1.7.2"
    for case in ref.CASES:
        name = case["name"]
        lab = gold[name + "/labels"]
        if case["full"]:
            assert lab.max() + 1 >= 2 and (lab < 0).any(), name
        assert ((gold[name + "/probs"] > 0) == (lab >= 0)).all(), name
    assert [n for n in NAMES if bool(gold[n + "/warned"])] == ["n257_inf"] and np.isinf(gold["n257_inf/mst_distance"]).sum() >= 5
    D = np.asarray(ref.matrix(ref.BY_NAME["n257_inf"]), np.float64)
    assert np.isinf(D).sum() > 600 and np.array_equal(D, D.T) and np.isfinite(np.diag(D)).all()
    # what the case table promises
    assert {2, 7, 64, 65, 257, 513, 3001, 256} == {c["N"] for c in ref.CASES}
    assert {2, 4, 5, 10} <= {c["min_cluster_size"] for c in ref.CASES} and {None, 1, 3} <= {c["min_samples"] for c in ref.CASES}
    assert any(c["min_samples"] == c["N"] for c in ref.CASES) and {1.0, 1.5} == {c["alpha"] for c in ref.CASES}
    assert {"eom", "leaf"} == {c["method"] for c in ref.CASES} and any(c["allow_single_cluster"] for c in ref.CASES)
    assert any(c["epsilon"] > 0 for c in ref.CASES) and any(c["max_cluster_size"] == 20 for c in ref.CASES)
    assert all(len(c["cuts"]) == 2 for c in ref.CASES)
    # the parameters bite: epsilon merges clusters, the size limit splits them, a single cluster is allowed
    assert gold["n257_half_eps/labels"].max() < gold["n257_half/labels"].max()
    assert not np.array_equal(gold["n513_f64_max12/labels"], gold["n513_f64_max/labels"])
    assert gold["rerank_n256_single/labels"].max() == 0 and gold["rerank_n256/labels"].max() + 1 == 16
    # tie-heavy weights: the order among equal weights is the sort's business, and a stable sort gives other labels somewhere
    ties = {n: len(gold[n + "/mst_distance"]) - len(np.unique(gold[n + "/mst_distance"])) for n in NAMES}
    assert ties["n3001_half"] > 1000 and ties["n64_half"] >= 5
    dup = np.asarray(ref.matrix(ref.BY_NAME["n257_dup"]))
    assert (dup[~np.eye(257, dtype=bool)] == 0).sum() > 0
    assert (np.diag(np.asarray(ref.matrix(ref.BY_NAME["rerank_n256"]))) != 0).any()          # the re-rank diagonal is not zero
    F = np.asarray(ref.matrix(ref.BY_NAME["rerank_n256"]))
    assert np.array_equal(F, F.T)


# ------------------------------------------------------------------ the estimator without a device
def test_surface():
    import inspect
    import ssg_amd
    from ssg_amd import selftraining
    assert cluster.HDBSCAN is hdbscan.HDBSCAN is ssg_amd.HDBSCAN
    assert callable(selftraining.generate_selflabel_hdbscan) and ssg_amd.generate_selflabel_hdbscan is selftraining.generate_selflabel_hdbscan
    est = hdbscan.HDBSCAN()
    assert (est.min_cluster_size, est.min_samples, est.cluster_selection_epsilon, est.max_cluster_size, est.metric, est.metric_params) == (5, None, 0.0, None, "euclidean", None)
    assert (est.alpha, est.algorithm, est.leaf_size, est.n_jobs, est.cluster_selection_method, est.allow_single_cluster, est.store_centers, est.copy) == (
        1.0, "auto", 40, None, "eom", False, None, False)
    assert list(inspect.signature(hdbscan.HDBSCAN.__init__).parameters)[1:] == [
        "min_cluster_size", "min_samples", "cluster_selection_epsilon", "max_cluster_size", "metric", "metric_params", "alpha", "algorithm", "leaf_size", "n_jobs",
        "cluster_selection_method", "allow_single_cluster", "store_centers", "copy"]
    assert hdbscan.HDBSCAN(7).min_cluster_size == 7                     # positional, like sklearn's
    src = open(hdbscan.__file__).read()
    assert "import sklearn" not in src and "from sklearn" not in src
    assert hdbscan.HIERARCHY_dtype.names == ("left_node", "right_node", "value", "cluster_size")
    protos = _lib.parse_header()
    for name in ("ssg_hdbscan_check", "ssg_hdbscan_core_dist", "ssg_hdbscan_mst", "ssg_hdbscan_lds_max_n"):
        assert name in protos, name


def test_parameter_errors_and_their_order():
    X = np.zeros((8, 8))
    ok = dict(metric="precomputed")
    must = "The %r parameter of HDBSCAN must be %s. Got %r instead."
    for kw, name, text in ((dict(min_cluster_size=1), "min_cluster_size", "an int in the range [2, inf)"),
                           (dict(min_cluster_size=2.0), "min_cluster_size", "an int in the range [2, inf)"),
                           (dict(min_cluster_size=True), "min_cluster_size", "an int in the range [2, inf)"),
                           (dict(min_samples=0), "min_samples", "an int in the range [1, inf) or None"),
                           (dict(min_samples=1.5), "min_samples", "an int in the range [1, inf) or None"),
                           (dict(cluster_selection_epsilon=-1.0), "cluster_selection_epsilon", "a float in the range [0.0, inf)"),
                           (dict(cluster_selection_epsilon="x"), "cluster_selection_epsilon", "a float in the range [0.0, inf)"),
                           (dict(max_cluster_size=0), "max_cluster_size", "None or an int in the range [1, inf)"),
                           (dict(max_cluster_size=2.5), "max_cluster_size", "None or an int in the range [1, inf)"),
                           (dict(metric_params=3), "metric_params", "an instance of 'dict' or None"),
                           (dict(alpha=0.0), "alpha", "a float in the range (0.0, inf)"), (dict(alpha=0), "alpha", "a float in the range (0.0, inf)"),
                           (dict(alpha=float("inf")), "alpha", "a float in the range (0.0, inf)"), (dict(alpha=float("nan")), "alpha", "a float in the range (0.0, inf)"),
                           (dict(leaf_size=0), "leaf_size", "an int in the range [1, inf)"), (dict(n_jobs=1.5), "n_jobs", "an instance of 'int' or None"),
                           (dict(allow_single_cluster=1), "allow_single_cluster", "an instance of 'bool' or an instance of 'numpy.bool'"),
                           (dict(copy=1), "copy", "an instance of 'bool' or an instance of 'numpy.bool'")):
        with pytest.raises(ValueError) as e:
            hdbscan.HDBSCAN(**ok, **kw).fit(X)
        assert str(e.value) == must % (name, text, kw[name]), kw
    for kw, name, options in ((dict(algorithm="x"), "algorithm", ("auto", "ball_tree", "brute", "kd_tree")),
                              (dict(cluster_selection_method="x"), "cluster_selection_method", ("eom", "leaf")),
                              (dict(store_centers="x"), "store_centers", ("both", "centroid", "medoid"))):
        with pytest.raises(ValueError) as e:
            hdbscan.HDBSCAN(**ok, **kw).fit(X)
        msg = str(e.value)                                           # (sklearn prints the options in the order of a set)
        assert msg.startswith("The %r parameter of HDBSCAN must be " % name) and "a str among {" in msg and msg.endswith("}. Got 'x' instead.")
        assert all(repr(o) in msg for o in options)
    # sklearn checks the parameters in the order of their sorted names, then store_centers with a precomputed matrix
    with pytest.raises(ValueError, match="'algorithm' parameter"):
        hdbscan.HDBSCAN(min_cluster_size=1, algorithm="x", **ok).fit(X)
    with pytest.raises(ValueError, match="'alpha' parameter"):
        hdbscan.HDBSCAN(min_cluster_size=1, alpha=-1.0, **ok).fit(X)
    with pytest.raises(ValueError, match="'min_cluster_size' parameter"):
        hdbscan.HDBSCAN(min_cluster_size=1, store_centers="centroid", **ok).fit(X)
    with pytest.raises(ValueError) as e:
        hdbscan.HDBSCAN(store_centers="centroid", **ok).fit(np.full((3, 4), np.nan))
    assert str(e.value) == "Cannot store centers when using a precomputed distance matrix."
    for metric in ("euclidean", "minkowski", "cosine"):
        with pytest.raises(ValueError, match="metric='precomputed' only"):
            hdbscan.HDBSCAN(metric=metric).fit(X)
    # values sklearn accepts: a bool where a number is asked for, numpy's bool where a bool is
    hdbscan.HDBSCAN(alpha=True, leaf_size=True, n_jobs=True, cluster_selection_epsilon=True, copy=np.bool_(True), allow_single_cluster=np.bool_(False), **ok)._validate()


def test_shape_errors_and_their_order():
    """inputs that never reach the device, in sklearn's order: NaN, one sample, min_samples, not square"""
    ok = dict(metric="precomputed", min_cluster_size=2)
    with pytest.raises(ValueError) as e:
        hdbscan.HDBSCAN(**ok).fit(np.full((3, 4), np.nan))
    assert str(e.value) == "np.nan values found in precomputed-dense"
    with pytest.raises(ValueError) as e:
        hdbscan.HDBSCAN(**ok).fit(np.zeros((1, 1)))
    assert str(e.value) == "n_samples=1 while HDBSCAN requires more than one sample"
    with pytest.raises(ValueError) as e:
        hdbscan.HDBSCAN(**ok).fit(np.zeros((1, 4)))
    assert str(e.value) == "n_samples=1 while HDBSCAN requires more than one sample"
    with pytest.raises(ValueError) as e:
        hdbscan.HDBSCAN(metric="precomputed").fit(np.zeros((3, 4)))
    assert str(e.value) == "min_samples (5) must be at most the number of samples in X (3)"
    for shape in ((3, 4), (5, 4)):
        with pytest.raises(ValueError) as e:
            hdbscan.HDBSCAN(**ok).fit(np.zeros(shape))
        assert str(e.value) == ("The precomputed distance matrix is expected to be symmetric, however it has shape %r. Please verify that the distance "
                                "matrix was constructed correctly." % (shape,))
    with pytest.raises(ValueError, match="Expected 2D array, got 1D array instead"):
        hdbscan.HDBSCAN(**ok).fit(np.zeros(4))
    class Sparse:                                                    # (what a scipy.sparse matrix looks like from outside)
        shape = (4, 4)

        def tocsr(self):
            return self

    with pytest.raises(TypeError, match="sparse input is not supported"):
        hdbscan.HDBSCAN(**ok).fit(Sparse())
    with pytest.raises(TypeError, match="unsupported distance matrix type"):
        hdbscan.HDBSCAN(**ok).fit([[0.0, 1.0], [1.0, 0.0]])


class _FakeHandle:
    group, row0, mode, lambda_value, M, v, device = None, 0, 2, 0.0, None, None, None

    def __init__(self, n):
        self.N = self.nrows = n

    def validate(self):
        self.validated = True
        return self


def test_fit_plumbing_errors_and_the_warning(gold, monkeypatch):
    """fit with the device part replaced by the golden arrays: min_samples, alpha and the state reach the device call, the handle is
    validated first; NaN wins over asymmetry, both come from the counts of the one read; the infinite-edge warning is sklearn's; a
    sharded handle is refused; min_samples larger than N looks for NaN first"""
    seen = {}

    def fake(name, nan=0, asym=0):
        def run(h, k, alpha, state):
            seen.update(k=k, alpha=alpha, state=state, validated=getattr(h, "validated", False))
            return (nan, asym, gold[name + "/core"]) + _mst(gold, name)
        return run

    case = ref.BY_NAME["n257_half_a15"]
    h = _FakeHandle(257)
    monkeypatch.setattr(hdbscan, "_as_handle", lambda X: h)
    monkeypatch.setattr(hdbscan, "_device_mst", fake("n257_half_a15"))
    X = np.zeros((257, 257))
    est = hdbscan.HDBSCAN(metric="precomputed", min_cluster_size=4, min_samples=3, alpha=1.5)
    est.state = 2
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert est.fit_predict(X) is est.labels_
    assert seen == dict(k=3, alpha=1.5, state=2, validated=True) and est._min_samples == 3 and est.n_features_in_ == 257
    if np.array_equal(np.argsort(gold["n257_half_a15/mst_distance"]), gold["n257_half_a15/row_order"]):
        assert _same_bits(est.labels_, gold["n257_half_a15/labels"]) and _same_bits(est.probabilities_, gold["n257_half_a15/probs"])
    assert _same_bits(est._single_linkage_tree_["value"], gold["n257_half_a15/slt_value"]) and case["alpha"] == 1.5
    est = hdbscan.HDBSCAN(metric="precomputed", min_cluster_size=7).fit(X)
    assert seen["k"] == 7 and est._min_samples == 7 and seen["alpha"] == 1.0 and seen["state"] == 0
    for nan, asym, text in ((3, 0, "np.nan values found in precomputed-dense"), (3, 8, "np.nan values found in precomputed-dense"),
                            (0, 2, "The precomputed distance matrix is expected to be symmetric, however its values appear to be asymmetric. Please verify that "
                                   "the distance matrix was constructed correctly.")):
        monkeypatch.setattr(hdbscan, "_device_mst", fake("n257_half", nan, asym))
        with pytest.raises(ValueError) as e:
            hdbscan.HDBSCAN(metric="precomputed").fit(X)
        assert str(e.value) == text
    monkeypatch.setattr(hdbscan, "_device_mst", fake("n257_inf"))
    with pytest.warns(UserWarning) as w:
        hdbscan.HDBSCAN(metric="precomputed").fit(X)
    assert str(w[0].message) == ("The minimum spanning tree contains edge weights with value infinity. Potentially, you are missing too many distances in the "
                                 "initial distance matrix for the given neighborhood size.")
    # min_samples larger than N: sklearn has looked for NaN before
    for nan, text in ((0, "min_samples (300) must be at most the number of samples in X (257)"), (1, "np.nan values found in precomputed-dense")):
        monkeypatch.setattr(hdbscan, "_device_counts", lambda h, nan=nan: (nan, 0))
        with pytest.raises(ValueError) as e:
            hdbscan.HDBSCAN(metric="precomputed", min_samples=300).fit(X)
        assert str(e.value) == text
    h.group = object()
    with pytest.raises(ValueError, match="single GPU"):
        hdbscan.HDBSCAN(metric="precomputed").fit(X)
    h.group, h.N, h.nrows = None, 1, 1
    with pytest.raises(ValueError, match="n_samples=1 while HDBSCAN requires more than one sample"):
        hdbscan.HDBSCAN(metric="precomputed").fit(X)


# ------------------------------------------------------------------ the entry points' refusals
def test_entry_points_refuse_before_any_device_call():
    """everything outside the rules returns -1 and names the entry point in ssg_last_error -- no device is touched (this box has none)"""
    L = _lib.lib()
    P = ctypes.c_void_p
    a = P(4096)
    cap = L.ssg_hdbscan_lds_max_n()
    assert 16384 <= cap and cap * 8 + 256 <= 160 * 1024

    def chk(M=a, v=None, N=8, mode=2, counts=a):
        return L.ssg_hdbscan_check(M, v, N, mode, 0.0, counts, None)

    def core(M=a, v=None, N=8, mode=2, k=2, alpha=1.0, out=a):
        return L.ssg_hdbscan_core_dist(M, v, N, mode, 0.0, k, alpha, out, None)

    def mst(M=a, v=None, N=8, mode=2, core_=a, alpha=1.0, state=0, ws=a, ws_bytes=1 << 30, c=a, n=a, d=a):
        return L.ssg_hdbscan_mst(M, v, N, mode, 0.0, core_, alpha, state, ws, ws_bytes, c, n, d, None)

    for what, call in (("null matrix", lambda: chk(M=None)), ("N = 1", lambda: chk(N=1)), ("mode 3", lambda: chk(mode=3)), ("mode 0 without v", lambda: chk(mode=0)),
                       ("null counts", lambda: chk(counts=None)), ("misaligned counts", lambda: chk(counts=P(4100)))):
        assert call() == -1, what
        assert b"ssg_hdbscan_check" in L.ssg_last_error(), what
    for what, call in (("null matrix", lambda: core(M=None)), ("N = 1", lambda: core(N=1)), ("N = 0", lambda: core(N=0)), ("mode -1", lambda: core(mode=-1)),
                       ("mode 0 without v", lambda: core(mode=0)), ("min_samples = 0", lambda: core(k=0)), ("min_samples = N + 1", lambda: core(k=9)),
                       ("null output", lambda: core(out=None)), ("alpha = 0", lambda: core(alpha=0.0)), ("negative alpha", lambda: core(alpha=-1.0)),
                       ("infinite alpha", lambda: core(alpha=float("inf"))), ("NaN alpha", lambda: core(alpha=float("nan")))):
        assert call() == -1, what
        assert b"ssg_hdbscan_core_dist" in L.ssg_last_error(), what
    for what, call in (("null matrix", lambda: mst(M=None)), ("N = 1", lambda: mst(N=1)), ("mode 3", lambda: mst(mode=3)), ("mode 0 without v", lambda: mst(mode=0)),
                       ("null core", lambda: mst(core_=None)), ("null current", lambda: mst(c=None)), ("null next", lambda: mst(n=None)),
                       ("null distance", lambda: mst(d=None)), ("misaligned distance", lambda: mst(d=P(4100))), ("alpha = 0", lambda: mst(alpha=0.0)),
                       ("NaN alpha", lambda: mst(alpha=float("nan"))), ("state 3", lambda: mst(state=3)), ("state -1", lambda: mst(state=-1)),
                       ("LDS state beyond its capacity", lambda: mst(N=cap + 1, state=1)), ("global state without a workspace", lambda: mst(state=2, ws=None)),
                       ("global state, short workspace", lambda: mst(state=2, ws_bytes=63)), ("auto beyond LDS without a workspace", lambda: mst(N=cap + 1, ws=None)),
                       ("unaligned workspace", lambda: mst(state=2, ws=P(4100)))):
        assert call() == -1, what
        assert b"ssg_hdbscan_mst" in L.ssg_last_error(), what
    with pytest.raises(ValueError, match="ssg_hdbscan_mst"):
        _lib.check(mst(state=3), "ssg_hdbscan_mst")


# ------------------------------------------------------------------ the scalar rules of hdbscan.hip, compiled for x86
@pytest.fixture(scope="module")
def hx(tmp_path_factory):
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else (shutil.which("g++") or shutil.which("c++"))
    assert cxx, "no C++ compiler"
    d = tmp_path_factory.mktemp("hx_hdbscan")
    out, on = [], False
    for line in open(os.path.join(ROOT, "self-similarity-grouping_amd", "csrc", "hdbscan.hip")):
        if "end of the scalar rules" in line:
            break
        if on:
            out.append(line)
        if "the scalar rules (tests/test_hdbscan_host.py" in line:
            on = True
    text = "".join(out)
    for name in ("hdbscan_mreach", "hdbscan_min_update", "hdbscan_better", "hdbscan_close"):
        assert "__device__ __forceinline__" in text and name + "(" in text, name
    (d / "hdbscan_cut.inc").write_text(text)
    so = str(d / "libhx_hdbscan.so")
    r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I" + str(d), "-o", so,
                        os.path.join(ROOT, "tools", "hostexec", "hdbscan_rules.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # the kernels use the rules they publish: no second copy of the comparisons outside the marked text
    rest = open(os.path.join(ROOT, "self-similarity-grouping_amd", "csrc", "hdbscan.hip")).read().split("end of the scalar rules")[1]
    for name in ("hdbscan_mreach(", "hdbscan_min_update(", "hdbscan_better(", "hdbscan_close("):
        assert name in rest, name
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _edge_values():
    tiny = 5e-324
    return np.array([0.0, -0.0, tiny, -tiny, 1e-320, 2.2250738585072014e-308, 1e-300, 1e-9, 1e-7, 0.1, 0.1 + 0.2, 0.3, 1 / 3, 0.5, 1.0, np.nextafter(1.0, 2), np.nextafter(1.0, 0),
                     2.0, 65504.0, 1e100, 1.7976931348623157e308, np.inf, -1.0, -np.inf])


def test_three_way_max_and_min_update_are_numpy(hx):
    v = _edge_values()
    rng = np.random.RandomState(2)
    extra = np.float16(rng.uniform(0, 3, 40)).astype(np.float64)         # tie-heavy, like a half matrix
    v = np.concatenate([v, extra])
    a, b, c = (x.ravel().copy() for x in np.meshgrid(v, v, v, indexing="ij"))
    got = np.empty_like(a)
    hx.hx_hdbscan_mreach(_p(a), _p(b), _p(c), ctypes.c_long(a.size), _p(got))
    want = np.array([max(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())])      # max(core[c], core[j], d): the first of equal values
    assert _same_bits(got, want)
    assert np.array_equal(got, np.maximum(np.maximum(a, b), c))                                  # and numpy's value
    m, r = (x.ravel().copy() for x in np.meshgrid(v, v, indexing="ij"))
    got = np.empty_like(m)
    hx.hx_hdbscan_min_update(_p(m), _p(r), ctypes.c_long(m.size), _p(got))
    assert np.array_equal(got, np.minimum(m, r))
    nz = ~((m == 0) & (r == 0))
    assert _same_bits(got[nz], np.minimum(m, r)[nz])                      # bit for bit wherever the two are not both a zero
    assert ((m == r) & nz).sum() > 50 and (m < r).sum() > 500 and (m > r).sum() > 500


def test_argmin_tie_rule(hx):
    """a step on an all-zero row with core 0 leaves the state as it is: the arg-min alone, folded in both directions"""
    rng = np.random.RandomState(5)
    hx.hx_hdbscan_step.restype = ctypes.c_long
    for trial in range(200):
        n = int(rng.randint(1, 40))
        m = rng.choice([0.25, 0.5, 0.5, 1.0, np.inf, np.inf], size=n)
        if trial % 5 == 0:
            m[:] = np.inf                                    # nothing reachable: the smallest remaining index
        S = np.where(rng.uniform(size=n) < 0.4, np.nan, m)
        idx = np.flatnonzero(~np.isnan(S))
        want = int(idx[np.argmin(S[idx])]) if idx.size else -1
        for desc in (0, 1):
            state, best = S.copy(), ctypes.c_double(-1.0)
            d = np.full(n, np.inf)                           # an infinite row improves nothing
            got = hx.hx_hdbscan_step(_p(d), _p(d), ctypes.c_double(0.0), ctypes.c_long(n), desc, _p(state), ctypes.byref(best))
            assert got == want, (trial, desc)
            assert _same_bits(state, S) and (want < 0 or best.value == S[want])


@pytest.mark.parametrize("name", ["n7", "n65_all", "n257_half_a15", "n257_dup", "n257_inf", "rerank_n256"])
def test_compiled_rules_walk_the_golden_tree(hx, gold, name):
    """the loop of hdbscan.hip with its compiled rules (three-way max, min-update, arg-min) and the data movement in numpy gives the golden"""
    case = ref.BY_NAME[name]
    X = np.ascontiguousarray(ref.matrix(case), dtype=np.float64)
    n, alpha = case["N"], case["alpha"]
    core = np.ascontiguousarray(np.sort(X, axis=1)[:, ref.min_samples_of(case) - 1] / alpha)
    assert _same_bits(core, gold[name + "/core"])
    hx.hx_hdbscan_step.restype = ctypes.c_long
    S = np.full(n, np.inf)
    cur, nxt, dist = np.empty(n - 1, np.int64), np.empty(n - 1, np.int64), np.empty(n - 1)
    c = 0
    for t in range(n - 1):
        S[c] = np.nan
        row = np.ascontiguousarray(X[c] / alpha)
        best = ctypes.c_double()
        j = hx.hx_hdbscan_step(_p(row), _p(core), ctypes.c_double(core[c]), ctypes.c_long(n), t & 1, _p(S), ctypes.byref(best))
        cur[t], nxt[t], dist[t] = c, j, best.value
        c = j
    for g, key in zip((cur, nxt, dist), MST):
        assert _same_bits(g, gold["%s/%s" % (name, key)]), (name, key)


def test_allclose_predicate_is_numpy_at_and_beyond_its_bound(hx):
    rng = np.random.RandomState(9)
    base = np.concatenate([rng.uniform(0, 2, 2000), np.float16(rng.uniform(0, 2, 500)).astype(np.float64), np.exp(rng.uniform(np.log(1e-12), np.log(1e6), 1500)),
                           [0.0, 1e-9, 1e-7, 1.0, 100.0]])
    xs, ys = [], []
    for y in (base, -base):
        tol = 1e-9 + 1e-7 * np.abs(y)
        for f in (0.0, 0.5, 1.0, -1.0, 1.0000001, 2.0, -2.0):
            x = y + f * tol                                   # around the bound
            for steps in (0, 1, -1, 2, -2):                   # and a few ulps to either side of it
                xx = x.copy()
                for _ in range(abs(steps)):
                    xx = np.nextafter(xx, np.inf if steps > 0 else -np.inf)
                xs.append(xx); ys.append(y)
    e = _edge_values()
    ex, ey = (g.ravel() for g in np.meshgrid(e, e, indexing="ij"))
    xs.append(ex); ys.append(ey)
    x, y = np.ascontiguousarray(np.concatenate(xs)), np.ascontiguousarray(np.concatenate(ys))
    got = np.empty(x.size, np.uint8)
    hx.hx_hdbscan_close(_p(x), _p(y), ctypes.c_long(x.size), _p(got))
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.isclose(x, y, rtol=1e-7, atol=1e-9)
        by_hand = (np.abs(x - y) <= 1e-9 + 1e-7 * np.abs(y)) & np.isfinite(y) | (x == y)
    assert np.array_equal(got.astype(bool), want) and np.array_equal(want, by_hand)
    assert want.sum() > 10000 and (~want).sum() > 10000
    inf = np.inf
    for a, b, close in ((inf, inf, True), (-inf, -inf, True), (inf, -inf, False), (inf, 1.0, False), (1.0, inf, False), (0.0, -0.0, True), (1e-9, 0.0, True),
                        (np.nextafter(1e-9, 1), 0.0, False), (0.0, 1e-9, True)):
        o = np.empty(1, np.uint8)
        hx.hx_hdbscan_close(_p(np.array([a])), _p(np.array([b])), ctypes.c_long(1), _p(o))
        assert bool(o[0]) == close == bool(np.isclose(a, b, rtol=1e-7, atol=1e-9)), (a, b)
