"""CPU half of the agglomerative tests: the restatement of tests/agglomerative_ref.py against what scipy 1.15.3 and sklearn 1.7.2 gave
(tests/golden/agglomerative_cases.npz; live scipy and sklearn where they import), the product's host stage (ssg_amd/agglomerative.py: the
stable sort, `label`, the cut, the small-cluster rule) fed the golden merges, every parameter error with its text, and the refusals of
the three entry points, which are made before any device call; and the scalar rules of csrc/agglomerative.hip -- the better-than order, the
previous-element rule, the complete, average and single updates -- compiled for x86 from the SAME SOURCE TEXT
(tools/hostexec/agglomerative_rules.cpp) and held to numpy and to scipy's loop."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import agglomerative_ref as ref

NAMES = [c["name"] for c in ref.CASES]


@pytest.fixture(scope="module")
def gold():
    return ref.load_golden()


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _fits(gold, key, N):
    """(tag, n_clusters, distance_threshold) of every stored fit"""
    return [("k%d" % k, k, None) for k in ref.n_clusters_options(N)] + [("t%d" % i, None, float(t)) for i, t in enumerate(gold[key + "/thresholds"])]


@pytest.mark.parametrize("method", ref.LINKAGES)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_scipy_and_sklearn(gold, name, method):
    """the restated loops, sort, label and cut give the golden Z, merges and labels; the entry-by-entry loops agree where N is small;
    live scipy and sklearn give the golden too where they import"""
    case, key = ref.BY_NAME[name], "%s/%s" % (name, method)
    D = ref.matrix(case)
    stats = {}
    x, y, d, s = ref.merges(D, method, stats=stats)
    assert _same_bits(x, gold[key + "/x"]) and _same_bits(y, gold[key + "/y"]) and _same_bits(d, gold[key + "/d"])
    if method != "single":
        assert _same_bits(s, gold[key + "/size"]) and stats["scans"] <= 3 * (case["N"] - 1)
        if case["kind"] == "prevtie":
            assert stats["prev_kept"] >= 1, "the case must show chain[-2] keeping a tie against a lower-indexed slot"
    Z = ref.label(x, y, d)
    assert _same_bits(Z, gold[key + "/Z"])
    if case["N"] <= ref.LITERAL_MAX_N:
        for a, b in zip(ref.merges(D, method, literal=True), (x, y, d, s)):
            assert (a is None and b is None) or _same_bits(a, b)
    assert _same_bits(np.array(ref.thresholds(Z)), gold[key + "/thresholds"])
    for tag, k, t in _fits(gold, key, case["N"]):
        _, n_clusters, labels = ref.fit(Z, k, t)
        assert n_clusters == int(gold["%s/%s/n_clusters" % (key, tag)]) and np.array_equal(labels, gold["%s/%s/labels" % (key, tag)]), (key, tag)
    try:
        from scipy.cluster.hierarchy import linkage
        from sklearn.cluster import AgglomerativeClustering
    except ImportError:
        return
    assert _same_bits(linkage(ref.condensed(D), method=method), Z)
    tag, k, t = _fits(gold, key, case["N"])[-2]
    est = AgglomerativeClustering(n_clusters=k, distance_threshold=t, metric="precomputed", linkage=method).fit(np.array(D, dtype=np.float64))
    assert np.array_equal(est.labels_, gold["%s/%s/labels" % (key, tag)])


def test_the_cases_cover_what_they_are_for(gold):
    assert {c["N"] for c in ref.CASES} >= {2, 3, 17, 65, 130, 257, 1025} and any(1400 <= c["N"] <= 1600 for c in ref.CASES)
    D = ref.matrix(ref.BY_NAME["n130_asym"])
    assert not np.array_equal(D, D.T)
    Dn = ref.matrix(ref.BY_NAME["n130_neg"])
    assert (Dn < 0).any() and np.signbit(Dn[Dn == 0]).any() and not np.signbit(Dn[Dn == 0]).all()
    assert len(np.unique(ref.matrix(ref.BY_NAME["n65_equal"]))) == 1
    for name in ("n65_q16", "n257_q16", "n1025_q16"):
        Dq = ref.matrix(ref.BY_NAME[name])
        assert Dq.dtype == np.float16 and len(np.unique(Dq)) <= 8
    # the lower triangle and the diagonal take no part: scrambling them changes nothing
    case = ref.BY_NAME["n65_q16"]
    X = np.array(ref.matrix(case), dtype=np.float64)
    X[np.tril_indices(len(X))] = np.random.RandomState(0).uniform(-5, 5, len(np.tril_indices(len(X))[0]))
    for method in ref.LINKAGES:
        assert _same_bits(ref.linkage(X, method), gold["n65_q16/%s/Z" % method])


@pytest.mark.parametrize("method", ref.LINKAGES)
@pytest.mark.parametrize("name", NAMES)
def test_host_stage_on_the_golden_merges(gold, name, method):
    """ssg_amd.agglomerative's host stage -- the stable sort, label, the cut -- fed the golden merges gives the golden Z, children_,
    distances_, n_clusters_ and labels_"""
    from ssg_amd import agglomerative as ag
    case, key = ref.BY_NAME[name], "%s/%s" % (name, method)
    Z = ag._label(gold[key + "/x"], gold[key + "/y"], gold[key + "/d"])
    assert _same_bits(Z, gold[key + "/Z"])
    children = Z[:, :2].astype(int)
    for tag, k, t in _fits(gold, key, case["N"]):
        n_clusters = k if t is None else int(np.count_nonzero(Z[:, 2] >= t)) + 1
        assert n_clusters == int(gold["%s/%s/n_clusters" % (key, tag)])
        labels = ag._hc_cut(n_clusters, children, case["N"])
        assert labels.dtype == np.intp and np.array_equal(labels, gold["%s/%s/labels" % (key, tag)]), (key, tag)
        for m in (1, 2, 4, 9):
            assert np.array_equal(ag._drop_small(labels, m), ref.drop_small(labels, m)), (key, tag, m)
    with pytest.raises(ValueError, match=r"Cannot extract more clusters than samples: %d clusters were given for a tree with %d leaves\." % (case["N"] + 1, case["N"])):
        ag._hc_cut(case["N"] + 1, children, case["N"])


def test_small_cluster_rule():
    from ssg_amd.agglomerative import _drop_small
    lab = np.array([3, 3, 0, 3, 1, 1, 0, 2, 3, 1, 1])
    assert _drop_small(lab, 4).tolist() == [0, 0, -1, 0, 1, 1, -1, -1, 0, 1, 1]
    assert _drop_small(lab, 2).tolist() == [0, 0, 1, 0, 2, 2, 1, -1, 0, 2, 2]
    assert _drop_small(lab, 1).tolist() == [0, 0, 1, 0, 2, 2, 1, 3, 0, 2, 2]
    assert _drop_small(lab, 5).tolist() == [-1] * 11


PRE = "The %r parameter of AgglomerativeClustering must be "


@pytest.mark.parametrize("kw, text", [
    (dict(n_clusters=0), PRE % "n_clusters" + "an int in the range [1, inf) or None. Got 0 instead."),
    (dict(n_clusters=2.0), PRE % "n_clusters" + "an int in the range [1, inf) or None. Got 2.0 instead."),
    (dict(metric="foo"), " or a callable. Got 'foo' instead."),
    (dict(memory=3), PRE % "memory" + "an instance of 'str', an object implementing 'cache' or None. Got 3 instead."),
    (dict(connectivity=3), PRE % "connectivity" + "an array-like, a sparse matrix, a callable or None. Got 3 instead."),
    (dict(compute_full_tree="x"), PRE % "compute_full_tree" + "a str among {'auto'} or an instance of 'bool' or an instance of 'numpy.bool'. Got 'x' instead."),
    (dict(linkage="foo"), "}. Got 'foo' instead."),
    (dict(n_clusters=None, distance_threshold=-1.0), PRE % "distance_threshold" + "a float in the range [0.0, inf) or None. Got -1.0 instead."),
    (dict(compute_distances=1), PRE % "compute_distances" + "an instance of 'bool' or an instance of 'numpy.bool'. Got 1 instead."),
])
def test_parameter_constraints(kw, text):
    """sklearn's _parameter_constraints with its texts (the options of a str parameter are printed sorted; sklearn prints a set); they
    are checked before X is looked at, so X may be anything; sklearn itself gives the same text where it imports"""
    from ssg_amd import AgglomerativeClustering
    base = dict(metric="precomputed", linkage="average")
    base.update(kw)
    with pytest.raises(ValueError) as e:
        AgglomerativeClustering(**base).fit(None)
    assert str(e.value).endswith(text) and str(e.value).startswith(PRE % next(iter(k for k in kw if k != "n_clusters" or len(kw) == 1)))
    try:
        from sklearn.cluster import AgglomerativeClustering as Sk
    except ImportError:
        return
    with pytest.raises(ValueError) as s:
        Sk(**base).fit(np.zeros((3, 3)))
    if "a str among {'" not in text and "callable" not in text and not text.startswith("}"):
        assert str(s.value) == str(e.value)
    else:
        assert str(s.value).endswith(text) and sorted(str(s.value)) == sorted(str(e.value))       # the same options in another order


def test_fit_refusals_in_sklearn_s_order():
    """what sklearn's _fit refuses after it has validated X, first match first; and this class's own refusal of what it does not
    implement, which comes after them"""
    from ssg_amd import AgglomerativeClustering as A
    from ssg_amd.agglomerative import _FULL_TREE, _ONE_OF
    base = dict(metric="precomputed", linkage="average")
    assert _ONE_OF == "Exactly one of n_clusters and distance_threshold has to be set, and the other needs to be None."
    assert _FULL_TREE == "compute_full_tree must be True if distance_threshold is set."
    assert str(A(n_clusters=2, distance_threshold=1.0, **base)._fit_errors()) == _ONE_OF
    assert str(A(n_clusters=None, **base)._fit_errors()) == _ONE_OF
    assert str(A(n_clusters=2, distance_threshold=1.0, compute_full_tree=False, metric="precomputed", linkage="ward")._fit_errors()) == _ONE_OF
    assert str(A(n_clusters=None, distance_threshold=1.0, compute_full_tree=False, **base)._fit_errors()) == _FULL_TREE
    assert str(A(n_clusters=None, distance_threshold=1.0, compute_full_tree=False, metric="precomputed", linkage="ward")._fit_errors()) == _FULL_TREE
    assert str(A(n_clusters=2, metric="precomputed", linkage="ward")._fit_errors()) == "precomputed was provided as metric. Ward can only work with euclidean distances."
    for kw in (dict(metric="euclidean", linkage="average"), dict(metric="euclidean"), dict(metric="cosine", linkage="single"),
               dict(metric="precomputed", linkage="complete", connectivity=np.eye(3)), dict(metric=lambda X: X, linkage="average")):
        err = A(n_clusters=2, **kw)._fit_errors()
        assert isinstance(err, ValueError) and "implements the precomputed, unconstrained case only" in str(err), kw
    for kw in (dict(n_clusters=2), dict(n_clusters=None, distance_threshold=0.0), dict(n_clusters=True), dict(n_clusters=2, compute_full_tree=False),
               dict(n_clusters=2, memory="/nonexistent", pooling_func=np.mean), dict(n_clusters=np.int64(3), compute_distances=True)):
        for linkage in ("average", "complete", "single"):
            est = A(metric="precomputed", linkage=linkage, **kw)
            est._validate()
            assert est._fit_errors() is None
    # sklearn's defaults
    d = A()
    assert (d.n_clusters, d.metric, d.memory, d.connectivity, d.compute_full_tree, d.linkage, d.distance_threshold, d.compute_distances) == (
        2, "euclidean", None, None, "auto", "ward", None, False)
    import ssg_amd
    from ssg_amd import cluster
    assert cluster.AgglomerativeClustering is A and ssg_amd.agglomerative.AgglomerativeClustering is A


def test_inputs_refused_before_the_device():
    """an input that is not a square of at least two samples never reaches the device: sklearn's refusals in its order (NaN, infinity,
    too few samples, not square)"""
    import torch
    from ssg_amd import AgglomerativeClustering as A
    from ssg_amd.agglomerative import _NAN, linkage
    fit = lambda X, **kw: A(n_clusters=kw.pop("n_clusters", 1), metric="precomputed", linkage="average", **kw).fit(X)      # noqa: E731
    assert _NAN.startswith("Input X contains NaN.\nAgglomerativeClustering does not accept missing values encoded as NaN natively.")
    X = np.arange(15, dtype=np.float64).reshape(3, 5)
    with pytest.raises(ValueError, match=r"^Distance matrix should be square, got matrix of shape \(3, 5\)$"):
        fit(X)
    with pytest.raises(ValueError, match=r"^Distance matrix should be square, got matrix of shape \(3, 5\)$"):
        fit(torch.from_numpy(X))
    with pytest.raises(ValueError, match=r"^Found array with 1 sample\(s\) \(shape=\(1, 1\)\) while a minimum of 2 is required by AgglomerativeClustering\.$"):
        fit(X[:1, :1])
    with pytest.raises(ValueError, match=r"^Found array with 1 sample\(s\) \(shape=\(1, 5\)\) while a minimum of 2 is required by AgglomerativeClustering\.$"):
        fit(X[:1])
    with pytest.raises(ValueError, match="Expected 2D array, got 1D array instead"):
        fit(X[0])
    Y = X.copy()
    Y[2, 4] = np.inf
    for dt in (np.float64, np.float32, np.float16):
        with pytest.raises(ValueError) as e:
            fit(Y.astype(dt))
        assert str(e.value) == "Input X contains infinity or a value too large for dtype('%s')." % np.dtype(dt).name
    Y[0, 1] = np.nan
    with pytest.raises(ValueError) as e:
        fit(Y)
    assert str(e.value) == _NAN
    with pytest.raises(ValueError) as e:
        fit(Y, n_clusters=2, distance_threshold=1.0)             # X is validated before _fit refuses the parameters
    assert str(e.value) == _NAN
    with pytest.raises(ValueError, match="implements the methods"):
        linkage(X, "ward")
    with pytest.raises(TypeError):
        fit([[0.0, 1.0], [1.0, 0.0]])
    try:
        from sklearn.cluster import AgglomerativeClustering as Sk
    except ImportError:
        return
    with pytest.raises(ValueError) as s:
        Sk(n_clusters=1, metric="precomputed", linkage="average").fit(Y)
    assert str(s.value) == _NAN


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """SSG_ERR_INVALID before any device call: null or misaligned pointers, N < 2, a bad mode, method or state, a bad pitch, a missing
    workspace; every message names its entry point"""
    from ssg_amd import _lib
    L = _lib.lib()
    P = lambda a: ctypes.c_void_p(a)      # noqa: E731  (never dereferenced: every call below is refused)
    M, v, W, C = P(0x10000), P(0x20000), P(0x40000), P(0x80000)
    assert L.ssg_agglo_lds_max_n() % 4 == 0 and 16000 <= L.ssg_agglo_lds_max_n() <= 160 * 1024 // 8
    bad_check = [(None, v, 8, 1, C), (M, v, 1, 1, C), (M, v, 8, 3, C), (M, v, 8, -1, C), (M, None, 8, 0, C), (M, v, 8, 1, None), (M, v, 8, 1, P(0x80004)),
                 (P(0x10001), v, 8, 1, C), (P(0x10004), v, 8, 2, C), (M, P(0x20001), 8, 0, C)]
    for (m, vv, n, mode, c) in bad_check:
        assert L.ssg_agglo_check(m, vv, n, mode, 0.3, c, None) == -1, (m, vv, n, mode, c)
        assert b"ssg_agglo_check" in L.ssg_last_error()
    bad_expand = [(None, v, 8, 1, W, 8), (M, v, 1, 1, W, 8), (M, v, 8, 5, W, 8), (M, None, 8, 0, W, 8), (M, v, 8, 1, None, 8), (M, v, 8, 1, P(0x40010), 8),
                  (M, v, 8, 1, W, 4), (M, v, 9, 1, W, 9), (M, v, 9, 1, W, 10), (M, v, 8, 1, W, 0)]
    for (m, vv, n, mode, w, ld) in bad_expand:
        assert L.ssg_agglo_expand(m, vv, n, mode, 0.3, w, ld, None) == -1, (m, vv, n, mode, w, ld)
        assert b"ssg_agglo_expand" in L.ssg_last_error()
    x, y, d, s, f, ws = P(0x100000), P(0x200000), P(0x300000), P(0x400000), P(0x500000), P(0x600000)
    big = L.ssg_agglo_lds_max_n() + 4
    good = dict(W=W, N=8, ld=8, method=0, state=0, counts=C, ws=ws, ws_bytes=64, x=x, y=y, d=d, s=s, f=f)
    bad_loop = [dict(W=None), dict(W=P(0x40008)), dict(N=1), dict(ld=4), dict(ld=9), dict(method=3), dict(method=-1), dict(state=3), dict(state=-1), dict(counts=None),
                dict(x=None), dict(y=None), dict(d=None), dict(s=None), dict(f=None), dict(x=P(0x100004)), dict(f=P(0x500004)), dict(counts=P(0x80004)),
                dict(N=big, ld=big, state=1), dict(N=big, ld=big, state=0, ws=None), dict(N=big, ld=big, state=2, ws_bytes=big * 8 - 8),
                dict(state=2, ws=None), dict(state=2, ws_bytes=56), dict(state=2, ws=P(0x600008))]
    for change in bad_loop:
        a = dict(good)
        a.update(change)
        rc = L.ssg_agglo_nn_chain(a["W"], a["N"], a["ld"], a["method"], a["state"], a["counts"], a["ws"], a["ws_bytes"], a["x"], a["y"], a["d"], a["s"], a["f"], None)
        assert rc == -1, change
        assert b"ssg_agglo_nn_chain" in L.ssg_last_error()


# ------------------------------------------------------------------ the scalar rules of agglomerative.hip, compiled for x86
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "self-similarity-grouping_amd", "csrc", "agglomerative.hip")
RULES = ("agglo_better", "agglo_prev_keeps", "agglo_complete", "agglo_average", "agglo_min_update")


@pytest.fixture(scope="module")
def hx(tmp_path_factory):
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else (shutil.which("g++") or shutil.which("c++"))
    assert cxx, "no C++ compiler"
    d = tmp_path_factory.mktemp("hx_agglomerative")
    out, on = [], False
    for line in open(HIP):
        if "end of the scalar rules" in line:
            break
        if on:
            out.append(line)
        if "the scalar rules (tests/test_agglomerative_host.py" in line:
            on = True
    text = "".join(out)
    for name in RULES:
        assert "__device__ __forceinline__" in text and name + "(" in text, name
    (d / "agglomerative_cut.inc").write_text(text)
    so = str(d / "libhx_agglomerative.so")
    r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I" + str(d), "-o", so,
                        os.path.join(ROOT, "tools", "hostexec", "agglomerative_rules.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # the kernels use the rules they publish
    rest = open(HIP).read().split("end of the scalar rules")[1]
    for name in RULES:
        assert name + "(" in rest, name
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_update_rules_are_scipy_s(hx):
    """the average update is two products, a sum and a quotient rounded once each (numpy's separate operations; a fused multiply-add
    gives other bits on a part of these inputs); the complete update and the single-linkage min-update keep the first of equal values,
    signed zeros included"""
    from fractions import Fraction
    rs = np.random.RandomState(3)
    n = 20000
    da = np.concatenate([rs.uniform(0, 3, n), np.float16(rs.uniform(0, 3, n)).astype(np.float64), rs.standard_normal(n) * 1e-3])
    db = np.concatenate([rs.uniform(0, 3, n), np.float16(rs.uniform(0, 3, n)).astype(np.float64), rs.standard_normal(n) * 1e3])
    na, nb = rs.randint(1, 9000, 3 * n).astype(np.int32), rs.randint(1, 9000, 3 * n).astype(np.int32)
    got = np.empty_like(da)
    hx.hx_agglo_average(_p(da), _p(db), _p(na), _p(nb), ctypes.c_long(da.size), _p(got))
    want = (na.astype(np.float64) * da + nb.astype(np.float64) * db) / (na + nb).astype(np.float64)
    assert _same_bits(got, want)
    fused = 0
    for i in range(300):                                       # what a fused na * da + (nb * db) would give: the sum rounded once from the exact product
        prod = nb[i].astype(np.float64) * db[i]
        exact = Fraction(int(na[i])) * Fraction(float(da[i])) + Fraction(float(prod))
        fused += float(exact) / float(na[i] + nb[i]) != want[i]
    assert fused >= 5, "the inputs must tell a fused multiply-add from two roundings"
    v = np.array([0.0, -0.0, 5e-324, -5e-324, 0.25, 0.5, 0.5, 1.0, np.nextafter(1.0, 2), 2.0, -1.0, -0.5, 1e300, -1e300])
    a, b = (x.ravel().copy() for x in np.meshgrid(v, v, indexing="ij"))
    got = np.empty_like(a)
    hx.hx_agglo_complete(_p(a), _p(b), ctypes.c_long(a.size), _p(got))
    assert _same_bits(got, np.array([max(x, y) for x, y in zip(a.tolist(), b.tolist())]))          # Cython's max(d_xi, d_yi): the first of equal values
    hx.hx_agglo_min_update(_p(a), _p(b), ctypes.c_long(a.size), _p(got))
    assert _same_bits(got, np.array([y if x > y else x for x, y in zip(a.tolist(), b.tolist())]))   # `if D[k] > dist: D[k] = dist`


def test_scan_rule_is_scipy_s_in_any_fold_order(hx):
    """the arg-min folded on (value, index) in ascending or descending order, then the previous-element rule once, against scipy's loop
    entry by entry: start at (p, row[p]), move only on a strictly smaller value"""
    rs = np.random.RandomState(4)
    kept = moved = 0
    for trial in range(400):
        n = int(rs.randint(2, 40))
        row = rs.randint(0, 4, n).astype(np.float64) / 4.0 - (0.5 if trial % 3 == 0 else 0.0)
        size = (rs.uniform(size=n) < 0.7).astype(np.int32)
        x = int(rs.randint(0, n))
        others = [i for i in range(n) if size[i] > 0 and i != x]
        if not others:
            continue
        p = int(others[rs.randint(0, len(others))]) if trial % 4 else -1
        y, cur = (p, row[p]) if p >= 0 else (-1, np.inf)
        for i in range(n):
            if size[i] == 0 or i == x:
                continue
            if row[i] < cur:
                cur, y = row[i], i
        for descending in (0, 1):
            c = ctypes.c_double()
            hx.hx_agglo_scan.restype = ctypes.c_long
            got = hx.hx_agglo_scan(_p(row), _p(size), ctypes.c_long(n), ctypes.c_long(x), ctypes.c_long(p), descending, ctypes.byref(c))
            assert (got, c.value) == (y, cur), (trial, descending)
        if p >= 0 and y == p and any(row[i] == row[p] and i < p for i in others):
            kept += 1
        if p >= 0 and y != p:
            moved += 1
    assert kept > 20 and moved > 20
