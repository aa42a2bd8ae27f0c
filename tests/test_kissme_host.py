"""CPU suite of the metric learners (ssg_amd/metric_learning.py, ssg_amd/dist_metric.py): the float64 restatement of
tests/kissme_ref.py against what the untouched reference did (tests/golden/kissme_cases.npz, tools/make_golden_kissme.py),
validate_cov_matrix bit for bit, the factory and its errors, and the argument validation of the ssg_kissme_* / ssg_pairdiff_cov_f64
entry points (no launch)."""
import ctypes

import numpy as np
import pytest

import kissme_ref as kr


@pytest.fixture(scope="module")
def g(golden):
    return golden("kissme_cases.npz")


def test_case_table_matches_the_golden(g):
    assert list(g["names"]) == sorted(kr.CASES)
    for name in kr.CASES:
        X, y = kr.make_case(name)
        assert X.dtype == np.float32 and np.array_equal(X, g[name + "_X"]) and np.array_equal(y, g[name + "_y"]) and y.dtype == g[name + "_y"].dtype
        assert int(g[name + "_seed"]) == kr.FIT_SEED[name]
    P = {n: int(g[n + "_ia1"].shape[0]) for n in kr.CASES}
    assert P == {"A": 1344, "B": 336, "C": 600, "D": 485} and P["C"] % 16 == 8 and P["D"] % 2 == 1
    assert int(g["A_eig_rounds"]) == 0 and int(g["B_eig_rounds"]) == 3          # A is positive definite at once, B takes three rounds
    assert kr.make_case("D")[0].shape[1] % 16 != 0 and kr.make_case("D")[1].dtype == np.float32


@pytest.mark.parametrize("name", sorted(kr.CASES))
def test_restatement_index_pairs_equal_the_references(g, name):
    _, y = kr.make_case(name)
    ia1, ib1, p, ia0, ib0 = kr.index_pairs(y, rng=np.random.RandomState(kr.FIT_SEED[name]))
    for got, key in ((ia1, "ia1"), (ib1, "ib1"), (p, "p"), (ia0, "ia0"), (ib0, "ib0")):
        assert np.array_equal(got, g["%s_%s" % (name, key)]), key
    # the position -> pair rule of the device, restated in numpy int64, gives the same sampled pairs
    a, b, total = kr.unrank_rule(y, p)
    assert np.array_equal(a, ia0) and np.array_equal(b, ib0) and total == y.shape[0] * (y.shape[0] - 1) // 2 - ia1.shape[0]


@pytest.mark.parametrize("name", sorted(kr.CASES))
def test_stream_next_draw_for_every_kind_of_rng(g, name):
    """np.random, a RandomState and a seed leave the stream where the reference's fit left it: `_stream` hands out the object whose
    .choice kissme.py:46 calls, and fit calls it once with (num_non_matches, num_matches, replace=False)"""
    from ssg_amd import metric_learning as ml
    _, y = kr.make_case(name)
    _, _, m = kr.pair_order(y)
    nm, nn = int(m.sum()), int((~m).sum())
    seed = kr.FIT_SEED[name]
    state = np.random.get_state()
    try:
        np.random.seed(seed)
        assert ml._stream(np.random) is np.random
        p = ml._stream(np.random).choice(nn, nm, replace=False)
        nxt = np.random.randint(0, 2 ** 31 - 1, size=4)
    finally:
        np.random.set_state(state)
    assert np.array_equal(p, g[name + "_p"]) and np.array_equal(nxt, g[name + "_next"])
    rs = np.random.RandomState(seed)
    assert ml._stream(rs) is rs
    assert np.array_equal(rs.choice(nn, nm, replace=False), g[name + "_p"]) and np.array_equal(rs.randint(0, 2 ** 31 - 1, size=4), g[name + "_next"])
    own = ml._stream(seed)
    assert isinstance(own, np.random.RandomState)
    assert np.array_equal(own.choice(nn, nm, replace=False), g[name + "_p"]) and np.array_equal(own.randint(0, 2 ** 31 - 1, size=4), g[name + "_next"])
    for bad in (np.random.default_rng(0), None, True, 1.5):
        with pytest.raises(TypeError):
            ml._stream(bad)


def test_validate_cov_matrix_bit_for_bit(g):
    """the reference's validate_cov_matrix on its own input -> output pairs: A (no eigendecomposition), B and D (three rounds each) and an
    indefinite 24 x 24 matrix (one round), bit for bit.

    Case C (d = 144, three rounds) is held to the structure only: the reference's shift is -min(v) k^2 with v the eigenVECTOR matrix of
    np.linalg.eig, and above n = 128 LAPACK reduces to Hessenberg form with blocked code on threaded level-3 BLAS, so the eigenvectors --
    their signs and normalisation, hence min(v) -- depend on the number of BLAS threads: the recorded diagonal of C starts 5.2026 (8
    threads), one thread gives 5.2065.  Its output must be the symmetrised input plus one non-negative multiple of the identity, and
    positive definite."""
    from ssg_amd.metric_learning import validate_cov_matrix
    for name in ("A", "B", "D"):
        M_in = g[name + "_val_in"].copy()
        out = validate_cov_matrix(M_in)
        assert out.dtype == np.float64 and np.array_equal(out, g[name + "_M"]), name
        assert np.array_equal(M_in, g[name + "_val_in"])                          # the caller's matrix is left alone
        np.linalg.cholesky(out)
    assert [int(g[n + "_eig_rounds"]) for n in "ABCD"] == [0, 3, 3, 3] and int(g["extra_eig_rounds"]) == 1
    assert np.array_equal(validate_cov_matrix(g["extra_val_in"]), g["extra_val_out"])
    M_in = g["C_val_in"]
    sym = (M_in + M_in.T) * 0.5
    for out in (validate_cov_matrix(M_in), g["C_M"]):
        off = ~np.eye(144, dtype=bool)
        assert np.array_equal(out[off], sym[off])
        shift = np.diag(out) - np.diag(sym)
        assert shift.min() > 0 and shift.max() - shift.min() <= 8 * np.spacing(np.abs(np.diag(out)).max())
        np.linalg.cholesky(out)
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(sym)


def test_restatement_is_the_references_fit_to_float32_accuracy(g):
    """the reference multiplies float32 differences; the float64 restatement agrees with its M (before validation) to the 1e-5 relative
    error of that route -- a check of the restatement, not a bound the device is held to"""
    for name in sorted(kr.CASES):
        X, y = kr.make_case(name)
        r = kr.fit64(X, y, g[name + "_p"])
        ref = g[name + "_val_in"]
        assert np.linalg.norm(r["M_raw"] - ref) <= 1e-4 * np.linalg.norm(ref), name


def test_factory_names_and_errors():
    import ssg_amd
    from ssg_amd import metric_learning as ml
    from ssg_amd.dist_metric import DistanceMetric
    assert ssg_amd.get_metric is ml.get_metric and ssg_amd.DistanceMetric is DistanceMetric
    assert ssg_amd.KISSME is ml.KISSME and ssg_amd.Euclidean is ml.Euclidean and ssg_amd.validate_cov_matrix is ml.validate_cov_matrix
    assert isinstance(ml.get_metric("euclidean"), ml.Euclidean) and isinstance(ml.get_metric("kissme"), ml.KISSME)
    with pytest.raises(KeyError) as e:
        ml.get_metric("mahalanobis")
    assert e.value.args == ("Unknown metric:", "mahalanobis")
    for name in ("itml", "lmnn", "lsml", "sdml", "nca", "lfda", "rca"):
        with pytest.raises(KeyError, match="metric_learn"):
            ml.get_metric(name)
    eu = ml.get_metric("euclidean")
    X = np.arange(12, dtype=np.float32).reshape(4, 3)
    eu.fit(X)
    assert np.array_equal(eu.metric(), np.eye(3)) and eu.transform() is X and eu.transform(X[:2]) is not None and np.array_equal(eu.transform(X[:2]), X[:2])
    dm = DistanceMetric()
    assert dm.algorithm == "euclidean" and isinstance(dm.metric, ml.Euclidean) and dm.train(None, None) is None
    assert dm.transform(X) is X
    assert isinstance(DistanceMetric("kissme").metric, ml.KISSME) and DistanceMetric("kissme").metric.metric() is None
    with pytest.raises(KeyError):
        DistanceMetric("nope")
    k = ml.KISSME()
    with pytest.raises(ValueError, match="fit first"):
        k.transform(X)
    with pytest.raises(TypeError):
        k.fit(X, np.zeros(4), rng=np.random.default_rng(0))
    with pytest.raises(ValueError, match="no matching pair"):
        k.fit(X, None)


def test_entry_points_refuse_bad_arguments_without_gpu():
    from ssg_amd import _lib
    L = _lib.lib()
    ws = ctypes.cast(ctypes.create_string_buffer(1 << 12), ctypes.c_void_p)
    for n, G in ((0, 1), (-4, 1), ((1 << 24) + 1, 2), (10, 0), (10, 11)):
        assert L.ssg_kissme_index(ws, n, G, ws, ws, ws, ws, ws, None) == -1 and b"ssg_kissme_index" in L.ssg_last_error()
        assert L.ssg_kissme_match_pairs(ws, ws, ws, ws, ws, n, G, 1, ws, ws, None) == -1 and b"ssg_kissme_match_pairs" in L.ssg_last_error()
        assert L.ssg_kissme_unrank(ws, 1, ws, ws, ws, ws, ws, n, G, ws, ws, None) == -1 and b"ssg_kissme_unrank" in L.ssg_last_error()
    assert L.ssg_kissme_index(None, 10, 2, ws, ws, ws, ws, ws, None) == -1 and b"NULL" in L.ssg_last_error()
    assert L.ssg_kissme_index(ws, 10, 2, ws, ws, ws, ws, None, None) == -1
    assert L.ssg_kissme_match_pairs(ws, ws, ws, ws, ws, 10, 2, 0, ws, ws, None) == -1 and b"P1=0" in L.ssg_last_error()
    assert L.ssg_kissme_match_pairs(ws, ws, ws, ws, ws, 10, 2, 46, ws, ws, None) == -1                 # 10 rows have 45 pairs
    assert L.ssg_kissme_match_pairs(ws, ws, ws, ws, ws, 10, 2, 45, ws, None, None) == -1 and b"NULL" in L.ssg_last_error()
    assert L.ssg_kissme_unrank(ws, 0, ws, ws, ws, ws, ws, 10, 2, ws, ws, None) == -1 and b"T=0" in L.ssg_last_error()
    assert L.ssg_kissme_unrank(None, 5, ws, ws, ws, ws, ws, 10, 2, ws, ws, None) == -1 and b"NULL" in L.ssg_last_error()
    for n, ldx, P, d, div in ((0, 32, 5, 32, 5.0), (10, 32, 0, 32, 5.0), (10, 40, 5, 40, 5.0),       # n, P, d % 16
                              (10, 8, 5, 8, 5.0), (10, 16400, 5, 16400, 5.0),                        # d < 16, d > 16384
                              (10, 16, 5, 32, 5.0), (10, 34, 5, 32, 5.0),                            # ldx < d, ldx % 4
                              (10, 32, 5, 32, 0.0), (10, 32, 5, 32, -1.0), (10, 32, 5, 32, float("nan"))):
        assert L.ssg_pairdiff_cov_f64(ws, n, ldx, ws, ws, P, d, div, ws, None) == -1, (n, ldx, P, d, div)
        assert b"ssg_pairdiff_cov_f64" in L.ssg_last_error()
    assert L.ssg_pairdiff_cov_f64(None, 10, 32, ws, ws, 5, 32, 5.0, ws, None) == -1 and b"NULL" in L.ssg_last_error()
    assert L.ssg_pairdiff_cov_f64(ctypes.c_void_p(ws.value + 4), 10, 32, ws, ws, 5, 32, 5.0, ws, None) == -1 and b"aligned" in L.ssg_last_error()
