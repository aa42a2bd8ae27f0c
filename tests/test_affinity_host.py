"""CPU checks of the affinity propagation path: the numpy restatement tests/affinity_ref.py against sklearn 1.7.2's recorded results
(tests/golden/affinity_cases.npz) and against sklearn itself where it is installed, the column-sum order it rests on, and what
ssg_amd.cluster.AffinityPropagation decides before it touches the device."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affinity_ref as ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "affinity_cases.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("name", list(ref.CASES))
def test_restatement_equals_golden(gold, name):
    r = ref.case_result(name)
    assert r["n_iter"] == int(gold[name + "_n_iter"])
    assert np.array_equal(r["centers"], gold[name + "_centers"])
    assert np.array_equal(r["labels"], gold[name + "_labels"])
    assert [ref.sha(r["A"]), ref.sha(r["R"]), ref.sha(r["S"])] == list(gold[name + "_sha"])
    if ref.EXPECTED.get(name) is not None:
        assert (r["n_iter"], len(r["centers"])) == ref.EXPECTED[name]


@pytest.mark.parametrize("name", ["a", "a_seed5", "c", "f", "g", "h1", "h2", "h16"])
def test_restatement_equals_sklearn(name):
    cluster = pytest.importorskip("sklearn.cluster")
    X = ref.case_input(ref.CASES[name][0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk = cluster.AffinityPropagation(affinity="precomputed", **ref.case_kwargs(name)).fit(X.copy())
    r = ref.case_result(name)
    assert sk.n_iter_ == r["n_iter"]
    assert np.array_equal(np.asarray(sk.cluster_centers_indices_, dtype=np.int64), r["centers"])
    assert np.array_equal(sk.labels_, r["labels"])
    assert ref.sha(sk.affinity_matrix_) == ref.sha(r["S"])


def test_numpy_column_sum_adds_rows_in_order():
    rng = np.random.default_rng(0)
    T = rng.standard_normal((700, 700)) * 10.0 ** rng.integers(-8, 8, (700, 700))
    assert np.array_equal(np.sum(T, axis=0), ref.colsum_seq(T))
    ii = np.sort(rng.choice(700, 333, replace=False))
    sub = T[ii[:, None], ii]                           # the fancy-indexed sub-matrix of the exemplar refinement
    assert np.array_equal(np.sum(sub, axis=0), ref.colsum_seq(sub))
    # and the order matters: another one gives other bits on this matrix
    assert not np.array_equal(ref.colsum_seq(T[::-1]), ref.colsum_seq(T))


def test_exports():
    import ssg_amd
    from ssg_amd import cluster, selftraining
    assert ssg_amd.AffinityPropagation is cluster.AffinityPropagation
    assert ssg_amd.generate_selflabel_affinity is selftraining.generate_selflabel_affinity
    assert issubclass(cluster.ConvergenceWarning, UserWarning)
    try:
        from sklearn.exceptions import ConvergenceWarning
    except ImportError:
        return
    assert cluster.ConvergenceWarning is ConvergenceWarning


def test_constructor_matches_sklearn():
    import inspect
    from ssg_amd.cluster import AffinityPropagation
    est = AffinityPropagation()
    want = dict(damping=0.5, max_iter=200, convergence_iter=15, copy=True, preference=None, affinity="euclidean", verbose=False, random_state=None)
    for k, v in want.items():
        assert getattr(est, k) == v or (v is None and getattr(est, k) is None)
    params = inspect.signature(AffinityPropagation.__init__).parameters
    assert list(params)[1:9] == list(want)
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in params.items() if n != "self")
    assert 8 <= params["poll_every"].default <= 32


@pytest.mark.parametrize("kw, word", [
    (dict(damping=0.49), "damping"), (dict(damping=1.0), "damping"), (dict(damping="x"), "damping"),
    (dict(max_iter=0), "max_iter"), (dict(max_iter=2.5), "max_iter"), (dict(convergence_iter=0), "convergence_iter"),
    (dict(copy=1), "copy"), (dict(poll_every=0), "poll_every"),
])
def test_parameter_validation(kw, word):
    from ssg_amd.cluster import AffinityPropagation
    args = dict(affinity="precomputed")
    args.update(kw)
    with pytest.raises(ValueError, match="The '%s' parameter of AffinityPropagation must be" % word):
        AffinityPropagation(**args).fit(np.zeros((3, 3)))


def test_affinity_other_than_precomputed_raises():
    from ssg_amd.cluster import AffinityPropagation
    for aff in ("euclidean", "cosine"):
        with pytest.raises(ValueError, match="implements affinity='precomputed' only"):
            AffinityPropagation(affinity=aff).fit(np.zeros((3, 3)))


def test_bad_random_state_raises():
    from ssg_amd.cluster import AffinityPropagation
    with pytest.raises(ValueError, match="cannot be used to seed"):
        AffinityPropagation(affinity="precomputed", random_state="seed").fit(np.zeros((3, 3)))


def test_distance_handle_is_refused():
    torch = pytest.importorskip("torch")
    from ssg_amd.cluster import AffinityPropagation
    from ssg_amd.rerank import DistHandle
    h = DistHandle(4, 2, torch.zeros((4, 4), dtype=torch.float64))
    with pytest.raises(TypeError, match=r"pass -h\.final_dist\(\)"):
        AffinityPropagation(affinity="precomputed").fit(h)
    sharded = DistHandle(4, 2, torch.zeros((2, 4), dtype=torch.float64), row0=0, nrows=2, group=object())
    with pytest.raises(ValueError, match="single GPU"):
        AffinityPropagation(affinity="precomputed").fit(sharded)


def test_shape_is_checked_before_the_device_is_touched():
    from ssg_amd.cluster import AffinityPropagation
    with pytest.raises(ValueError, match="must be a square array"):
        AffinityPropagation(affinity="precomputed").fit(np.zeros((3, 4)))
    with pytest.raises(ValueError, match="Expected 2D array"):
        AffinityPropagation(affinity="precomputed").fit(np.zeros(3))
