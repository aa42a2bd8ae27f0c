"""Records tests/golden/kissme_cases.npz from the untouched reference:  python tools/make_golden_kissme.py /path/to/reference

The reference's reid/metric_learning/kissme.py is loaded from its file with a stub `metric_learn.base_metric.BaseMetricLearner` of our own
in sys.modules (the library is not installed).  Its `fit` runs on every case of tests/kissme_ref.py under np.random.seed(FIT_SEED); what
it does inside is observed from outside, nothing of it is restated here:
    the four row gathers X[idx]        through an ndarray subclass that notes every index array it is asked for  -> ia1, ib1, ia0, ib0
    np.random.choice                   wrapped for the length of the call                                        -> p
    validate_cov_matrix                the module's global is wrapped: its argument and its return value          -> val_in, M
    np.linalg.eig                      counted: the rounds of the validate loop
and the stream's next draw after `fit`.  One more validate pair comes from an indefinite symmetric 24 x 24 matrix, so that the loop is
recorded whatever the cases do."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kissme_ref  # noqa: E402


def load_reference(path):
    ml = types.ModuleType("metric_learn"); base = types.ModuleType("metric_learn.base_metric")

    class BaseMetricLearner(object):
        pass
    base.BaseMetricLearner = BaseMetricLearner
    ml.base_metric = base
    sys.modules["metric_learn"] = ml; sys.modules["metric_learn.base_metric"] = base
    spec = importlib.util.spec_from_file_location("reference_kissme", os.path.join(path, "reid", "metric_learning", "kissme.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Noting(np.ndarray):
    """an array that notes the index arrays it is gathered with"""
    asked = None

    def __getitem__(self, key):
        if isinstance(key, np.ndarray) and key.ndim == 1 and self.ndim == 2:
            self.asked.append(np.array(key))
            return np.asarray(self)[key]
        return np.asarray(self).__getitem__(key)


def observe(mod, fn):
    """run fn() with choice / validate_cov_matrix / eig of the reference's module watched -> dict"""
    seen = {"eig": 0}
    choice, validate, eig = np.random.choice, mod.validate_cov_matrix, np.linalg.eig

    def w_choice(*a, **k):
        seen["p"] = choice(*a, **k)
        return seen["p"]

    def w_validate(M):
        seen["val_in"] = np.array(M)
        out = validate(M)
        seen["val_out"] = np.array(out)
        return out

    def w_eig(*a, **k):
        seen["eig"] += 1
        return eig(*a, **k)
    np.random.choice, mod.validate_cov_matrix, np.linalg.eig = w_choice, w_validate, w_eig
    try:
        fn()
    finally:
        np.random.choice, mod.validate_cov_matrix, np.linalg.eig = choice, validate, eig
    return seen


def main(reference):
    mod = load_reference(reference)
    out = {"names": np.array(sorted(kissme_ref.CASES))}
    for name in sorted(kissme_ref.CASES):
        X, y = kissme_ref.make_case(name)
        seed = kissme_ref.FIT_SEED[name]
        Xn = X.view(Noting); Xn.asked = []
        learner = mod.KISSME()
        np.random.seed(seed)
        seen = observe(mod, lambda: learner.fit(Xn, y))
        nxt = np.random.randint(0, 2 ** 31 - 1, size=4)
        ia1, ib1, ia0, ib0 = Xn.asked
        assert learner.M_.dtype == np.float64 and np.array_equal(learner.M_, seen["val_out"])
        print("%s: n=%d d=%d P=%d non-matching=%d, validate loop: %d eig calls" %
              (name, X.shape[0], X.shape[1], ia1.shape[0], X.shape[0] * (X.shape[0] - 1) // 2 - ia1.shape[0], seen["eig"]))
        for k, v in (("X", X), ("y", y), ("seed", np.int64(seed)), ("ia1", ia1.astype(np.int32)), ("ib1", ib1.astype(np.int32)),
                     ("p", np.asarray(seen["p"]).astype(np.int64)), ("ia0", ia0.astype(np.int32)), ("ib0", ib0.astype(np.int32)),
                     ("next", nxt.astype(np.int64)), ("val_in", seen["val_in"]), ("M", learner.M_), ("eig_rounds", np.int64(seen["eig"]))):
            out["%s_%s" % (name, k)] = v
    rs = np.random.RandomState(7)
    Q, _ = np.linalg.qr(rs.standard_normal((24, 24)))
    sym = (Q * np.linspace(-0.5, 3.0, 24)).dot(Q.T)              # eigenvalues from -0.5 to 3: not positive definite
    seen = observe(mod, lambda: mod.validate_cov_matrix(sym))
    assert seen["eig"] >= 1
    print("extra validate pair: %d eig calls" % seen["eig"])
    out["extra_val_in"], out["extra_val_out"], out["extra_eig_rounds"] = sym, seen["val_out"], np.int64(seen["eig"])
    path = os.path.join(ROOT, "tests", "golden", "kissme_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])
