"""CPU suite for the SSG++ label step (ssg_amd.eug, ssg_amd.semitraining): the host-only mirrors against the reference's own
outputs (tests/golden/eug_cases.npz, tools/make_golden_eug.py) and the argument checks of the new C entry points."""
import os
import types

import numpy as np
import pytest

import ssg_amd
from ssg_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eug_cases.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def fake_dataset(g):
    trainval = [(str(f), int(f[:4]), int(f[6])) for f in g["upd_trainval"]]
    return types.SimpleNamespace(images_dir="/data/market/images", trainval=trainval)


@pytest.mark.parametrize("sample", ["random", "cluster"])
@pytest.mark.parametrize("seed", [0, 3])
def test_updata_lable_matches_reference_golden(g, tmp_path, sample, seed):
    from ssg_amd.eug import updata_lable
    ds = fake_dataset(g)
    np.random.seed(12345)          # the split depends on the seed argument alone
    unl, lbl = updata_lable(ds, g["upd_label"], "fake", sample=sample, load_path=str(tmp_path) + "/", seed=seed)
    tag = "%s_%d" % (sample, seed)
    assert [f for f, _, _ in lbl] == list(g["upd_l_fnames_" + tag])
    assert [p for _, p, _ in lbl] == list(g["upd_l_pid_" + tag]) and [c for _, _, c in lbl] == list(g["upd_l_cam_" + tag])
    assert [f for f, _, _ in unl] == list(g["upd_u_fnames_" + tag])
    assert os.path.exists(str(tmp_path / ("%s_fake.pkl" % sample)))
    unl2, lbl2 = updata_lable(ds, g["upd_label"], "fake", sample=sample, load_path=str(tmp_path) + "/", seed=seed + 1)
    assert unl2 == unl and lbl2 == lbl                  # a cached split is read back, whatever the seed


def test_updata_lable_rejects_unknown_sampler(g, tmp_path):
    from ssg_amd.eug import updata_lable
    with pytest.raises(ValueError):
        updata_lable(fake_dataset(g), g["upd_label"], "fake", sample="nearest", load_path=str(tmp_path) + "/")


def test_generate_new_train_data_matches_reference_golden(g, capsys):
    from ssg_amd.eug import EUGMixin
    nl, per_id = int(g["nl"]), int(g["per_id"])
    ids = np.arange(nl * per_id) % nl
    eug = EUGMixin()
    eug.u_label, eug.l_label = ids[nl:], ids[:nl]
    eug.u_data = [["u_%04d.jpg" % i, int(p), i % 6] for i, p in enumerate(eug.u_label)]
    eug.l_data = [["l_%04d.jpg" % i, int(p), 1.0] for i, p in enumerate(eug.l_label)]
    new = eug.generate_new_train_data(g["gen_sel"], g["gen_pred"])
    assert [f for f, _, _ in new] == list(g["gen_fnames"])
    assert [p for _, p, _ in new] == list(g["gen_labels"]) and all(type(p) is int for _, p, _ in new[nl:])
    assert [float(c) for _, _, c in new] == list(g["gen_third"])
    assert "selected pseudo-labeled data: " in capsys.readouterr().out


def test_classification_mode_is_refused():
    from ssg_amd.eug import EUGMixin
    eug = EUGMixin()
    eug.mode = "Classification"
    with pytest.raises(NotImplementedError, match="num_class"):
        eug.estimate_label()
    with pytest.raises(NotImplementedError):
        eug.get_Classification_result()


def test_semitraining_generate_selflabel_start_epoch_rule(monkeypatch):
    """semitraining.py:327: the eps rule runs at n_iter == args.start_epoch (not at 0); other iterations reuse the cached
    estimators.  selftraining's rule (iteration 0) is unchanged."""
    from ssg_amd import semitraining, selftraining
    calls = []

    def fake_chain(dist, rho, min_samples=4):
        calls.append(("eps", dist, rho))
        return 0.25, 10, 3, np.array([0, 0, 1, -1]), np.array([0, 1])
    monkeypatch.setattr(semitraining, "eps_rule_dbscan", fake_chain)

    class Cached:
        def __init__(self, tag):
            self.tag = tag

        def fit_predict(self, dist):
            calls.append(("fit", self.tag, dist))
            return np.array([2, 2, -1, 5])

    args = types.SimpleNamespace(no_rerank=False, rho=1.6e-3, start_epoch=3)
    cache = []
    labels, cache = semitraining.generate_selflabel(["e0", "e1"], ["r0", "r1"], 3, args, cache)
    assert [c[:2] for c in calls] == [("eps", "r0"), ("eps", "r1")] and len(cache) == 2
    assert cache[0].eps == 0.25 and np.array_equal(labels[0], [0, 0, 1, -1])
    assert all(type(c).__name__ == "DBSCAN" and c.min_samples == 4 for c in cache)
    calls.clear()
    cache[:] = [Cached("a"), Cached("b")]               # (the cached estimators' own fit runs on the GPU)
    labels, cache2 = semitraining.generate_selflabel(["e0", "e1"], ["r0", "r1"], 4, args, cache)
    assert cache2 is cache and len(cache) == 2
    assert calls == [("fit", "a", "r0"), ("fit", "b", "r1")] and np.array_equal(labels[1], [2, 2, -1, 5])
    calls.clear()
    cached = [Cached("a")]                               # iteration 0 of a resumed run is not the start epoch: no eps rule
    semitraining.generate_selflabel(["e0"], ["r0"], 0, types.SimpleNamespace(no_rerank=True, rho=1e-3, start_epoch=2), cached)
    assert calls == [("fit", "a", "e0")]
    assert selftraining.generate_selflabel is not semitraining.generate_selflabel
    assert ssg_amd.generate_selflabel_semi is semitraining.generate_selflabel


def test_eug_entry_points_validate_arguments_without_gpu():
    L = _lib.lib()
    assert L.ssg_eug_nn_splits(12185, 751) >= 1
    assert L.ssg_eug_nn_f32(None, 10, None, 4, 40000, None, 1, None, None, None, None, None, None, None) == -1      # d > 32768
    assert b"d <=" in L.ssg_last_error()
    assert L.ssg_eug_nn_f32(None, 10, None, 4, 64, None, 7, None, None, None, None, None, None, None) == -1         # wrong nsplit
    assert L.ssg_eug_dist_label_f32(None, 0, 4, None, None, None, None, None, None, None) == -1
    assert L.ssg_eug_select_top(None, 10, 11, None, None, None) == -1 and b"k <= n" in L.ssg_last_error()
    assert L.ssg_eug_select_top(None, 10, -1, None, None, None) == -1
