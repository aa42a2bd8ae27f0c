"""GPU suite for the SSG++ label step (csrc/eug.hip behind ssg_amd.eug) against the reference's own reid/eug.py outputs
(tests/golden/eug_cases.npz, written by tools/make_golden_eug.py) and against numpy at Market-1501 scale."""
import os

import numpy as np
import pytest
import torch

import ssg_amd
from synth import clustered

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eug_cases.npz")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def case(g, d):
    """the features of the golden case of width d (regenerated, checked against the recorded sha256)"""
    import hashlib
    nl, per_id = int(g["nl"]), int(g["per_id"])
    x = clustered(nl * per_id, d, int(g["seed_%d" % d]), per_id=per_id)
    assert hashlib.sha256(x.tobytes()).hexdigest() == str(g["sha_%d" % d]), "synth.clustered no longer reproduces the fixture"
    ids = np.arange(x.shape[0]) % nl
    return x[nl:], x[:nl], ids[nl:], ids[:nl]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def test_dist_label_crafted_matrices_bit_identical(g, dev):
    from ssg_amd.eug import dissimilarity_from_dist
    for name in g["crafted"]:
        M = g["crafted_dist_" + name]
        lab, sc, conf = dissimilarity_from_dist(torch.from_numpy(M).to(dev), g["crafted_l_label"])
        assert lab.dtype == sc.dtype == conf.dtype == np.float64
        assert same_bits(lab, g["crafted_labels_" + name]), name
        assert same_bits(sc, g["crafted_scores_" + name]), name
        assert same_bits(conf, g["crafted_conf_" + name]), name
        lab2, sc2, conf2 = dissimilarity_from_dist(M, g["crafted_l_label"])          # numpy input
        assert same_bits(conf2, conf) and same_bits(lab2, lab) and same_bits(sc2, sc)


@pytest.mark.parametrize("d", [64, 2048, 6144, 8200])
def test_dist_label_reference_rerank_matrices_bit_identical(g, dev, d):
    from ssg_amd.eug import dissimilarity_from_dist
    _, _, _, ll = case(g, d)
    lab, sc, conf = dissimilarity_from_dist(g["rr_dist_%d" % d], ll)
    assert same_bits(lab, g["rr_labels_%d" % d]) and same_bits(sc, g["rr_scores_%d" % d]) and same_bits(conf, g["rr_conf_%d" % d])


@pytest.mark.parametrize("d", [64, 2048, 6144, 8200])
def test_nearest_labelled_bit_identical(g, dev, d):
    """rerank=False: np.linalg.norm(l - u, axis=1) + argmin, bit for bit (8200: numpy's 8192-element chunks)"""
    from ssg_amd.eug import estimate_label_device
    u, l, _, ll = case(g, d)
    lab, sc = estimate_label_device(torch.from_numpy(u).to(dev), torch.from_numpy(l).to(dev), ll, rerank=False, weight=True)
    assert same_bits(lab, g["nn_labels_%d" % d]) and same_bits(sc, g["nn_scores_%d" % d])


@pytest.mark.parametrize("d", [64, 2048, 6144, 8200])
def test_rerank_chain_vs_reference(g, dev, d):
    """rerank=True end to end on the device (re_ranking_init -> kernel b).  np.dot / np.exp are not reproducible bit for bit, so
    scores within 2e-5 (test_re_ranking_init_vs_reference_golden's bound), labels equal on every such row whose reference
    min-vs-second gap exceeds 1e-4, confidence within 1e-4.  A near-tie in the top-(k1+1) ranking (distances within float32
    rounding of each other) can give a row another k-reciprocal set and move its score by far more than that: at d = 6144 one row
    of the 168 does, so up to 2 % of the rows may fall outside the score and confidence bounds."""
    from ssg_amd.eug import estimate_label_device
    u, l, _, ll = case(g, d)
    lab, sc, conf = estimate_label_device(torch.from_numpy(u).to(dev), torch.from_numpy(l).to(dev), ll, rerank=True, weight=True)
    close = np.abs(sc - g["rr_scores_%d" % d]) < 2e-5
    assert close.mean() >= 0.98, np.flatnonzero(~close)
    clear = close & (g["rr_gap_%d" % d] > 1e-4)
    assert clear.mean() > 0.5 and np.array_equal(lab[clear], g["rr_labels_%d" % d][clear])
    assert (np.abs(conf - g["rr_conf_%d" % d]) < 1e-4).mean() >= 0.98
    lab2, sc2 = estimate_label_device(u, l, ll, rerank=True)                           # numpy features, no confidence
    assert np.array_equal(lab2, lab) and np.array_equal(sc2, sc)


def test_select_top_reference_golden(g, dev):
    from ssg_amd.eug import select_top
    for i, k in enumerate(g["sel_k"]):
        assert np.array_equal(select_top(g["sel_scores"], int(k)), g["sel_masks"][i]), k
        assert np.array_equal(select_top(g["sel_scores"], int(k), labels=g["sel_labels"]), g["sel_true_masks"][i]), k


def test_select_top_tie_rule(dev):
    """ties that straddle the cut go to the lowest indices == the first k of a STABLE argsort of -scores (NaN last, -0 == +0);
    up to 128 000 entries"""
    from ssg_amd.eug import select_top
    s = np.array([0.5, 0.9, 0.5, -0.0, 0.9, 0.5, np.nan, 0.0, 0.5, 0.9])
    assert np.flatnonzero(select_top(s, 5)).tolist() == [0, 1, 2, 4, 9]
    assert np.flatnonzero(select_top(s, 8)).tolist() == [0, 1, 2, 3, 4, 5, 8, 9]
    assert np.flatnonzero(select_top(s, 9)).tolist() == [0, 1, 2, 3, 4, 5, 7, 8, 9]
    assert select_top(s, 10).all() and not select_top(s, 0).any()
    assert np.flatnonzero(select_top(s, 5, labels=[0, -1, 3, 3, 3, 3, 3, 3, 3, 3])).tolist() == [0, 2, 4, 9]
    rng = np.random.default_rng(5)
    for n in (1, 1000, 12185, 128000):
        for vals in (rng.integers(0, 7, n) / 8.0, -rng.random(n), np.where(rng.random(n) < 0.01, np.nan, rng.integers(-3, 3, n) * 1e300)):
            for k in (0, 1, n // 3, n // 2 + 1, n):
                ref = np.zeros(n, bool); ref[np.argsort(-vals, kind="stable")[:k]] = True
                assert np.array_equal(select_top(torch.from_numpy(vals).to(dev), k), ref), (n, k)
    with pytest.raises(ValueError):
        select_top(s, 11)


def test_market_scale(dev):
    """Nu = 12 185, Nl = 751, d = 6144 (Market-1501, num_split = 2): kernel a exactly against numpy on 256 sampled rows, kernel b
    against numpy's argmin / column max on the re-rank matrix the device chain returns"""
    from ssg_amd.eug import dissimilarity_from_dist, nearest_labelled
    from ssg_amd.rerank import re_ranking_init_device
    nu, nl, d = 12185, 751, 6144
    gen = torch.Generator(device=dev).manual_seed(11)
    c = torch.nn.functional.normalize(torch.randn(nl, d, device=dev, generator=gen), dim=1)
    pid = torch.randint(0, nl, (nu,), device=dev, generator=gen)
    u = torch.nn.functional.normalize(c[pid] + 0.6 * torch.randn(nu, d, device=dev, generator=gen) / d ** 0.5, dim=1)
    lf = torch.nn.functional.normalize(c + 0.6 * torch.randn(nl, d, device=dev, generator=gen) / d ** 0.5, dim=1)
    l_label = np.arange(nl) * 3 + 7
    labels, scores, argmin, minval = nearest_labelled(u, lf, l_label)
    torch.cuda.synchronize()
    rows = np.random.default_rng(3).choice(nu, 256, replace=False)
    un, ln = u[torch.from_numpy(rows).to(dev)].cpu().numpy(), lf.cpu().numpy()
    am, mv = argmin.cpu().numpy(), minval.cpu().numpy()
    lab, sc = labels.cpu().numpy(), scores.cpu().numpy()
    for r, i in enumerate(rows):
        dist = np.linalg.norm(ln - un[r], axis=1)
        j = np.argmin(dist)
        assert am[i] == j and mv[i].view(np.uint32) == dist[j].view(np.uint32), i
        assert lab[i] == l_label[j] and sc[i] == -dist[j]
    D = re_ranking_init_device(u, lf)
    assert D.shape == (nu, nl) and D.is_cuda
    lab_b, sc_b, conf_b, am_b = dissimilarity_from_dist(D, l_label, return_argmin=True)
    Dh = D.cpu().numpy()
    ja = np.argmin(Dh, axis=1)
    mins = Dh[np.arange(nu), ja]
    assert np.array_equal(am_b, ja) and np.array_equal(lab_b, l_label[ja].astype(np.float64))
    assert np.array_equal(sc_b, (-mins).astype(np.float64))
    assert same_bits(conf_b, (np.float32(1) - mins / np.max(Dh, axis=0)[ja]).astype(np.float64))


def test_eug_mixin_end_to_end(dev, capsys):
    """EUGMixin over a stand-in of reid/eug.py's EUG (the attributes its __init__ sets, a get_dataloader): an ssg_amd ResNet with
    synthetic weights, TensorBatchLoader loaders; checked against numpy on the same (device) features"""
    from ssg_amd.eug import EUGMixin
    from ssg_amd.evaluators import TensorBatchLoader, extract_embeddings
    nu, nl = 40, 8
    imgs = torch.randn(nu + nl, 3, 256, 128, generator=torch.Generator().manual_seed(4))
    model = ssg_amd.create("resnet50", num_classes=0, num_split=1, cluster=False, seed=1).cuda().eval()

    class RefEUG(object):                                 # what EUG.__init__ (eug.py:22-57) and get_dataloader provide
        def __init__(self, mode, rerank):
            self.mode, self.rerank, self.model = mode, rerank, model
            self.u_data = [["u_%d.jpg" % i, i % nl, 0] for i in range(nu)]
            self.l_data = [["l_%d.jpg" % i, i, 1.0] for i in range(nl)]
            self.u_label = np.array([p for _, p, _ in self.u_data]); self.l_label = np.array([p for _, p, _ in self.l_data])

        def get_dataloader(self, dataset, training=False):
            assert not training
            x = imgs[:nu] if dataset is self.u_data else imgs[nu:]
            return TensorBatchLoader(x, batch_size=16, fnames=[f for f, _, _ in dataset], pids=[p for _, p, _ in dataset])

    class EUG(EUGMixin, RefEUG):
        pass

    u = extract_embeddings(model, TensorBatchLoader(imgs[:nu], 16), for_eval=True)[0].cpu().numpy()
    l = extract_embeddings(model, TensorBatchLoader(imgs[nu:], 16), for_eval=True)[0].cpu().numpy()
    assert u.shape == (nu, 2048)
    eug = EUG("Dissimilarity", False)
    lab, sc = eug.estimate_label()
    ref_idx = [int(np.argmin(np.linalg.norm(l - x, axis=1))) for x in u]
    ref_sc = np.array([-np.linalg.norm(l - x, axis=1)[j] for x, j in zip(u, ref_idx)])
    assert lab.dtype == sc.dtype == np.float64
    assert np.array_equal(lab, eug.l_label[ref_idx].astype(np.float64)) and np.array_equal(sc, ref_sc)
    out = capsys.readouterr().out
    assert "label estimation by Dissimilarity mode." in out and "u_features (40, 2048) l_features (8, 2048)" in out
    assert "predictions on all the unlabeled data:" in out
    eug = EUG("Weight", True)
    lab, sc, conf = eug.estimate_label()
    ref = ssg_amd.re_ranking_init(u, l)
    assert np.abs(sc + ref.min(axis=1)).max() < 2e-5 and conf.dtype == np.float64 and np.all(conf <= 1)
    sel = eug.select_top_data(sc, 10)
    assert sel.dtype == bool and sel.sum() == 10 and np.array_equal(sel, np.isin(np.arange(nu), np.argsort(-sc, kind="stable")[:10]))
    new = eug.generate_new_train_data(sel, lab)
    assert len(new) == nl + 10 and new[:nl] == eug.l_data
    assert eug.select_top_true_data(np.where(np.arange(nu) % 2 == 0, -1.0, lab), sc, 10).sum() == (sel & (np.arange(nu) % 2 == 1)).sum()
    with pytest.raises(ValueError):
        EUG("Weight", False).estimate_label()
