#!/usr/bin/env python3
"""Generate tests/golden/eug_cases.npz from the reference's own reid/eug.py (SSG++ label step; run where the reference is).

The reference EUG class is imported under make_golden.import_reid()'s stub modules and built with EUG.__new__ (no model, no
loaders); get_feature is patched to return fixed synth.clustered features, so the reference's own get_Dissimilarity_result /
estimate_label loops run on them.  For crafted matrices (exact ties within a row, NaN entries, a zero column) reid.eug.re_ranking_init
is patched to return the matrix, so the reference's own argmin / column-max loop runs on it.  Also recorded: select_top_data /
select_top_true_data, generate_new_train_data and the updata_lable split of a fake dataset (written in a temp directory).

Features are not stored: the tests regenerate them from (N, d, seed) with tools/synth.py and check their sha256 against the one
recorded here.
"""
import hashlib
import os
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "eug_cases.npz")

import make_golden  # noqa: E402
from synth import clustered  # noqa: E402

NL, PER_ID = 24, 8        # one labelled image per identity; N = NL * PER_ID images per case


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def case_features(d, seed):
    """the features of one case: labelled = the first image of each identity, unlabelled = the rest (synth.clustered order)"""
    x = clustered(NL * PER_ID, d, seed, per_id=PER_ID)
    ids = np.arange(x.shape[0]) % NL
    return x[NL:], x[:NL], ids[NL:], ids[:NL], x


def make_eug(E, u_feas, l_feas, u_label, l_label, mode, rerank):
    eug = E.EUG.__new__(E.EUG)
    eug.mode, eug.rerank = mode, rerank
    eug.u_label, eug.l_label = np.asarray(u_label), np.asarray(l_label)
    eug.u_data = [["u_%04d.jpg" % i, int(p), i % 6] for i, p in enumerate(u_label)]
    eug.l_data = [["l_%04d.jpg" % i, int(p), 1.0] for i, p in enumerate(l_label)]
    feats = {id(eug.u_data): u_feas, id(eug.l_data): l_feas}
    eug.get_feature = lambda dataset: feats[id(dataset)]
    return eug


def main():
    make_golden.import_reid()
    import reid.eug as E
    E.print = lambda *a, **k: None
    real_init = E.re_ranking_init
    rec = {"nl": NL, "per_id": PER_ID}

    # ---- both branches of get_Dissimilarity_result on synthetic embeddings, four widths (8200: numpy's 8192-element chunks)
    widths = (64, 2048, 6144, 8200)
    rec["widths"] = np.array(widths)
    for d in widths:
        seed = 500 + d
        u, l, ul, ll, x = case_features(d, seed)
        rec["seed_%d" % d] = seed; rec["sha_%d" % d] = sha(x)
        lab, sc = make_eug(E, u, l, ul, ll, "Dissimilarity", False).estimate_label()
        rec["nn_labels_%d" % d], rec["nn_scores_%d" % d] = lab, sc
        seen = {}

        def recording(*a, **k):
            seen["D"] = real_init(*a, **k)
            return seen["D"]
        E.re_ranking_init = recording
        try:
            lab, sc, conf = make_eug(E, u, l, ul, ll, "Weight", True).estimate_label()
        finally:
            E.re_ranking_init = real_init
        rec["rr_dist_%d" % d] = seen["D"]
        rec["rr_labels_%d" % d], rec["rr_scores_%d" % d], rec["rr_conf_%d" % d] = lab, sc, conf
        lab2, sc2 = make_eug(E, u, l, ul, ll, "Dissimilarity", True).estimate_label()
        assert np.array_equal(lab, lab2) and np.array_equal(sc, sc2)
        D = seen["D"]
        srt = np.sort(D, axis=1)
        rec["rr_gap_%d" % d] = srt[:, 1] - srt[:, 0]
        print("d=%d: nn labels %d/%d correct, rerank labels %d/%d" % (d, int((rec["nn_labels_%d" % d] == ul).sum()), len(ul),
                                                                        int((lab == ul).sum()), len(ul)))

    # ---- crafted matrices through the reference's own loop (re_ranking_init patched)
    rng = np.random.default_rng(77)
    nu, nl = 150, 37
    crafted = {}
    crafted["ties"] = (rng.integers(0, 5, (nu, nl)) / 4.0).astype(np.float32)               # exact ties within every row
    m = rng.random((nu, nl)).astype(np.float32)
    m[5, [4, 30]] = np.nan                                                                   # NaN entries: the first NaN wins the argmin,
    m[9, [3, 8]] = np.nan                                                                    # and the columns holding one have NaN maxima
    m[40, 36] = np.nan
    crafted["nan"] = m
    z = (rng.integers(1, 9, (nu, nl)) / 8.0).astype(np.float32)
    z[:, 20] = 0.0                                                                           # a zero column: 0 / 0 confidence
    z[:, 11] = np.where(rng.random(nu) < 0.5, 0.0, z[:, 11])                                 # zero minima in a non-zero column: 1 - 0 / max
    crafted["zerocol"] = z
    crafted["neg"] = (rng.standard_normal((nu, nl)) * 0.3).astype(np.float32)              # negative entries and maxima
    rec["crafted"] = np.array(sorted(crafted))
    l_label = rng.permutation(1000)[:nl].astype(np.int64)
    u_label = rng.integers(0, 1000, nu)
    rec["crafted_l_label"] = l_label
    fu, fl = np.zeros((nu, 4), np.float32), np.zeros((nl, 4), np.float32)
    for name, M in crafted.items():
        E.re_ranking_init = lambda *a, **k: M      # noqa: B023
        try:
            lab, sc, conf = make_eug(E, fu, fl, u_label, l_label, "Weight", True).estimate_label()
        finally:
            E.re_ranking_init = real_init
        rec["crafted_dist_" + name] = M
        rec["crafted_labels_" + name], rec["crafted_scores_" + name], rec["crafted_conf_" + name] = lab, sc, conf
        print("crafted %s: %d NaN confidences" % (name, int(np.isnan(conf).sum())))

    # ---- select_top_data / select_top_true_data on tie-free scores
    eug = make_eug(E, fu, fl, u_label, l_label, "Dissimilarity", True)
    scores = -rng.random(1000)
    assert len(np.unique(scores)) == len(scores)
    ks = np.array([0, 1, 17, 500, 999, 1000])
    labels = rng.integers(-1, 5, 1000).astype(np.float64)
    rec["sel_scores"], rec["sel_labels"], rec["sel_k"] = scores, labels, ks
    rec["sel_masks"] = np.stack([eug.select_top_data(scores, int(k)) for k in ks])
    rec["sel_true_masks"] = np.stack([eug.select_top_true_data(labels, scores, int(k)) for k in ks])

    # ---- generate_new_train_data
    u, l, ul, ll, _ = case_features(64, 564)
    eug = make_eug(E, u, l, ul, ll, "Dissimilarity", False)
    pred = rec["nn_labels_64"]
    sel = eug.select_top_data(rec["nn_scores_64"], 100)
    new = eug.generate_new_train_data(sel, pred)
    rec["gen_sel"], rec["gen_pred"] = sel, pred
    rec["gen_fnames"] = np.array([f for f, _, _ in new]); rec["gen_labels"] = np.array([int(p) for _, p, _ in new])
    rec["gen_third"] = np.array([float(c) for _, _, c in new])

    # ---- updata_lable: the one-shot split of a fake dataset, both samplers, two seeds
    n = 300
    trainval = [("%04d_c%ds1_%06d.jpg" % (i // 6, i % 6, i), i // 6, i % 6) for i in range(n)]
    dataset = types.SimpleNamespace(images_dir="/data/market/images", trainval=trainval)
    lab = rng.integers(-1, 40, n)
    rec["upd_label"] = lab
    for sample in ("random", "cluster"):
        for seed in (0, 3):
            with tempfile.TemporaryDirectory() as tmp:
                unl, lbl = E.updata_lable(dataset, lab, "fake", sample=sample, load_path=tmp + "/", seed=seed)
                unl2, lbl2 = E.updata_lable(dataset, lab, "fake", sample=sample, load_path=tmp + "/", seed=seed)   # the cached split
                assert unl2 == unl and lbl2 == lbl
            tag = "%s_%d" % (sample, seed)
            rec["upd_l_fnames_" + tag] = np.array([f for f, _, _ in lbl])
            rec["upd_l_pid_" + tag] = np.array([p for _, p, _ in lbl]); rec["upd_l_cam_" + tag] = np.array([c for _, _, c in lbl])
            rec["upd_u_fnames_" + tag] = np.array([f for f, _, _ in unl])
            print("updata_lable %s: %d labelled, %d unlabelled" % (tag, len(lbl), len(unl)))
    rec["upd_trainval"] = np.array([f for f, _, _ in trainval])
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024.0))


if __name__ == "__main__":
    main()
