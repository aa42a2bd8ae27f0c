"""Numpy restatement of the verification protocol (reid/evaluation_metrics/eval_far_gar.py:61-202) for one process, written for the
tests of ssg_amd.verification / csrc/verify.hip.

Two modes of `find_metric_threshold`:
  ref32 -- the reference's arithmetic: per-row float32 `.sum()` added into float32 running sums, float32 average and deviation;
  exact -- the same per-row sums taken in float64.
Counts, minima, maxima, order statistics and the threshold counts (as a function of the thresholds) do not depend on the mode.
The caller's `dist` is never modified."""
import numpy as np

DEFAULT_FAR = (1e-2, 1e-3, 1e-4, 1e-5)


def clamp_sqrt(dist):
    """:110-111 on a copy: float32 in, float32 out"""
    s = np.array(dist, dtype=np.float32, copy=True)
    s[s <= 0] = 0.0
    return np.sqrt(s)


def masks(qry_label, ref_label):
    q = np.asarray(qry_label).reshape(-1, 1); r = np.asarray(ref_label).reshape(1, -1)
    intra = r == q
    return intra, ~intra


def threshold_counts(values, intra, thresholds):
    """values [m, n] as compared (float32 against float64 scalars: numpy compares in double) -> int64 arrays
    (intra >= t, inter < t, intra < t)"""
    pos, neg = values[intra], values[~intra]
    ge = np.array([int((pos >= t).sum()) for t in thresholds], dtype=np.int64)
    lt = np.array([int((neg < t).sum()) for t in thresholds], dtype=np.int64)
    below = np.array([int((pos < t).sum()) for t in thresholds], dtype=np.int64)
    return ge, lt, below


def cal_classification_error(qry_label, ref_label, threshold_l, dist):
    """:61-100 with dist given: compared as it is -> (pos_err_rate, neg_err_rate, pos_num, neg_num, log)"""
    intra, _ = masks(qry_label, ref_label)
    thr = [np.float64(t) for t in threshold_l]
    ge, lt, _ = threshold_counts(np.asarray(dist), intra, thr)
    pos_num, neg_num = int(intra.sum()), int((~intra).sum())
    log = 'pos pair num {}, neg pair num {}\n'.format(pos_num, neg_num)
    return ge.astype('float') / pos_num, lt.astype('float') / neg_num, pos_num, neg_num, log


def find_metric_threshold(qry_label, ref_label, dist, mode="exact", far=DEFAULT_FAR):
    """-> dict of everything the protocol computes, plus 'lines' (what it prints, split at newlines)"""
    assert mode in ("exact", "ref32")
    s = clamp_sqrt(dist)
    intra, inter = masks(qry_label, ref_label)
    acc = np.float32 if mode == "ref32" else np.float64
    out = {}
    for name, mask in (("intra", intra), ("inter", inter)):
        tot = acc(0); tot2 = acc(0); num = 0
        mn = None; mx = None
        for i in range(s.shape[0]):
            row = s[i][mask[i]]
            if row.size == 0:
                raise ValueError("query %d has no %s element" % (i, name))
            wide = row if mode == "ref32" else row.astype(np.float64)
            tot = acc(tot + wide.sum()); tot2 = acc(tot2 + (wide ** 2).sum()); num += row.size
            mn = row.min() if mn is None else min(row.min(), mn)
            mx = row.max() if mx is None else max(row.max(), mx)
        avg = acc(tot / acc(num)) if mode == "ref32" else tot / num
        with np.errstate(invalid="ignore"):
            std = np.sqrt(acc(tot2 / acc(num) - avg ** 2)) if mode == "ref32" else np.sqrt(tot2 / num - avg ** 2)
        out[name + "_num"] = num; out[name + "_sum"] = tot; out[name + "_sum2"] = tot2
        out[name + "_avg"] = avg; out[name + "_std"] = std
        out[name + "_min"] = np.float32(mn); out[name + "_max"] = np.float32(mx)
    if np.isnan(s).any():
        raise ValueError("NaN in the block")
    lines = ['Intra Distance: {}, {:.4f}+-{:.4f}, min {:.4f}, max {:.4f}'.format(out["intra_num"], out["intra_avg"], out["intra_std"],
                                                                                out["intra_min"], out["intra_max"]),
             'Inter Distance: {}, {:.4f}+-{:.4f}, min {:.4f}, max {:.4f}'.format(out["inter_num"], out["inter_avg"], out["inter_std"],
                                                                                out["inter_min"], out["inter_max"])]
    out["too_bad"] = bool(out["intra_avg"] >= out["inter_avg"])
    if out["too_bad"]:
        lines.append('The Metric Feature Is Too Bad!')
        out["thresholds"] = out["pos_err_rate"] = out["neg_err_rate"] = None
        out["pos_err_num"] = out["neg_err_num"] = None
    else:
        out["thresholds"] = np.linspace(out["intra_avg"], out["inter_avg"], 10)
        ge, lt, _ = threshold_counts(s, intra, out["thresholds"])
        out["pos_err_num"], out["neg_err_num"] = ge, lt
        out["pos_err_rate"] = ge.astype('float') / out["intra_num"]; out["neg_err_rate"] = lt.astype('float') / out["inter_num"]
        lines += ['pos pair num {}, neg pair num {}'.format(out["intra_num"], out["inter_num"]), '']
    inter_sorted = np.sort(s[inter])
    out["far"] = tuple(far)
    out["num"] = [int(f * out["inter_num"]) for f in far]
    out["thr"] = np.array([inter_sorted[k] for k in out["num"]], dtype=np.float32)
    pos = s[intra]
    out["cnt"] = [int((pos < t).sum()) for t in out["thr"]]
    out["GAR"] = [float(c) / out["intra_num"] for c in out["cnt"]]
    for k, f in enumerate(far):
        lines.append("thr:%.4f  FAR:%.5f(%d/%d)  GAR:%.5f(%d/%d)" % (out["thr"][k], f, out["num"][k], out["inter_num"], out["GAR"][k], out["cnt"][k],
                                                                     out["intra_num"]))
    out["lines"] = lines
    out["inter_sorted"] = inter_sorted
    return out


# ------------------------------------------------------------------ the test cases (inputs only; tools/make_golden_verify.py records the
# reference's results for the balanced ones)
def _grid(v):
    """features on a grid of 1/64, |v| <= 4: every square, sum and dot product below is then exact in float32 and in float64, so the
    distance block has the same bits on every machine, whatever order a BLAS adds in"""
    return (np.clip(np.round(np.asarray(v, dtype=np.float64) * 64.0), -256, 256) / 64.0).astype(np.float32)


def _block(rng, m, n, d, n_ids, noise):
    """features around n_ids centres; gallery label j % n_ids (balanced), query label i % n_ids"""
    c = rng.standard_normal((n_ids, d))
    rl = (np.arange(n) % n_ids).astype(np.int64); ql = (np.arange(m) % n_ids).astype(np.int64)
    y = _grid(c[rl] + noise * rng.standard_normal((n, d)))
    x = _grid(c[ql] + noise * rng.standard_normal((m, d)))
    return x, ql, y, rl


def sqdist(x, y):
    """squared distances of grid features by the expansion: exact, float32"""
    x = x.astype(np.float64); y = y.astype(np.float64)
    return ((x ** 2).sum(1)[:, None] + (y ** 2).sum(1)[None, :] - 2.0 * (x @ y.T)).astype(np.float32)


def make_case(name, seed=None):
    """-> dict(ql, rl, dist [m, ld] float32 padded, n, balanced).  The padding columns hold NaN-free garbage (1e30) that must never be
    read as part of the block."""
    seeds = SEEDS
    rng = np.random.default_rng(seeds[name] if seed is None else seed)
    balanced = True
    if name in ("a", "b"):
        m, n, d, ld = 37, 203, 16, 208
        x, ql, y, rl = _block(rng, m, n, d, 7, 0.8)               # 203 = 7 * 29: every query has 29 matches
        dist = sqdist(x, y)
        if name == "b":                                           # 30 % of the gallery columns repeat the column 7 places before (the same
            for j in np.sort(rng.permutation(np.arange(7, n))[: int(0.3 * n)]):      # identity, so the labels stay balanced): exact ties
                dist[:, j] = dist[:, j - 7]
    elif name == "c":
        m, n, d, ld = 24, 96, 8, 100
        x, ql, y, rl = _block(rng, m, n, d, 6, 0.3)
        y[:m] = x                                                 # gallery holds the queries: zeros; negative entries are put in below
        dist = sqdist(x, y)
        dist[rng.random(dist.shape) < 0.05] = 0.0
        dist[rng.random(dist.shape) < 0.05] *= np.float32(-1.0)
    elif name == "d":
        m, n, d, ld = 64, 4099, 16, 4100
        x, ql, y, rl = _block(rng, m, n, d, 65, 0.4)              # 4099 = 63 * 65 + 4: identities 0..3 have 64 images, the others 63
        ql = (4 + np.arange(m) % 61).astype(np.int64)             # queries of the 63-image identities only: equally many matches each
        x = _grid(y[ql] + 0.4 * rng.standard_normal((m, d)))
        dist = sqdist(x, y)
    elif name == "e":
        m, n, d, ld = 30, 120, 8, 120
        x, ql, y, rl = _block(rng, m, n, d, 6, 0.3)
        rl = np.roll(rl, 1)                                       # labels shifted against the features: intra pairs are the far ones
        ql = (ql + 3) % 6
        dist = sqdist(x, y)
    elif name == "f":
        m, n, d, ld = 20, 150, 8, 152
        x, ql, y, rl = _block(rng, m, n, d, 5, 0.35)
        rl = rl.copy(); rl[-30:] = -1                             # junk gallery entries (6 of each identity): inter for every query
        dist = sqdist(x, y)
    else:
        raise KeyError(name)
    pad = np.full((m, ld), np.float32(1e30), dtype=np.float32)
    pad[:, :n] = dist
    return {"name": name, "ql": ql, "rl": rl, "dist": pad, "n": n, "balanced": balanced, "x": x, "y": y}


CASES = ("a", "b", "c", "d", "e", "f")
SEEDS = {"a": 11, "b": 17, "c": 13, "d": 14, "e": 15, "f": 16}
