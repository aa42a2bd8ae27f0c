"""What the silhouette tests share (tests/test_silhouette_host.py, tests/test_gpu_silhouette.py, tools/make_silhouette_golden.py): the
case table, the matrices and labelings rebuilt from seeds, and a sequential restatement of what sklearn 1.7.2's `silhouette_samples(X,
labels, metric='precomputed')` computes: per row one running float64 sum per cluster, added in column order (`np.bincount(labels,
weights=row)`), the own cluster's sum, the smallest mean of another cluster, then sklearn's four numpy lines.
tests/golden/silhouette_cases.npz holds what sklearn itself gave for every case: the labels, the per-sample result, the scores.  No
sklearn import and no GPU here.

The restatement is written apart from the product (ssg_amd/silhouette.py, csrc/silhouette.hip) so that the two check each other.
"""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = os.path.join(GOLDEN_DIR, "silhouette_cases.npz")
RERANK_FILE, RERANK_LAMBDA = "rerank_n256_l01_ref.npz", 0.1

# kind: 'f64' symmetric uniform distances with a zero diagonal; 'f32' / 'f16' the same cast down (expected: sklearn on the float64 copy);
# 'neg' a symmetric matrix of normal draws, negative entries among them; 'rerank' the final_dist of a re-rank golden with its diagonal
# zeroed.  labeling: 'halves' two clusters of N / 2 (the longest chains); 'big_single' one cluster of N - 1 and a singleton; 'pairs'
# all pairs plus one triple (and one singleton when N is even); 'many' more clusters than a workgroup has threads at N = 1030; 'gapped'
# negative and gapped integer labels; 'noise' a third of the samples labelled -1 (ignore_noise); 'few' eight clusters.
# sample: the case also stores silhouette_score(sample_size=N // 2, random_state=SAMPLE_SEED) and the stream's next draw.
SAMPLE_SEED = 3
CASES = [
    dict(name="n3_halves", N=3, kind="f64", labeling="halves", seed=1),
    dict(name="n7_halves", N=7, kind="f64", labeling="halves", seed=2),
    dict(name="n7_big_single", N=7, kind="f64", labeling="big_single", seed=3),
    dict(name="n7_pairs", N=7, kind="f64", labeling="pairs", seed=4),
    dict(name="n7_gapped", N=7, kind="f64", labeling="gapped", seed=5),
    dict(name="n65_halves", N=65, kind="f64", labeling="halves", seed=6, sample=True),
    dict(name="n65_big_single", N=65, kind="f64", labeling="big_single", seed=7),
    dict(name="n65_pairs", N=65, kind="f64", labeling="pairs", seed=8),
    dict(name="n65_gapped_f32", N=65, kind="f32", labeling="gapped", seed=9),
    dict(name="n65_gapped_f16", N=65, kind="f16", labeling="gapped", seed=10),
    dict(name="n65_neg", N=65, kind="neg", labeling="gapped", seed=11),
    dict(name="n65_noise", N=65, kind="f64", labeling="noise", seed=12),
    dict(name="n513_halves", N=513, kind="f64", labeling="halves", seed=13),
    dict(name="n513_big_single", N=513, kind="f64", labeling="big_single", seed=14),
    dict(name="n513_pairs_f16", N=513, kind="f16", labeling="pairs", seed=15),
    dict(name="n513_gapped_f32", N=513, kind="f32", labeling="gapped", seed=16),
    dict(name="n513_neg", N=513, kind="neg", labeling="halves", seed=17),
    dict(name="n513_noise", N=513, kind="f64", labeling="noise", seed=18),
    dict(name="n513_few", N=513, kind="f64", labeling="few", seed=19, sample=True),
    dict(name="n1030_halves", N=1030, kind="f64", labeling="halves", seed=20),
    dict(name="n1030_pairs", N=1030, kind="f64", labeling="pairs", seed=21),
    dict(name="n1030_many", N=1030, kind="f64", labeling="many", seed=22),
    dict(name="n1030_gapped_f16", N=1030, kind="f16", labeling="gapped", seed=23),
    dict(name="rerank_n256_few", N=256, kind="rerank", labeling="few", seed=24),
    dict(name="rerank_n256_noise", N=256, kind="rerank", labeling="noise", seed=25),
]
BY_NAME = {c["name"]: c for c in CASES}

_MATS = {}


def matrix(case):
    """the case's matrix as the tests hand it over (float16, float32 or float64); read-only.  The 'rerank' matrix is the golden final_dist
    as stored, with its non-zero diagonal: `expected_input` zeroes it."""
    key = (case["kind"], case["N"], case["seed"])
    if key in _MATS:
        return _MATS[key]
    N, kind = case["N"], case["kind"]
    rs = np.random.RandomState(2000 + case["seed"])
    if kind == "rerank":
        with np.load(os.path.join(GOLDEN_DIR, RERANK_FILE)) as z:
            D = z["final"]
        assert D.dtype == np.float64 and D.shape == (N, N)
    elif kind == "neg":
        U = rs.standard_normal((N, N))
        D = np.triu(U, 1) + np.triu(U, 1).T
    else:
        U = rs.uniform(0.05, 2.0, (N, N))
        D = np.triu(U, 1) + np.triu(U, 1).T
        D = D.astype({"f64": np.float64, "f32": np.float32, "f16": np.float16}[kind])
    D = np.ascontiguousarray(D)
    D.setflags(write=False)
    _MATS[key] = D
    return D


def expected_input(case):
    """the float64 matrix sklearn is given for this case: the float64 copy, the diagonal zeroed for 'rerank'"""
    X = np.array(matrix(case), dtype=np.float64)
    if case["kind"] == "rerank":
        np.fill_diagonal(X, 0.0)
    return X


def labels(case):
    """the case's labeling, rebuilt from its seed (the golden stores it too, and the tests compare)"""
    N, how = case["N"], case["labeling"]
    rs = np.random.RandomState(3000 + case["seed"])
    if how == "halves":
        lab = (np.arange(N) >= (N + 1) // 2).astype(np.int64)
    elif how == "big_single":
        lab = np.zeros(N, dtype=np.int64)
        lab[rs.randint(0, N)] = 1
    elif how == "pairs":
        lab = np.empty(N, dtype=np.int64)
        lab[:3] = 0                                               # the triple
        rest = N - 3
        lab[3:3 + 2 * (rest // 2)] = 1 + np.arange(2 * (rest // 2)) // 2
        if rest % 2:
            lab[-1] = 1 + rest // 2                               # (N even: one singleton is left over)
    elif how == "many":
        lab = rs.randint(0, 600, N).astype(np.int64)
    elif how == "gapped":
        lab = np.array([-7, -1, 3, 10, 1000], dtype=np.int64)[rs.randint(0, 5, N)]
        lab[:5] = [-7, -1, 3, 10, 1000]
    elif how == "few":
        lab = rs.randint(0, 8, N).astype(np.int64)
    elif how == "noise":
        lab = rs.randint(0, 6, N).astype(np.int64)
        lab[rs.permutation(N)[:N // 3]] = -1
    else:
        raise ValueError(how)
    if how not in ("halves",):
        lab = lab[rs.permutation(N)]
    return lab


def ignore_noise(case):
    return case["labeling"] == "noise"


# ---------------------------------------------------------------------------------------------------------------- the restatement
def reduce_rows(X, enc, C):
    """_silhouette_reduce, sequentially: for every row one running float64 sum per cluster, the columns added in order ->
    (intra [m] = s[i, own], inter [m] = min over c != own of s[i, c] / float64(freq[c]))"""
    m = len(enc)
    enc = [int(e) for e in enc]
    freq = [0] * C
    for e in enc:
        freq[e] += 1
    freq = np.array(freq, dtype=np.float64)
    intra, inter = np.empty(m, dtype=np.float64), np.empty(m, dtype=np.float64)
    for i, row in enumerate(np.asarray(X, dtype=np.float64).tolist()):
        s = [0.0] * C
        for j in range(m):
            s[enc[j]] += row[j]                                   # (a Python float is an IEEE double: one rounding per add)
        intra[i] = s[enc[i]]
        s[enc[i]] = np.inf
        inter[i] = (np.array(s, dtype=np.float64) / freq).min()
    return intra, inter


def silhouette_samples(X, lab):
    """sklearn's silhouette_samples(X, lab, metric='precomputed') for a float64 X whose checks have passed"""
    classes, enc = np.unique(np.asarray(lab), return_inverse=True)
    C, n = len(classes), len(enc)
    if not 1 < C < n:
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % C)
    freq = np.bincount(enc)
    intra, inter = reduce_rows(X, enc, C)
    denom = (freq - 1).take(enc, mode="clip")
    with np.errstate(divide="ignore", invalid="ignore"):
        intra /= denom
    sil = inter - intra
    with np.errstate(divide="ignore", invalid="ignore"):
        sil /= np.maximum(intra, inter)
    return np.nan_to_num(sil)


def samples_without_noise(X, lab):
    """sklearn on X[keep][:, keep], lab[keep] for keep = lab != -1, scattered back with NaN at the dropped positions"""
    lab = np.asarray(lab)
    keep = lab != -1
    out = np.full(len(lab), np.nan, dtype=np.float64)
    out[keep] = silhouette_samples(np.asarray(X)[keep][:, keep], lab[keep])
    return out


def sampled_score(X, lab, sample_size, rs):
    """silhouette_score(X, lab, metric='precomputed', sample_size=sample_size, random_state=rs) for a RandomState rs: the sub-matrix
    in PERMUTED order"""
    idx = rs.permutation(len(lab))[:sample_size]
    return float(np.mean(silhouette_samples(np.asarray(X)[idx].T[idx].T, np.asarray(lab)[idx])))


def expected(case):
    """the restatement's per-sample result for a case"""
    X, lab = expected_input(case), labels(case)
    return samples_without_noise(X, lab) if ignore_noise(case) else silhouette_samples(X, lab)


def load_golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
