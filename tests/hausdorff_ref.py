"""numpy restatement of reid/rerank_hausdorff.py:7-65 re_ranking with every float64 operation in the order scipy's cdist and
directed_hausdorff take it, so that it reproduces the reference's two returns bit for bit (tests/test_hausdorff_host.py holds it
against goldens written by the reference itself) and hands out the intermediate stages the device path is checked against.

Needs numpy only."""
import numpy as np


def seq_sqdist(a, b):
    """s[i, j]: s = 0.0; for c = 0 .. d-1: t = f64(a[i, c]) - f64(b[j, c]); s = s + t * t  (product and sum rounded separately)"""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    s = np.zeros((a.shape[0], b.shape[0]), dtype=np.float64)
    for c in range(a.shape[1]):
        t = a[:, c, None] - b[None, :, c]
        s = s + t * t
    return s


def seq_dist(a, b):
    return np.sqrt(seq_sqdist(a, b))


def half_distance(tgt, memory_save=False):
    """rerank_hausdorff.py:22-38: the half original distance (the float64 sums of half-rounded features in [-1, 1] are exact, and
    scipy's sqrt is correctly rounded like numpy's)"""
    feat = np.asarray(tgt).astype(np.float16)
    cd = seq_dist(feat, feat)
    if memory_save:
        return np.power(cd, 2).astype(np.float16)
    return np.power(cd.astype(np.float16), 2).astype(np.float16)


def knn_sets(D, k):
    """:43-49 -> list of ascending index arrays S_i = { j != i : D[i, j] <= k-th smallest of row i }"""
    sets = []
    for i in range(D.shape[0]):
        thr = np.sort(D[i])[k - 1]
        m = D[i] <= thr
        m[i] = False
        sets.append(np.nonzero(m)[0])
    return sets


def hausdorff_from_sets(E, sets):
    """H[i, j] = max(max_{a in S_i} min_{b in S_j} E[a, b], max_{b in S_j} min_{a in S_i} E[a, b]), H[i, i] = 0  (:52-58)"""
    N = E.shape[0]
    H = np.zeros((N, N), dtype=np.float64)
    for i in range(N):
        Ei = E[sets[i]]
        for j in range(i + 1, N):
            sub = Ei[:, sets[j]]
            H[i, j] = H[j, i] = max(sub.min(axis=1).max(), sub.min(axis=0).max())
    return H


def re_ranking(src, tgt, k=20, lambda_value=0.1, MemorySave=False):
    """-> dict(euclidean_dist float16, final_dist float64, vec, D, sets, E, H)"""
    src = np.asarray(src); tgt = np.asarray(tgt)
    vec = np.sqrt(seq_sqdist(tgt, src).min(axis=1))
    vec = vec / np.max(vec)
    D = half_distance(tgt, MemorySave)
    euclidean_dist = D / np.max(D)
    sets = knn_sets(D, k)
    E = seq_dist(tgt, tgt)
    H = hausdorff_from_sets(E, sets)
    Hn = H / np.max(H)
    source_dist = vec[None, :] + vec[:, None]
    final_dist = Hn * (1 - lambda_value) + source_dist * lambda_value
    return dict(euclidean_dist=euclidean_dist, final_dist=final_dist, vec=vec, D=D, sets=sets, E=E, H=H)


def load_cases(path):
    """tests/golden/hausdorff_cases.npz -> {name: dict(src, tgt, k, lambda_value, MemorySave, Minibatch, euclidean_dist, final_dist)}"""
    z = np.load(path)
    cases = {}
    for name in [str(n) for n in z["names"]]:
        k, lam, ms, mb = z[name + "_params"]
        N = z[name + "_tgt"].shape[0]
        final = np.zeros((N, N), dtype=np.float64)          # stored as its upper triangle: the reference's matrix is exactly symmetric
        final[np.triu_indices(N)] = z[name + "_final_dist_triu"]
        final = np.maximum(final, final.T)
        cases[name] = dict(src=z[name + "_src"], tgt=z[name + "_tgt"], k=int(k), lambda_value=float(lam), MemorySave=bool(ms), Minibatch=int(mb),
                           euclidean_dist=z[name + "_euclidean_dist"], final_dist=final)
    return cases
