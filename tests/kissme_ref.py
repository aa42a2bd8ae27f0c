"""What the KISSME suites (tests/test_kissme_host.py, tests/test_gpu_kissme.py), tools/make_golden_kissme.py and tools/kissme_errors.py
share: the case table, the data of each case, and a float64 restatement of reid/metric_learning/kissme.py:33-55 that needs no meshgrid.

A case is (classes x images, d, centre spread): features = class centre + unit noise in float32, rows shuffled.

    A  48 x 8, d = 32      n = 384, P = 1344; int64 labels
    B  12 x 8, d = 64      n = 96,  P = 336; float32 labels
    C  40 x 6, d = 144     n = 240, P = 600 = 37 * 16 + 8: two output tiles (the second 16 columns wide), a ragged last pair slice
    D  classes of 1, 1, 2, 3, 5, 9, 30 rows, d = 40 (column padding), float32 labels that are not dense, P = 485 (odd);
       n - classes = 44 >= d, so C1 has full rank

A plain module, imported by name: no fixture lives here."""
import numpy as np

U64 = 2.0 ** -53

CASES = {
    "A": dict(sizes=[8] * 48, d=32, spread=2.0, seed=101, label_dtype=np.int64),
    "B": dict(sizes=[8] * 12, d=64, spread=2.0, seed=102, label_dtype=np.float32),
    "C": dict(sizes=[6] * 40, d=144, spread=2.0, seed=103, label_dtype=np.int64),
    "D": dict(sizes=[1, 1, 2, 3, 5, 9, 30], d=40, spread=2.0, seed=104, label_dtype=np.float32),
}
FIT_SEED = {"A": 11, "B": 12, "C": 13, "D": 14}        # seeds the stream the non-matching pairs are drawn from


def make_case(name):
    """-> (X float32 [n, d], y [n]) of a case; labels are 7 * class + 3 (not dense), rows in shuffled order"""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"])
    sizes = c["sizes"]
    cls = np.repeat(np.arange(len(sizes)), sizes)
    centres = c["spread"] * rs.standard_normal((len(sizes), c["d"]))
    X = centres[cls] + rs.standard_normal((cls.shape[0], c["d"]))
    perm = rs.permutation(cls.shape[0])
    assert cls.shape[0] - len(sizes) >= c["d"]           # C1 is a sum of n - classes independent differences at most
    return np.ascontiguousarray(X[perm].astype(np.float32)), (7 * cls[perm] + 3).astype(c["label_dtype"])


def pair_order(y):
    """all pairs a < b in the reference's order (b ascending, a ascending inside b) -> (a, b, matches)"""
    y = np.asarray(y)
    n = y.shape[0]
    b, a = np.nonzero(np.tri(n, n, -1, dtype=bool))       # row-major over the strict lower triangle: rows are b, columns a < b
    return a, b, y[a] == y[b]


def index_pairs(y, p=None, rng=None):
    """-> ia1, ib1 (every matching pair), p, ia0, ib0 (the sampled non-matching pairs).  p is drawn from `rng` the way kissme.py:46 draws
    it unless it is given."""
    a, b, m = pair_order(y)
    num_matches = int(m.sum())
    if p is None:
        p = rng.choice(int((~m).sum()), num_matches, replace=False)
    return a[m], b[m], np.asarray(p), a[~m][p], b[~m][p]


def cov64(X, ia, ib, divisor):
    """-> (C float64, A) with C = S^T S / divisor in float64 from the float32 rows, and A = sum_p |s_pi| |s_pj| / divisor, the magnitude
    the error bound (P + 2) 2^-53 A of a length-P float64 sum in any order is taken from"""
    S = X[ia].astype(np.float64) - X[ib].astype(np.float64)
    return S.T.dot(S) / divisor, np.abs(S).T.dot(np.abs(S)) / divisor


def cov_bound(P, A):
    """|dev - ref64| <= (P + 2) 2^-53 A: tests/train_common.bound with float64's unit"""
    return (P + 2) * U64 * A


def fit64(X, y, p):
    """the reference's fit in float64 up to M before validate_cov_matrix, with the index pairs and the bound matrices"""
    ia1, ib1, p, ia0, ib0 = index_pairs(y, p=p)
    P = ia1.shape[0]
    C1, A1 = cov64(X, ia1, ib1, P)
    C0, A0 = cov64(X, ia0, ib0, P)
    return dict(ia1=ia1, ib1=ib1, p=p, ia0=ia0, ib0=ib0, P=P, C1=C1, C0=C0, B1=cov_bound(P, A1), B0=cov_bound(P, A0),
                M_raw=np.linalg.inv(C1) - np.linalg.inv(C0))


def unrank_rule(y, pos):
    """numpy int64 restatement of the position -> (a, b) rule of ssg_kissme_unrank, without enumerating pairs: b from the scan of
    b - rank[b]; then with L the ascending member list of b's class, j = the smallest j with L[j] - j > q, a = q + j"""
    y = np.asarray(y); pos = np.asarray(pos, dtype=np.int64)
    n = y.shape[0]
    _, den = np.unique(y, return_inverse=True)
    den = den.reshape(-1)
    order = np.argsort(den, kind="stable")                 # members: every class's rows ascending
    counts = np.bincount(den)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n, dtype=np.int64) - ptr[den[order]]
    nm_scan = np.concatenate([[0], np.cumsum(np.arange(n, dtype=np.int64) - rank)]).astype(np.int64)
    b = np.searchsorted(nm_scan, pos, side="right") - 1
    q = pos - nm_scan[b]
    a = np.empty_like(pos)
    for t in range(pos.shape[0]):
        L = order[ptr[den[b[t]]]: ptr[den[b[t]]] + rank[b[t]]].astype(np.int64)
        j = int(np.searchsorted(L - np.arange(L.shape[0], dtype=np.int64), q[t], side="right"))
        a[t] = q[t] + j
    return a, b.astype(np.int64), int(nm_scan[n])
