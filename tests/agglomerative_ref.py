"""What the agglomerative tests share (tests/test_agglomerative_host.py, tests/test_gpu_agglomerative.py,
tools/make_agglomerative_golden.py): the case table, the matrices rebuilt from seeds, and a restatement of what sklearn 1.7.2's
`AgglomerativeClustering(metric='precomputed', connectivity=None)` computes through scipy 1.15.3's `linkage`: `nn_chain` (average,
complete), `mst_single_linkage` (single), the stable sort, `label`, and sklearn's `_hc_cut`.  tests/golden/agglomerative_cases.npz holds
what scipy and sklearn themselves gave for every case and a sha256 of every rebuilt matrix.

The loops are restated twice: entry by entry in plain Python exactly as scipy's compiled loops run (`literal=True`, used where N is
small), and with one numpy pass per scan (used everywhere); tests/test_agglomerative_host.py holds the two against each other.  Both are
written apart from the product's host stage (ssg_amd/agglomerative.py) so that the two check each other.
"""
import hashlib
import heapq
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agglomerative_cases.npz")
LINKAGES = ("average", "complete", "single")
INF = float("inf")

# kind: 'q16' distances of random points quantised to a handful of float16 levels (nearly every scan has ties; float16 input);
# 'f64' the same distances unquantised; 'equal' every entry 0.5; 'neg' a float64 matrix drawn from seven levels, negative ones and
# both zeros among them; 'asym' a float64 matrix whose two triangles are drawn apart (only the upper one counts); 'prevtie' built so that
# chain[-2] ties with a lower-indexed slot; 'rerank' the final_dist of a re-rank golden.
CASES = [
    dict(name="n2", N=2, kind="f64", seed=1),
    dict(name="n3_q16", N=3, kind="q16", seed=2),
    dict(name="n17_prevtie", N=17, kind="prevtie", seed=3),
    dict(name="n65_q16", N=65, kind="q16", seed=4),
    dict(name="n65_equal", N=65, kind="equal", seed=0),
    dict(name="n130_asym", N=130, kind="asym", seed=5),
    dict(name="n130_neg", N=130, kind="neg", seed=6),
    dict(name="n257_q16", N=257, kind="q16", seed=7),
    dict(name="n1025_q16", N=1025, kind="q16", seed=8),
    dict(name="n1501_f64", N=1501, kind="f64", seed=9),
    dict(name="rerank_n256", N=256, kind="rerank", seed=0, file="rerank_n256_l03_ref.npz", lambda_value=0.3),
]
BY_NAME = {c["name"]: c for c in CASES}
LITERAL_MAX_N = 130                       # the entry-by-entry loops run up to this N

_MATS = {}


def matrix(case):
    """the case's matrix as the tests hand it over (float16 for kind 'q16', else float64); read-only"""
    key = (case["kind"], case["N"], case["seed"])
    if key in _MATS:
        return _MATS[key]
    N, kind = case["N"], case["kind"]
    rs = np.random.RandomState(1000 + case["seed"])
    if kind == "rerank":
        with np.load(os.path.join(os.path.dirname(GOLDEN), case["file"])) as z:
            D = z["final"]
        assert D.dtype == np.float64 and D.shape == (N, N)
    elif kind in ("q16", "f64"):
        centres = rs.standard_normal((max(2, N // 12), 3)) * 2.0
        pts = centres[rs.randint(0, len(centres), N)] + 0.5 * rs.standard_normal((N, 3))
        D = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
        if kind == "q16":
            D = (np.ceil(D / D.max() * 6.0) / 4.0).astype(np.float16)      # levels 0.25 .. 1.5 off the diagonal
            D[np.arange(N), np.arange(N)] = np.float16(0.125)               # a non-zero diagonal: it is never looked at
    elif kind == "equal":
        D = np.full((N, N), 0.5)
    elif kind == "neg":
        levels = np.array([-1.0, -0.5, -0.0, 0.0, 0.5, 1.0, 2.0])
        U = levels[rs.randint(0, len(levels), (N, N))]
        D = np.where(np.triu(np.ones((N, N), dtype=bool), 1), U, U.T)      # (not a sum: -0.0 + 0.0 is +0.0)
        D[np.arange(N), np.arange(N)] = -3.0
    elif kind == "asym":
        D = rs.uniform(0.1, 4.0, (N, N))
        assert not np.array_equal(D, D.T)
    elif kind == "prevtie":
        D = np.full((N, N), 5.0) + np.triu(0.001 * rs.randint(0, 3, (N, N)), 1)
        D = np.triu(D, 1) + np.triu(D, 1).T
        for (i, j, v) in ((0, 9, 3.0), (9, 12, 2.0), (4, 12, 2.0)):        # the chain 0 -> 9 -> 12; from 12, slot 4 ties with chain[-2] = 9
            D[i, j] = D[j, i] = v
    else:
        raise ValueError(kind)
    D = np.ascontiguousarray(D)
    D.setflags(write=False)
    _MATS[key] = D
    return D


def sha(D):
    return hashlib.sha256(np.ascontiguousarray(D).tobytes()).hexdigest()


def condensed(D):
    """what sklearn hands to scipy: X[np.triu_indices(N, 1)] (scipy widens it to float64)"""
    i, j = np.triu_indices(len(D), k=1)
    return np.asarray(D)[i, j].astype(np.float64)


def square(D):
    """the float64 square with d(i,j) = X[min(i,j), max(i,j)] on both sides; the diagonal is never read (set to NaN here to show it)"""
    X = np.asarray(D).astype(np.float64)
    W = np.where(np.triu(np.ones(X.shape, dtype=bool), 1), X, X.T)         # (not a sum: -0.0 + 0.0 is +0.0)
    W[np.arange(len(W)), np.arange(len(W))] = np.nan
    return W


# ---------------------------------------------------------------------------------------------------------------- the loops
def nn_chain(D, method, literal=False, stats=None):
    """scipy's nn_chain before its sort -> (x, y, distance, size), each [N - 1], in merge order.  stats (a dict): counts the scans and
    the scans on which chain[-2] kept a tie against a lower-indexed slot"""
    W = square(D)
    n = len(W)
    size = [1] * n
    live = np.ones(n, dtype=bool)
    chain = []
    ox, oy, od, osz = np.empty(n - 1, np.int64), np.empty(n - 1, np.int64), np.empty(n - 1, np.float64), np.empty(n - 1, np.int64)
    scans = prev_kept = 0
    for k in range(n - 1):
        if not chain:
            chain.append(next(i for i in range(n) if size[i] > 0))
        while True:
            x = chain[-1]
            scans += 1
            if literal:
                if len(chain) > 1:
                    y, cur = chain[-2], W[x, chain[-2]]
                else:
                    y, cur = -1, INF
                for i in range(n):
                    if size[i] == 0 or i == x:
                        continue
                    if W[x, i] < cur:
                        cur, y = W[x, i], i
            else:
                row = np.where(live, W[x], INF)
                row[x] = INF
                y = int(np.argmin(row))                                  # the lowest index attaining the minimum
                cur = row[y]
                if len(chain) > 1 and not cur < W[x, chain[-2]]:         # chain[-2] keeps every tie with the minimum
                    if y < chain[-2]:
                        prev_kept += 1
                    y, cur = chain[-2], W[x, chain[-2]]
            if len(chain) > 1 and y == chain[-2]:
                break
            chain.append(y)
        del chain[-2:]
        if x > y:
            x, y = y, x
        nx, ny = size[x], size[y]
        ox[k], oy[k], od[k], osz[k] = x, y, cur, nx + ny
        size[x], size[y] = 0, nx + ny
        live[x] = False
        if literal:
            for i in range(n):
                if size[i] == 0 or i == y:
                    continue
                a, b = W[i, x], W[i, y]
                v = max(a, b) if method == "complete" else (np.float64(nx) * a + np.float64(ny) * b) / np.float64(nx + ny)
                W[i, y] = W[y, i] = v
        else:
            a, b = W[x], W[y]
            v = np.where(b > a, b, a) if method == "complete" else (np.float64(nx) * a + np.float64(ny) * b) / np.float64(nx + ny)
            keep = live.copy()
            keep[y] = False
            W[y, keep] = v[keep]
            W[keep, y] = v[keep]
    if stats is not None:
        stats["scans"], stats["prev_kept"] = scans, prev_kept
    assert scans <= 3 * (n - 1)
    return ox, oy, od, osz


def mst_single_linkage(D, literal=False):
    """scipy's mst_single_linkage before its sort -> (x, y, distance), each [N - 1], in Prim order"""
    W = square(D)
    n = len(W)
    merged = np.zeros(n, dtype=bool)
    m = np.full(n, INF)
    ox, oy, od = np.empty(n - 1, np.int64), np.empty(n - 1, np.int64), np.empty(n - 1, np.float64)
    x = y = 0
    for k in range(n - 1):
        merged[x] = True
        if literal:
            cur = INF
            for i in range(n):
                if merged[i]:
                    continue
                if m[i] > W[x, i]:
                    m[i] = W[x, i]
                if m[i] < cur:
                    y, cur = i, m[i]
        else:
            m = np.where(m > W[x], W[x], m)                              # (W[x, x] is NaN: the comparison fails and m[x] stays)
            row = np.where(merged, INF, m)
            y = int(np.argmin(row))
            cur = row[y]
        ox[k], oy[k], od[k] = x, y, cur
        x = y
    return ox, oy, od


def merges(D, method, literal=False, stats=None):
    """-> (x, y, distance, size or None) in merge order"""
    if method == "single":
        return mst_single_linkage(D, literal) + (None,)
    return nn_chain(D, method, literal, stats)


def label(x, y, distance):
    """the stable sort by height and scipy's `label` -> Z [N - 1, 4]"""
    n = len(distance) + 1
    order = np.argsort(distance, kind="stable")
    parent = np.full(2 * n - 1, -1, dtype=np.int64)
    size = np.concatenate([np.ones(n, np.int64), np.zeros(n - 1, np.int64)])

    def find(a):
        while parent[a] != -1:
            a = parent[a]
        return a

    Z = np.empty((n - 1, 4))
    for i, e in enumerate(order):
        a, b = find(x[e]), find(y[e])
        Z[i] = (min(a, b), max(a, b), distance[e], size[a] + size[b])
        parent[a] = parent[b] = n + i
        size[n + i] = size[a] + size[b]
    return Z


def hc_cut(n_clusters, children, n_leaves):
    """sklearn's _hc_cut"""
    nodes = [-(max(children[-1]) + 1)]
    for _ in range(n_clusters - 1):
        these = children[-nodes[0] - n_leaves]
        heapq.heappush(nodes, -these[0])
        heapq.heappushpop(nodes, -these[1])
    lab = np.zeros(n_leaves, dtype=np.intp)

    def leaves(node):
        out, todo = [], [node]
        while todo:
            t = todo.pop()
            if t < n_leaves:
                out.append(t)
            else:
                todo.extend(children[t - n_leaves])
        return out

    for i, node in enumerate(nodes):
        lab[leaves(-node)] = i
    return lab


def linkage(D, method, literal=False):
    x, y, d, _ = merges(D, method, literal)
    return label(x, y, d)


# ---------------------------------------------------------------------------------------------------------------- the estimator's options
def n_clusters_options(N):
    return sorted({1, min(2, N), min(7, N), N})


def thresholds(Z):
    """below the first merge, between two merges, equal to a merge height, above the last (negative values are not valid thresholds:
    clipped to 0)"""
    h = Z[:, 2]
    mid = len(h) // 2
    out = [min(h[0] - 1.0, h[0] / 2.0), h[mid], h[-1] + 1.0]
    up = h[h > h[mid]]
    if len(up):
        out.append((h[mid] + up[0]) / 2.0)
    return sorted({float(max(0.0, t)) for t in out})


def fit(Z, n_clusters=None, distance_threshold=None):
    """-> (children_, n_clusters_, labels_)"""
    n = len(Z) + 1
    children = Z[:, :2].astype(int)
    k = n_clusters if distance_threshold is None else int(np.count_nonzero(Z[:, 2] >= distance_threshold)) + 1
    return children, k, hc_cut(k, children.tolist(), n)


def drop_small(labels, min_cluster_size):
    """the small-cluster rule of generate_selflabel_agglomerative"""
    labels = np.asarray(labels)
    out = np.full(len(labels), -1, dtype=np.intp)
    seen = []
    for i, l in enumerate(labels):
        if (labels == l).sum() >= min_cluster_size:
            if l not in seen:
                seen.append(l)
            out[i] = seen.index(l)
    return out


def load_golden():
    z = np.load(GOLDEN, allow_pickle=False)
    for c in CASES:
        assert str(z[c["name"] + "/sha256"]) == sha(matrix(c)), "the matrix of case %s is not the one the golden was made from" % c["name"]
    return z
