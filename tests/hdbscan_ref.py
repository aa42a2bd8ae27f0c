"""What the HDBSCAN tests share (tests/test_hdbscan_host.py, tests/test_gpu_hdbscan.py, tools/make_hdbscan_golden.py): the case table,
the matrices rebuilt from seeds (tests/optics_ref.py builds them), and a restatement of sklearn 1.7.2's `HDBSCAN(metric='precomputed')`
in numpy steps and plain loops: the core distances, Prim (`mst_from_mutual_reachability`), `make_single_linkage`, `tree_to_labels`
and `labelling_at_cut`.  tests/golden/hdbscan_cases.npz holds what sklearn itself gave for every case, the order in which the machine that
made the golden sorted the edges, and a sha256 of every rebuilt matrix.

The restatement follows sklearn's own data layout (the condensed tree as four parallel arrays, masks over them) and is written apart
from the product's host stage (ssg_amd/hdbscan.py, dictionaries and child lists), so that the two check each other.
"""
import hashlib
import os

import numpy as np

import optics_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hdbscan_cases.npz")
INF = float("inf")


def _case(name, N, kind, seed, mcs, ms=None, alpha=1.0, method="eom", single=False, eps=0.0, max_size=None, cuts=(0.2, 0.5), full=False, **extra):
    return dict(name=name, N=N, kind=kind, seed=seed, min_cluster_size=mcs, min_samples=ms, alpha=alpha, method=method, allow_single_cluster=single,
                epsilon=eps, max_cluster_size=max_size, cuts=tuple(cuts), full=full, **extra)


# kind: as in optics_ref ('half' float16-derived and tie-heavy with a non-zero diagonal, 'dup' exact zeros off the diagonal, 'f64',
# 'rerank' the final_dist of a re-rank golden), and 'inf': the 'half' matrix with a symmetric set of +inf entries -- five nodes lose every
# distance (they are unreachable: their edges weigh +inf and sklearn warns) and 300 more pairs lose theirs.
# full: sklearn's own result shows at least 2 clusters and at least one noise point (tools/make_hdbscan_golden.py asserts it).
CASES = [
    _case("n2", 2, "f64", 1, 2, cuts=(0.5, 10.0)),
    _case("n7", 7, "half", 2, 2, cuts=(0.5, 3.0)),
    _case("n64_half", 64, "half", 4, 4, full=True),
    _case("n64_half_m10", 64, "half", 4, 10, full=True),
    _case("n64_half_leaf", 64, "half", 4, 5, method="leaf", full=True),
    _case("n65_all", 65, "f64", 5, 5, ms=65, cuts=(3.0, 6.0)),
    _case("n257_half", 257, "half", 7, 5, full=True),
    _case("n257_half_a15", 257, "half", 7, 4, ms=3, alpha=1.5, cuts=(0.1, 0.3), full=True),
    _case("n257_half_eps", 257, "half", 7, 5, eps=1.5),
    _case("n257_dup", 257, "dup", 8, 4, full=True),
    _case("n257_dup_m2", 257, "dup", 8, 2, ms=3, method="leaf", eps=0.1),
    _case("n257_inf", 257, "inf", 7, 5),
    _case("n513_f64", 513, "f64", 9, 10, full=True),
    _case("n513_f64_max", 513, "f64", 9, 5, max_size=20),
    _case("n513_f64_max12", 513, "f64", 9, 5, max_size=12),       # (20 changes nothing on this matrix, 12 does)
    _case("n513_half_ms1", 513, "half", 10, 4, ms=1),
    _case("n3001_half", 3001, "half", 11, 4, full=True),
    # the final_dist of an existing re-rank golden (lambda 0.3): on the GPU the matrix is the mode-0 handle re_ranking_device builds from
    # that golden's features, read through its compact form
    _case("rerank_n256", 256, "rerank", 0, 4, cuts=(0.6, 0.63), file="rerank_n256_l03_ref.npz", lambda_value=0.3),
    _case("rerank_n256_single", 256, "rerank", 0, 10, single=True, cuts=(0.6, 0.63), file="rerank_n256_l03_ref.npz", lambda_value=0.3),
]
BY_NAME = {c["name"]: c for c in CASES}

_MATS = {}


def matrix(case):
    """the case's matrix as the tests hand it over: float16 for kinds 'half' and 'inf' (its float64 copy is what sklearn saw), else
    float64; read-only and shared between the cases that use the same matrix"""
    key = (case["kind"], case["N"], case["seed"])
    if key in _MATS:
        return _MATS[key]
    kind = case["kind"]
    if kind == "rerank":
        # read here: optics_ref.matrix keeps a 'rerank' matrix of a case outside its own table under the key it gives every such case,
        # and would hand it out again for the next one
        with np.load(os.path.join(os.path.dirname(GOLDEN), case["file"])) as z:
            D = z["final"]
        assert D.dtype == np.float64 and D.shape == (case["N"], case["N"])
        D.setflags(write=False)
    else:
        D = optics_ref.matrix(dict(name="hdbscan:%s:%d:%d" % key, N=case["N"], kind="half" if kind == "inf" else kind, seed=case["seed"]))
    if kind == "inf":
        D = np.array(D)
        N = case["N"]
        rs = np.random.RandomState(case["seed"] + 3000)
        gone = rs.permutation(N)[:5]
        keep = D[np.arange(N), np.arange(N)].copy()
        D[gone, :] = np.inf
        D[:, gone] = np.inf
        a, b = rs.randint(0, N, size=300), rs.randint(0, N, size=300)
        D[a, b] = np.inf
        D[b, a] = np.inf
        D[np.arange(N), np.arange(N)] = keep                             # the diagonal stays finite
        D.setflags(write=False)
    _MATS[key] = D
    return D


def sha(D):
    return hashlib.sha256(np.ascontiguousarray(D).tobytes()).hexdigest()


def min_samples_of(case):
    return case["min_cluster_size"] if case["min_samples"] is None else case["min_samples"]


# ---------------------------------------------------------------------------------------------------------------- core distances, Prim
def core_distances(X, min_samples, alpha=1.0):
    """the min_samples-th smallest entry of every row of X / alpha, the diagonal counted as it stands"""
    X = np.asarray(X, dtype=np.float64) / alpha
    return np.partition(X, min_samples - 1, axis=1)[:, min_samples - 1].copy()


def prim(X, core, alpha=1.0):
    """mst_from_mutual_reachability on max(core[c], core[j], X[c, j] / alpha) without the N x N graph: from node 0, N - 1 steps; the
    edge is (the node the step started from, the first minimum over the remaining nodes, its value) -> (current, next, distance)"""
    X = np.asarray(X)                                                    # (widened row by row: a large float16 matrix stays as it is)
    n = len(X)
    labels = np.arange(n)
    m = np.full(n, np.inf)
    cur, nxt, dist = np.empty(n - 1, np.int64), np.empty(n - 1, np.int64), np.empty(n - 1, np.float64)
    c = 0
    for i in range(n - 1):
        keep = labels != c
        labels, m = labels[keep], m[keep]
        row = X[c, labels].astype(np.float64) / alpha
        mr = np.where(core[labels] > core[c], core[labels], core[c])     # max(core[c], core[j], d): the first of equal values
        mr = np.where(row > mr, row, mr)
        m = np.minimum(m, mr)
        k = int(np.argmin(m))
        cur[i], nxt[i], dist[i] = c, labels[k], m[k]
        c = int(labels[k])
    return cur, nxt, dist


# ---------------------------------------------------------------------------------------------------------------- single linkage
def single_linkage(cur, nxt, dist, row_order):
    """make_single_linkage on the edges taken in `row_order` -> (left, right, value, size), each [N - 1]"""
    n = len(dist) + 1
    parent = np.full(2 * n - 1, -1, dtype=np.int64)
    size = np.concatenate([np.ones(n, np.int64), np.zeros(n - 1, np.int64)])
    left, right, value, csize = np.empty(n - 1, np.int64), np.empty(n - 1, np.int64), np.empty(n - 1, np.float64), np.empty(n - 1, np.int64)

    def find(x):
        while parent[x] != -1:
            x = parent[x]
        return x

    for i, e in enumerate(row_order):
        a, b = find(cur[e]), find(nxt[e])
        left[i], right[i], value[i], csize[i] = a, b, dist[e], size[a] + size[b]
        parent[a] = parent[b] = n + i
        size[n + i] = csize[i]
    return left, right, value, csize


# ---------------------------------------------------------------------------------------------------------------- tree_to_labels
def _bfs_hierarchy(left, right, n, root):
    out, queue = [], [root]
    while queue:
        out.extend(queue)
        queue = [x - n for x in queue if x >= n]
        if queue:
            queue = [y for x in queue for y in (left[x], right[x])]
    return out


def condense_tree(left, right, value, csize, min_cluster_size):
    n = len(left) + 1
    root = 2 * (n - 1)
    next_label = n + 1
    relabel = np.empty(root + 1, dtype=np.int64)
    relabel[root] = n
    ignore = np.zeros(root + 1, dtype=bool)
    rows = []
    for node in _bfs_hierarchy(left, right, n, root):
        if ignore[node] or node < n:
            continue
        lt, rt, d = int(left[node - n]), int(right[node - n]), value[node - n]
        lam = 1.0 / d if d > 0.0 else np.inf
        lc = csize[lt - n] if lt >= n else 1
        rc = csize[rt - n] if rt >= n else 1
        small = []
        if lc >= min_cluster_size and rc >= min_cluster_size:
            for side, count in ((lt, lc), (rt, rc)):
                relabel[side] = next_label
                next_label += 1
                rows.append((relabel[node], relabel[side], lam, count))
        elif lc < min_cluster_size and rc < min_cluster_size:
            small = [lt, rt]
        elif lc < min_cluster_size:
            relabel[rt] = relabel[node]
            small = [lt]
        else:
            relabel[lt] = relabel[node]
            small = [rt]
        for side in small:
            for sub in _bfs_hierarchy(left, right, n, side):
                if sub < n:
                    rows.append((relabel[node], sub, lam, 1))
                ignore[sub] = True
    parent = np.array([r[0] for r in rows], dtype=np.int64)
    child = np.array([r[1] for r in rows], dtype=np.int64)
    lam = np.array([r[2] for r in rows], dtype=np.float64)
    size = np.array([r[3] for r in rows], dtype=np.int64)
    return parent, child, lam, size


def compute_stability(parent, child, lam, size):
    smallest = int(parent.min())
    births = np.full(max(int(child.max()), smallest) + 1, np.nan)
    for c, v in zip(child, lam):
        births[c] = v
    births[smallest] = 0.0
    result = np.zeros(int(parent.max()) - smallest + 1)
    for p, v, s in zip(parent, lam, size):
        result[p - smallest] += (v - births[p]) * s
    return {i + smallest: result[i] for i in range(len(result))}


def _bfs_cluster_tree(tp, tc, root):
    out, queue = [], np.array([root], dtype=np.int64)
    while len(queue) > 0:
        out.extend(queue.tolist())
        queue = tc[np.isin(tp, queue)]
    return out


def _leaves(tp, tc, node):
    kids = tc[tp == node]
    if len(kids) == 0:
        return [int(node)]
    return sum([_leaves(tp, tc, k) for k in kids], [])


def _traverse_upwards(tp, tc, tv, epsilon, leaf, allow_single_cluster):
    root = tp.min()
    parent = tp[tc == leaf][0]
    if parent == root:
        return int(parent) if allow_single_cluster else int(leaf)
    with np.errstate(divide="ignore"):
        parent_eps = 1 / tv[tc == parent][0]
    if parent_eps > epsilon:
        return int(parent)
    return _traverse_upwards(tp, tc, tv, epsilon, parent, allow_single_cluster)


def _epsilon_search(leaves, tp, tc, tv, epsilon, allow_single_cluster):
    selected, processed = [], []
    for leaf in leaves:
        with np.errstate(divide="ignore"):
            eps = 1 / tv[tc == leaf][0]
        if eps < epsilon:
            if leaf not in processed:
                up = _traverse_upwards(tp, tc, tv, epsilon, leaf, allow_single_cluster)
                selected.append(up)
                processed.extend(x for x in _bfs_cluster_tree(tp, tc, up) if x != up)
        else:
            selected.append(leaf)
    return set(selected)


def get_clusters(parent, child, lam, size, stability, method="eom", allow_single_cluster=False, epsilon=0.0, max_cluster_size=None):
    node_list = sorted(stability.keys(), reverse=True)
    if not allow_single_cluster:
        node_list = node_list[:-1]
    tree = size > 1
    tp, tc, tv, ts = parent[tree], child[tree], lam[tree], size[tree]
    is_cluster = {c: True for c in node_list}
    n_samples = int(child[size == 1].max()) + 1
    if max_cluster_size is None:
        max_cluster_size = n_samples + 1
    sizes = {int(c): int(s) for c, s in zip(tc, ts)}
    if allow_single_cluster:
        sizes[node_list[-1]] = int(ts[tp == node_list[-1]].sum())
    if method == "eom":
        for node in node_list:
            subtree = np.sum([stability[int(c)] for c in tc[tp == node]])
            if subtree > stability[node] or sizes[node] > max_cluster_size:
                is_cluster[node] = False
                stability[node] = subtree
            else:
                for sub in _bfs_cluster_tree(tp, tc, node):
                    if sub != node:
                        is_cluster[sub] = False
        if epsilon != 0.0 and len(tp) > 0:
            eom = [c for c in is_cluster if is_cluster[c]]
            selected = []
            if len(eom) == 1 and eom[0] == tp.min():
                if allow_single_cluster:
                    selected = eom
            else:
                selected = _epsilon_search(set(eom), tp, tc, tv, epsilon, allow_single_cluster)
            for c in is_cluster:
                is_cluster[c] = c in selected
    else:
        leaves = set(_leaves(tp, tc, tp.min())) if len(tp) else set()
        if len(leaves) == 0:
            for c in is_cluster:
                is_cluster[c] = False
            is_cluster[int(parent.min())] = True
        selected = _epsilon_search(leaves, tp, tc, tv, epsilon, allow_single_cluster) if epsilon != 0.0 else leaves
        for c in is_cluster:
            is_cluster[c] = c in selected
    clusters = {c for c in is_cluster if is_cluster[c]}
    cluster_map = {c: i for i, c in enumerate(sorted(clusters))}
    reverse_map = {i: c for c, i in cluster_map.items()}

    # _do_labelling: sklearn's union-find by rank over the rows whose child is not a selected cluster
    root = int(parent.min())
    up, rank = list(range(int(parent.max()) + 1)), [0] * (int(parent.max()) + 1)

    def find(x):
        if up[x] != x:
            up[x] = find(up[x])
        return up[x]

    for p, c in zip(parent.tolist(), child.tolist()):
        if c not in clusters:
            a, b = find(p), find(c)
            if rank[a] < rank[b]:
                up[a] = b
            elif rank[a] > rank[b]:
                up[b] = a
            else:
                up[b] = a
                rank[a] += 1
    labels = np.empty(root, dtype=np.int64)
    for pt in range(root):
        cl = find(pt)
        label = -1
        if cl != root:
            label = cluster_map[cl]
        elif len(clusters) == 1 and allow_single_cluster:
            point_lambda = lam[child == pt]
            with np.errstate(divide="ignore"):
                threshold = 1 / epsilon if epsilon != 0.0 else lam[parent == cl].max()
            if point_lambda >= threshold:
                label = cluster_map[cl]
        labels[pt] = label

    # get_probabilities with max_lambdas as sklearn runs it (the last run of consecutive rows of a parent wins)
    deaths = np.zeros(int(parent.max()) + 1)
    current, mx = parent[0], lam[0]
    for p, v in zip(parent[1:], lam[1:]):
        if p == current:
            mx = max(mx, v)
        else:
            deaths[current] = mx
            current, mx = p, v
    deaths[current] = mx
    probs = np.zeros(root)
    for c, v in zip(child, lam):
        if c >= root or labels[c] == -1:
            continue
        m = deaths[reverse_map[int(labels[c])]]
        probs[c] = 1.0 if (m == 0.0 or np.isinf(v)) else min(v, m) / m
    return labels, probs


def tree_to_labels(left, right, value, csize, min_cluster_size, method="eom", allow_single_cluster=False, epsilon=0.0, max_cluster_size=None):
    parent, child, lam, size = condense_tree(left, right, value, csize, min_cluster_size)
    return get_clusters(parent, child, lam, size, compute_stability(parent, child, lam, size), method, allow_single_cluster, epsilon, max_cluster_size)


def labelling_at_cut(left, right, value, cut, min_cluster_size):
    n = len(left) + 1
    root = 2 * (n - 1)
    up, rank = list(range(root + 1)), [0] * (root + 1)

    def find(x):
        if up[x] != x:
            up[x] = find(up[x])
        return up[x]

    def union(x, y):
        a, b = find(x), find(y)
        if rank[a] < rank[b]:
            up[a] = b
        elif rank[a] > rank[b]:
            up[b] = a
        else:
            up[b] = a
            rank[a] += 1

    for i in range(n - 1):
        if value[i] < cut:
            union(int(left[i]), n + i)
            union(int(right[i]), n + i)
    rep = np.array([find(i) for i in range(n)])
    out = np.empty(n, dtype=np.int64)
    nxt = 0
    for r in np.unique(rep):
        members = rep == r
        if members.sum() < min_cluster_size:
            out[members] = -1
        else:
            out[members] = nxt
            nxt += 1
    return out


def run_case(case, cur, nxt, dist, row_order):
    """the restatement's host stage of one case on a given spanning tree and edge order -> dict of what the golden stores"""
    left, right, value, csize = single_linkage(cur, nxt, dist, row_order)
    labels, probs = tree_to_labels(left, right, value, csize, case["min_cluster_size"], case["method"], case["allow_single_cluster"], case["epsilon"],
                                   case["max_cluster_size"])
    out = dict(slt_left=left, slt_right=right, slt_value=value, slt_size=csize, labels=labels, probs=probs)
    for i, cut in enumerate(case["cuts"]):
        out["cut%d" % i] = labelling_at_cut(left, right, value, cut, case["min_cluster_size"])
    return out


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
