"""HDBSCAN on MI355X for a precomputed distance matrix -- a look-alike of sklearn 1.7.2 `HDBSCAN(metric='precomputed')`.

The three stages that touch the N x N matrix run on the device (csrc/hdbscan.hip): the NaN / symmetry check, the core distances (one wave
per row) and Prim's spanning tree of the mutual reachability graph (N - 1 strictly sequential steps in ONE workgroup).  They give sklearn's
core distances and its spanning tree -- all three fields of every edge, in Prim order -- bit for bit: like sklearn the matrix is widened to
float64 first, so a float32 or float16 matrix gives the results of its float64 copy.  Unlike sklearn nothing N x N is written: sklearn
overwrites the float64 matrix with the mutual reachability graph (8 N^2 bytes), here the matrix is read in place through its handle.

Everything after the tree works on N-long arrays and stays on the host, restated in numpy and plain Python: the sort of the edges, single
linkage, the condensed tree, the stabilities, the selection ('eom' / 'leaf', `cluster_selection_epsilon`, `max_cluster_size`,
`allow_single_cluster`), the labels and the probabilities, and `dbscan_clustering` (DBSCAN* labels at any cut from one fit).  sklearn is
not imported.

The edges are sorted with `np.argsort`, numpy's default sort, exactly as sklearn sorts them.  That sort is not stable, the edge weights
are heavily tied (a weight is usually somebody's core distance) and the order among equal weights changes the tree and the labels: the
result equals sklearn's on the same machine with the same numpy, and two machines whose numpy sorts ties differently may disagree with
each other just as two sklearn runs on them would.  `_tree_from_mst` takes an explicit `row_order` for callers that need a fixed order.

Input: whatever `cluster.as_handle` takes -- numpy, torch, a `DistHandle` or the `DeviceBackedArray` that `re_ranking` returns (read in
place through the handle's compact form, never materialised in float64) -- except that `+inf` entries and negative entries are let
through, as sklearn's HDBSCAN lets them through.  One GPU only: a row-sharded handle is refused.  Sparse input is refused.
"""
import numbers
import warnings

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

HIERARCHY_dtype = np.dtype([("left_node", np.intp), ("right_node", np.intp), ("value", np.float64), ("cluster_size", np.intp)])
MST_edge_dtype = np.dtype([("current_node", np.int64), ("next_node", np.int64), ("distance", np.float64)])

_ASYMMETRIC = ("The precomputed distance matrix is expected to be symmetric, however its values appear to be asymmetric. Please verify "
               "that the distance matrix was constructed correctly.")
_INF_EDGES = ("The minimum spanning tree contains edge weights with value infinity. Potentially, you are missing too many distances in "
              "the initial distance matrix for the given neighborhood size.")


def _read_back(*tensors):
    """THE blocking host read of a fit: every tensor travels as one DMA copy into pooled page-locked memory behind the queued kernels,
    then one wait.  -> numpy arrays (the tests count the calls of this function)."""
    from . import hostio
    outs = []
    for t in tensors:
        o = hostio.pinned_empty(t.shape, t.dtype)
        o.copy_(t, non_blocking=True)
        outs.append(o)
    torch.cuda.current_stream(tensors[0].device).synchronize()
    return [o.numpy().copy() for o in outs]


# ------------------------------------------------------------------------------------------------------------ parameters
def _is_int(x):
    return isinstance(x, numbers.Integral)


def _is_real(x):
    return isinstance(x, numbers.Real)


def _is_bool(x):
    return isinstance(x, (bool, np.bool_))


def _bad(name, must, value):
    return ValueError("The %r parameter of HDBSCAN must be %s. Got %r instead." % (name, must, value))


def _str_among(options):
    return "a str among {%s}" % ", ".join(repr(o) for o in sorted(options))


def _as_handle(X):
    """cluster.as_handle without its value checks: sklearn's HDBSCAN lets +inf (a missing distance) and negative entries through, and
    its NaN refusal has its own message, raised from the device's count"""
    from . import cluster
    from .rerank import DistHandle
    valid = getattr(X, "valid_handle", None)
    if isinstance(X, DistHandle) or (callable(valid) and isinstance(valid(), DistHandle)):
        return cluster.as_handle(X)
    device = torch.device("cuda", torch.cuda.current_device())
    if isinstance(X, np.ndarray):
        if X.dtype == np.float16:
            return DistHandle(X.shape[0], 1, torch.from_numpy(np.ascontiguousarray(X)).to(device))
        return DistHandle(X.shape[0], 2, torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(device))
    if X.dtype == torch.float16:
        return DistHandle(X.shape[0], 1, X.to(device).contiguous())
    return DistHandle(X.shape[0], 2, X.to(device=device, dtype=torch.float64).contiguous())


# ------------------------------------------------------------------------------------------------------------ the device stages
def _device_counts(h):
    """the check alone (the error path of a min_samples larger than N, where sklearn looks for NaN first) -> (nan, asymmetric)"""
    L = _lib.lib()
    with torch.cuda.device(h.device):
        counts = torch.empty(2, dtype=torch.int64, device=h.device)
        check(L.ssg_hdbscan_check(ptr(h.M), ptr(h.v), h.N, h.mode, h.lambda_value, ptr(counts), stream()), "ssg_hdbscan_check")
        (c,) = _read_back(counts)
    return int(c[0]), int(c[1])


def _device_mst(h, k, alpha, state):
    """check, core distances and Prim on handle `h`, queued behind each other, one blocking read -> (nan, asymmetric, core [N],
    current [N-1], next [N-1], distance [N-1])"""
    N = h.N
    L = _lib.lib()
    dev = h.device
    n2 = (N + 1) & ~1                                                    # (every piece starts on a 16-byte boundary)
    with torch.cuda.device(dev):
        st = stream()
        f = torch.empty(3 * n2, dtype=torch.float64, device=dev)         # core | distance | the loop's state when it lives in global memory
        i = torch.empty(2 + 2 * N, dtype=torch.int64, device=dev)        # counts | current | next
        core, dist, ws = f[:N], f[n2:n2 + N - 1], f[2 * n2:]
        args = (ptr(h.M), ptr(h.v), N, h.mode, h.lambda_value)
        check(L.ssg_hdbscan_check(*args, ptr(i[:2]), st), "ssg_hdbscan_check")
        check(L.ssg_hdbscan_core_dist(*args, k, alpha, ptr(core), st), "ssg_hdbscan_core_dist")
        check(L.ssg_hdbscan_mst(*args, ptr(core), alpha, state, ptr(ws), n2 * 8, ptr(i[2:2 + N - 1]), ptr(i[2 + N:2 + 2 * N - 1]), ptr(dist), st),
              "ssg_hdbscan_mst")
        fh, ih = _read_back(f[:2 * n2], i)                               # one blocking read: the counts and the three edge arrays (and core)
    return int(ih[0]), int(ih[1]), fh[:N].copy(), ih[2:2 + N - 1].copy(), ih[2 + N:2 + 2 * N - 1].copy(), fh[n2:n2 + N - 1].copy()


# ------------------------------------------------------------------------------------------------------------ the host stages
def _single_linkage(current, nxt, distance, row_order=None):
    """_process_mst: the edges sorted by weight (np.argsort, numpy's default sort, unless `row_order` is given), then make_single_linkage:
    a union-find in which the i-th merge gets the id N + i -> structured array [N - 1] of HIERARCHY_dtype"""
    n = len(distance) + 1
    if row_order is None:
        row_order = np.argsort(distance)
    row_order = np.asarray(row_order)
    cur, nx, val = np.asarray(current)[row_order].tolist(), np.asarray(nxt)[row_order].tolist(), np.asarray(distance)[row_order]
    parent = [-1] * (2 * n - 1)
    size = [1] * n + [0] * (n - 1)

    def find(x):
        top = x
        while parent[top] != -1:
            top = parent[top]
        while x != top and parent[x] != top:
            x, parent[x] = parent[x], top
        return top

    out = np.zeros(n - 1, dtype=HIERARCHY_dtype)
    left, right, csize = [0] * (n - 1), [0] * (n - 1), [0] * (n - 1)
    for i in range(n - 1):
        a, b = find(cur[i]), find(nx[i])
        left[i], right[i], csize[i] = a, b, size[a] + size[b]
        parent[a] = parent[b] = n + i
        size[n + i] = csize[i]
    out["left_node"], out["right_node"], out["value"], out["cluster_size"] = left, right, val, csize
    return out


def _bfs_hierarchy(left, right, n, root):
    out, queue = [], [root]
    while queue:
        out.extend(queue)
        nxt = []
        for x in queue:
            if x >= n:
                nxt.append(left[x - n])
                nxt.append(right[x - n])
        queue = nxt
    return out


def _condense_tree(tree, min_cluster_size):
    """_condense_tree: walk the hierarchy from the root breadth first; a split whose two sides both hold min_cluster_size points makes two
    new clusters, a smaller side falls out of its parent point by point at lambda = 1 / distance -> (parent, child, lambda, size) lists"""
    left, right = tree["left_node"].tolist(), tree["right_node"].tolist()
    value, csize = tree["value"].tolist(), tree["cluster_size"].tolist()
    n = len(left) + 1
    root = 2 * (n - 1)
    next_label = n + 1
    relabel = [0] * (root + 1)
    relabel[root] = n
    ignore = [False] * (root + 1)
    P, C, V, S = [], [], [], []

    def fall_out(sub_root, label, lam):
        for sub in _bfs_hierarchy(left, right, n, sub_root):
            if sub < n:
                P.append(label); C.append(sub); V.append(lam); S.append(1)
            ignore[sub] = True

    for node in _bfs_hierarchy(left, right, n, root):
        if ignore[node] or node < n:
            continue
        lt, rt, d = left[node - n], right[node - n], value[node - n]
        lam = 1.0 / d if d > 0.0 else np.inf
        lc = csize[lt - n] if lt >= n else 1
        rc = csize[rt - n] if rt >= n else 1
        if lc >= min_cluster_size and rc >= min_cluster_size:
            relabel[lt] = next_label
            next_label += 1
            P.append(relabel[node]); C.append(relabel[lt]); V.append(lam); S.append(lc)
            relabel[rt] = next_label
            next_label += 1
            P.append(relabel[node]); C.append(relabel[rt]); V.append(lam); S.append(rc)
        elif lc < min_cluster_size and rc < min_cluster_size:
            fall_out(lt, relabel[node], lam)
            fall_out(rt, relabel[node], lam)
        elif lc < min_cluster_size:
            relabel[rt] = relabel[node]
            fall_out(lt, relabel[node], lam)
        else:
            relabel[lt] = relabel[node]
            fall_out(rt, relabel[node], lam)
    return P, C, V, S


def _compute_stability(P, C, V, S):
    """sum over the rows of a cluster of (lambda - birth of the cluster) * size, accumulated in row order"""
    smallest = min(P)
    births = {c: v for c, v in zip(C, V)}
    births[smallest] = 0.0
    result = [0.0] * (max(P) - smallest + 1)
    for p, v, s in zip(P, V, S):
        result[p - smallest] += (v - births.get(p, np.nan)) * s
    return {i + smallest: result[i] for i in range(len(result))}


def _get_clusters(P, C, V, S, stability, method, allow_single_cluster, epsilon, max_cluster_size):
    """_get_clusters: the selection, then _do_labelling and get_probabilities -> (labels int64 [N], probabilities float64 [N])"""
    node_list = sorted(stability.keys(), reverse=True)
    if not allow_single_cluster:
        node_list = node_list[:-1]                                       # (without the root)
    tree_rows = [r for r in range(len(P)) if S[r] > 1]                   # the cluster tree: the rows whose child is a cluster
    tP, tC, tV, tS = [P[r] for r in tree_rows], [C[r] for r in tree_rows], [V[r] for r in tree_rows], [S[r] for r in tree_rows]
    kids = {}
    for p, c in zip(tP, tC):
        kids.setdefault(p, []).append(c)
    row_of = {c: r for r, c in enumerate(tC)}                            # a cluster is the child of exactly one row
    is_cluster = {c: True for c in node_list}
    n_samples = max(c for c, s in zip(C, S) if s == 1) + 1
    if max_cluster_size is None:
        max_cluster_size = n_samples + 1
    sizes = dict(zip(tC, tS))
    root = min(P)
    if allow_single_cluster:
        sizes[node_list[-1]] = sum(s for p, s in zip(tP, tS) if p == node_list[-1])

    def below(node):
        out, queue = [], [node]
        while queue:
            out.extend(queue)
            queue = [c for x in queue for c in kids.get(x, ())]
        return out

    def traverse_upwards(leaf):
        parent = tP[row_of[leaf]]
        if parent == root:
            return parent if allow_single_cluster else leaf              # the node closest to the root
        with np.errstate(divide="ignore"):
            parent_eps = 1 / np.float64(tV[row_of[parent]])
        return parent if parent_eps > epsilon else traverse_upwards(parent)

    def epsilon_search(leaves):
        selected, processed = [], set()
        for leaf in leaves:
            with np.errstate(divide="ignore"):
                eps = 1 / np.float64(tV[row_of[leaf]])
            if eps < epsilon:
                if leaf not in processed:
                    up = traverse_upwards(leaf)
                    selected.append(up)
                    processed.update(x for x in below(up) if x != up)
            else:
                selected.append(leaf)
        return set(selected)

    if method == "eom":
        for node in node_list:
            subtree = np.sum([stability[c] for c in kids.get(node, ())])
            if subtree > stability[node] or sizes[node] > max_cluster_size:
                is_cluster[node] = False
                stability[node] = subtree
            else:
                for sub in below(node):
                    if sub != node:
                        is_cluster[sub] = False
        if epsilon != 0.0 and len(tP) > 0:
            eom = [c for c in is_cluster if is_cluster[c]]
            selected = []
            if len(eom) == 1 and eom[0] == min(tP):                      # only the root: no epsilon search
                if allow_single_cluster:
                    selected = eom
            else:
                selected = epsilon_search(set(eom))
            for c in is_cluster:
                is_cluster[c] = c in selected
    else:
        leaves = set()
        if tP:
            stack = [min(tP)]
            while stack:
                x = stack.pop()
                if x in kids:
                    stack.extend(kids[x])
                else:
                    leaves.add(x)
        if len(leaves) == 0:
            for c in is_cluster:
                is_cluster[c] = False
            is_cluster[root] = True
        selected = epsilon_search(leaves) if epsilon != 0.0 else leaves
        for c in is_cluster:
            is_cluster[c] = c in selected

    clusters = {c for c in is_cluster if is_cluster[c]}
    cluster_map = {c: i for i, c in enumerate(sorted(clusters))}
    reverse_map = {i: c for c, i in cluster_map.items()}

    # _do_labelling: a point belongs to the first selected cluster on its way up (a union-find whose representative is the top node)
    top = {}
    for p, c in zip(P, C):
        if c not in clusters:
            top[c] = top.get(p, p)
    row_of_point = {}
    max_lambda_under = {}
    if len(clusters) == 1 and allow_single_cluster:
        row_of_point = {c: r for r, c in enumerate(C)}
        for p, v in zip(P, V):
            if p not in max_lambda_under or v > max_lambda_under[p]:
                max_lambda_under[p] = v
    labels = np.empty(root, dtype=np.intp)
    for pt in range(root):
        cl = top.get(pt, pt)
        label = -1
        if cl != root:
            label = cluster_map[cl]
        elif len(clusters) == 1 and allow_single_cluster:
            with np.errstate(divide="ignore"):
                threshold = 1 / np.float64(epsilon) if epsilon != 0.0 else max_lambda_under[cl]
            if V[row_of_point[pt]] >= threshold:
                label = cluster_map[cl]
        labels[pt] = label

    # get_probabilities; max_lambdas keeps, per cluster, the maximum of the LAST run of consecutive rows of that parent
    deaths = {}
    current_parent, max_lambda = P[0], V[0]
    for p, v in zip(P[1:], V[1:]):
        if p == current_parent:
            max_lambda = max(max_lambda, v)
        else:
            deaths[current_parent] = max_lambda
            current_parent, max_lambda = p, v
    deaths[current_parent] = max_lambda
    probs = np.zeros(root, dtype=np.float64)
    for c, v in zip(C, V):
        if c >= root or labels[c] == -1:
            continue
        mx = deaths.get(reverse_map[int(labels[c])], 0.0)
        probs[c] = 1.0 if (mx == 0.0 or np.isinf(v)) else min(v, mx) / mx
    return labels, probs


def tree_to_labels(single_linkage_tree, min_cluster_size=10, cluster_selection_method="eom", allow_single_cluster=False,
                   cluster_selection_epsilon=0.0, max_cluster_size=None):
    """sklearn.cluster._hdbscan._tree.tree_to_labels -> (labels_, probabilities_)"""
    P, C, V, S = _condense_tree(single_linkage_tree, int(min_cluster_size))
    return _get_clusters(P, C, V, S, _compute_stability(P, C, V, S), cluster_selection_method, bool(allow_single_cluster),
                         float(cluster_selection_epsilon), max_cluster_size)


def labelling_at_cut(linkage, cut, min_cluster_size):
    """sklearn.cluster._hdbscan._tree.labelling_at_cut: the components of the merges below `cut`; a component smaller than
    min_cluster_size is noise; labels follow the ids of the components' representatives (a union-find by rank, as sklearn's)"""
    n = len(linkage) + 1
    root = 2 * (n - 1)
    up, rank = list(range(root + 1)), [0] * (root + 1)

    def find(x):
        top = x
        while up[top] != top:
            top = up[top]
        while up[x] != top:
            x, up[x] = up[x], top
        return top

    def union(x, y):
        a, b = find(x), find(y)
        if rank[a] < rank[b]:
            up[a] = b
        elif rank[a] > rank[b]:
            up[b] = a
        else:
            up[b] = a
            rank[a] += 1

    cluster = n
    for lt, rt, v in zip(linkage["left_node"].tolist(), linkage["right_node"].tolist(), linkage["value"].tolist()):
        if v < cut:
            union(lt, cluster)
            union(rt, cluster)
        cluster += 1
    rep = [find(i) for i in range(n)]
    count = {}
    for r in rep:
        count[r] = count.get(r, 0) + 1
    label_of, nxt = {}, 0
    for r in sorted(count):
        if count[r] < min_cluster_size:
            label_of[r] = -1
        else:
            label_of[r] = nxt
            nxt += 1
    return np.array([label_of[r] for r in rep], dtype=np.intp)


def _tree_from_mst(current, nxt, distance, min_cluster_size, cluster_selection_method="eom", allow_single_cluster=False,
                   cluster_selection_epsilon=0.0, max_cluster_size=None, row_order=None):
    """the whole host stage: the spanning tree in Prim order -> (_single_linkage_tree_, labels_, probabilities_).  `row_order`: the order
    in which the edges are merged; default `np.argsort(distance)`, numpy's default (unstable) sort, which is what sklearn calls"""
    tree = _single_linkage(current, nxt, distance, row_order)
    labels, probs = tree_to_labels(tree, min_cluster_size, cluster_selection_method, allow_single_cluster, cluster_selection_epsilon, max_cluster_size)
    return tree, labels, probs


# ------------------------------------------------------------------------------------------------------------ the estimator
class HDBSCAN:
    """sklearn.cluster.HDBSCAN (1.7.2) look-alike for metric='precomputed' running on the GPU: the same constructor arguments and
    defaults, `fit`, `fit_predict`, `dbscan_clustering`, `labels_`, `probabilities_`, `_single_linkage_tree_`, `_min_samples` and
    `n_features_in_`, the same errors and the same warning.  Any other metric raises.  `metric_params`, `algorithm`, `leaf_size` and
    `n_jobs` are accepted and ignored.  `copy` is accepted and has no effect, because the input is never modified -- sklearn with its
    default `copy=False` overwrites the caller's matrix with the mutual reachability graph.  One GPU only.  The class attribute `state`
    (0 auto, 1 LDS, 2 global memory) places the state of the spanning-tree loop; every placement gives the same result."""

    state = 0

    def __init__(self, min_cluster_size=5, min_samples=None, cluster_selection_epsilon=0.0, max_cluster_size=None, metric="euclidean",
                 metric_params=None, alpha=1.0, algorithm="auto", leaf_size=40, n_jobs=None, cluster_selection_method="eom",
                 allow_single_cluster=False, store_centers=None, copy=False):
        self.min_cluster_size, self.min_samples, self.alpha, self.max_cluster_size = min_cluster_size, min_samples, alpha, max_cluster_size
        self.cluster_selection_epsilon, self.metric, self.metric_params, self.algorithm = cluster_selection_epsilon, metric, metric_params, algorithm
        self.leaf_size, self.n_jobs, self.cluster_selection_method, self.allow_single_cluster = leaf_size, n_jobs, cluster_selection_method, allow_single_cluster
        self.store_centers, self.copy = store_centers, copy

    def _validate(self):
        """sklearn's _parameter_constraints, checked in its order (the parameter names sorted); InvalidParameterError is a ValueError"""
        if not (isinstance(self.algorithm, str) and self.algorithm in ("auto", "brute", "kd_tree", "ball_tree")):
            raise _bad("algorithm", _str_among(("auto", "brute", "kd_tree", "ball_tree")), self.algorithm)
        if not _is_bool(self.allow_single_cluster):
            raise _bad("allow_single_cluster", "an instance of 'bool' or an instance of 'numpy.bool'", self.allow_single_cluster)
        if not _is_real(self.alpha) or not 0.0 < self.alpha < np.inf:
            raise _bad("alpha", "a float in the range (0.0, inf)", self.alpha)
        if not _is_real(self.cluster_selection_epsilon) or not self.cluster_selection_epsilon >= 0:
            raise _bad("cluster_selection_epsilon", "a float in the range [0.0, inf)", self.cluster_selection_epsilon)
        if not (isinstance(self.cluster_selection_method, str) and self.cluster_selection_method in ("eom", "leaf")):
            raise _bad("cluster_selection_method", _str_among(("eom", "leaf")), self.cluster_selection_method)
        if not _is_bool(self.copy):
            raise _bad("copy", "an instance of 'bool' or an instance of 'numpy.bool'", self.copy)
        if not _is_int(self.leaf_size) or self.leaf_size < 1:
            raise _bad("leaf_size", "an int in the range [1, inf)", self.leaf_size)
        if self.max_cluster_size is not None and (not _is_int(self.max_cluster_size) or self.max_cluster_size < 1):
            raise _bad("max_cluster_size", "None or an int in the range [1, inf)", self.max_cluster_size)
        if self.metric != "precomputed":
            raise ValueError("ssg_amd.hdbscan.HDBSCAN implements metric='precomputed' only (the SSG grouping path clusters a precomputed "
                             "re-rank distance); got metric=%r" % (self.metric,))
        if self.metric_params is not None and not isinstance(self.metric_params, dict):
            raise _bad("metric_params", "an instance of 'dict' or None", self.metric_params)
        if not _is_int(self.min_cluster_size) or self.min_cluster_size < 2:
            raise _bad("min_cluster_size", "an int in the range [2, inf)", self.min_cluster_size)
        if self.min_samples is not None and (not _is_int(self.min_samples) or self.min_samples < 1):
            raise _bad("min_samples", "an int in the range [1, inf) or None", self.min_samples)
        if self.n_jobs is not None and not _is_int(self.n_jobs):
            raise _bad("n_jobs", "an instance of 'int' or None", self.n_jobs)
        if self.store_centers is not None and not (isinstance(self.store_centers, str) and self.store_centers in ("centroid", "medoid", "both")):
            raise _bad("store_centers", "None or " + _str_among(("centroid", "medoid", "both")), self.store_centers)

    def fit(self, X, y=None):
        from . import cluster
        from .rerank import DistHandle
        self._validate()
        if self.store_centers is not None:
            raise ValueError("Cannot store centers when using a precomputed distance matrix.")
        if hasattr(X, "tocsr") or hasattr(X, "todense"):
            raise TypeError("ssg_amd.hdbscan.HDBSCAN takes a dense precomputed distance matrix; sparse input is not supported")
        min_samples = int(self.min_cluster_size if self.min_samples is None else self.min_samples)
        valid = getattr(X, "valid_handle", None)
        is_handle = isinstance(X, DistHandle) or (callable(valid) and isinstance(valid(), DistHandle))
        if not is_handle:
            if not isinstance(X, np.ndarray) and not torch.is_tensor(X):
                raise TypeError("unsupported distance matrix type %r" % type(X))
            shape = tuple(int(s) for s in X.shape)
            if len(shape) != 2:
                raise ValueError("Expected 2D array, got %dD array instead" % len(shape))
            if shape[0] != shape[1] or shape[0] == 1:
                # nothing here reaches the device: sklearn's refusals of such an input, in its order
                if bool(np.isnan(X).any() if isinstance(X, np.ndarray) else torch.isnan(X).any()):
                    raise ValueError("np.nan values found in precomputed-dense")
                if shape[0] == 1:
                    raise ValueError("n_samples=1 while HDBSCAN requires more than one sample")
                self._min_samples = min_samples
                if min_samples > shape[0]:
                    raise ValueError("min_samples (%d) must be at most the number of samples in X (%d)" % (min_samples, shape[0]))
                raise ValueError("The precomputed distance matrix is expected to be symmetric, however it has shape %r. Please verify that "
                                 "the distance matrix was constructed correctly." % (shape,))
        h = _as_handle(X)
        if hasattr(h, "validate"):
            h.validate()
        if h.group is not None or h.row0 != 0 or h.nrows != h.N:
            raise ValueError("HDBSCAN runs on a single GPU: a row-sharded DistHandle is not supported")
        if h.N == 1:
            raise ValueError("n_samples=1 while HDBSCAN requires more than one sample")
        self._min_samples = min_samples
        if min_samples > h.N:
            if _device_counts(h)[0]:
                raise ValueError("np.nan values found in precomputed-dense")
            raise ValueError("min_samples (%d) must be at most the number of samples in X (%d)" % (min_samples, h.N))
        nan, asym, core, cur, nxt, dist = _device_mst(h, min_samples, float(self.alpha), int(self.state))
        if nan:
            raise ValueError("np.nan values found in precomputed-dense")
        if asym:
            raise ValueError(_ASYMMETRIC)
        if np.isinf(dist).any():
            warnings.warn(_INF_EDGES, UserWarning)
        self._core_distances, self._mst = core, (cur, nxt, dist)
        self.n_features_in_ = h.N
        self._single_linkage_tree_, self.labels_, self.probabilities_ = _tree_from_mst(
            cur, nxt, dist, self.min_cluster_size, self.cluster_selection_method, self.allow_single_cluster, self.cluster_selection_epsilon,
            self.max_cluster_size)
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def dbscan_clustering(self, cut_distance, min_cluster_size=5):
        """DBSCAN* labels (DBSCAN without the border points) at `cut_distance` from the fitted single-linkage tree; components smaller
        than `min_cluster_size` are noise"""
        return labelling_at_cut(self._single_linkage_tree_, float(cut_distance), int(min_cluster_size))
