"""Agglomerative clustering on MI355X for a precomputed distance matrix -- a look-alike of sklearn 1.7.2
`AgglomerativeClustering(metric='precomputed', connectivity=None, linkage='average' | 'complete' | 'single')`.

sklearn hands the condensed upper triangle of the matrix to scipy's `linkage`; the three stages that touch the N x N matrix run on the
device instead (csrc/agglomerative.hip): the NaN / inf check, the float64 working square W built from the upper triangle alone, and the
merge loop -- scipy's `nn_chain` for average and complete linkage, its `mst_single_linkage` for single linkage -- N - 1 strictly
sequential merges in ONE workgroup.  They give scipy's merges (both slots, the height, the size) in merge order bit for bit: like scipy
the matrix is widened to float64 first, so a float32 or float16 matrix gives the results of its float64 copy.  Only the strict upper
triangle counts: the diagonal and the lower triangle are never looked at, no symmetry check is made, negative entries pass.

Everything after the merges works on N-long arrays and stays on the host, restated in numpy and plain Python: the STABLE sort of the
merges by height (scipy's `kind='mergesort'`; unlike HDBSCAN's edge sort the result does not depend on the machine's numpy), scipy's
`label` pass (a union-find in row order; merge i gets the id N + i), and sklearn's `_hc_cut` (a heap walk from the root).  sklearn and
scipy are not imported.

Input: whatever `cluster.as_handle` takes -- numpy, torch, a `DistHandle` or the `DeviceBackedArray` that `re_ranking` returns (read in
place through the handle's compact form; the input is never modified).  The working square costs 8 N^2 bytes on the device (2 GB at
N = 16 000); nothing N x N reaches the host.  One GPU only: a row-sharded handle is refused.
"""
import heapq
import numbers

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from .hdbscan import _as_handle, _read_back

_METHODS = {"average": 0, "complete": 1, "single": 2}
_LINKAGES = ("ward", "complete", "average", "single")
_METRICS = ("braycurtis", "canberra", "chebyshev", "cityblock", "correlation", "cosine", "dice", "euclidean", "hamming", "haversine", "jaccard",
            "l1", "l2", "mahalanobis", "manhattan", "matching", "minkowski", "nan_euclidean", "precomputed", "rogerstanimoto", "russellrao",
            "seuclidean", "sokalmichener", "sokalsneath", "sqeuclidean", "wminkowski", "yule")
_NAN = ("Input X contains NaN.\nAgglomerativeClustering does not accept missing values encoded as NaN natively. For supervised learning, you might want to "
        "consider sklearn.ensemble.HistGradientBoostingClassifier and Regressor which accept missing values encoded as NaNs natively. Alternatively, it is "
        "possible to preprocess the data, for instance by using an imputer transformer in a pipeline or drop samples with missing values. See "
        "https://scikit-learn.org/stable/modules/impute.html You can find a list of all estimators that handle NaN values at the following page: "
        "https://scikit-learn.org/stable/modules/impute.html#estimators-that-handle-nan-values")
_INF = "Input X contains infinity or a value too large for dtype('%s')."
_ONE_OF = "Exactly one of n_clusters and distance_threshold has to be set, and the other needs to be None."
_FULL_TREE = "compute_full_tree must be True if distance_threshold is set."


# ------------------------------------------------------------------------------------------------------------ the device stages
def _device_counts(h):
    """the check alone (the error paths on which sklearn looks at the values of X before it refuses a parameter) -> (nan, inf)"""
    L = _lib.lib()
    with torch.cuda.device(h.device):
        counts = torch.empty(2, dtype=torch.int64, device=h.device)
        check(L.ssg_agglo_check(ptr(h.M), ptr(h.v), h.N, h.mode, h.lambda_value, ptr(counts), stream()), "ssg_agglo_check")
        (c,) = _read_back(counts)
    return int(c[0]), int(c[1])


def _device_merges(h, method, state=0):
    """check, expand and the merge loop on handle `h`, queued behind each other, one blocking read -> (nan, inf, flag, scans, x [N-1],
    y [N-1], distance [N-1], size [N-1]) in merge order.  The outputs keep their sentinels (-1, NaN) when the loop returned early."""
    N = h.N
    L = _lib.lib()
    dev = h.device
    n1, n4 = N - 1, (N + 3) & ~3
    with torch.cuda.device(dev):
        st = stream()
        W = torch.empty((N, n4), dtype=torch.float64, device=dev)        # the working square, rows 32-byte aligned
        i = torch.full((4 + 3 * n1,), -1, dtype=torch.int64, device=dev)  # counts | flag, scans | x | y | size
        f = torch.full((n1,), float("nan"), dtype=torch.float64, device=dev)
        ws = torch.empty(n4, dtype=torch.float64, device=dev)            # the loop's state when it lives in global memory
        check(L.ssg_agglo_check(ptr(h.M), ptr(h.v), N, h.mode, h.lambda_value, ptr(i[:2]), st), "ssg_agglo_check")
        check(L.ssg_agglo_expand(ptr(h.M), ptr(h.v), N, h.mode, h.lambda_value, ptr(W), n4, st), "ssg_agglo_expand")
        check(L.ssg_agglo_nn_chain(ptr(W), N, n4, method, state, ptr(i[:2]), ptr(ws), n4 * 8, ptr(i[4:4 + n1]), ptr(i[4 + n1:4 + 2 * n1]), ptr(f),
                                   ptr(i[4 + 2 * n1:]), ptr(i[2:4]), st), "ssg_agglo_nn_chain")
        fh, ih = _read_back(f, i)                                        # one blocking read: the counts, the flag and the four merge arrays
    return (int(ih[0]), int(ih[1]), int(ih[2]), int(ih[3]), ih[4:4 + n1].copy(), ih[4 + n1:4 + 2 * n1].copy(), fh, ih[4 + 2 * n1:].copy())


# ------------------------------------------------------------------------------------------------------------ the host stages
def _label(x, y, distance):
    """scipy's linkage after its loop: the merges sorted by height with a stable sort, then `label`: a union-find in row order; row i
    gets the two roots, the smaller first, the merged cluster the id N + i and its size column 3 -> Z [N - 1, 4] float64"""
    n = len(distance) + 1
    order = np.argsort(np.asarray(distance), kind="stable")
    xs, ys = np.asarray(x)[order].tolist(), np.asarray(y)[order].tolist()
    parent = [-1] * (2 * n - 1)
    size = [1] * n + [0] * (n - 1)

    def find(a):
        top = a
        while parent[top] != -1:
            top = parent[top]
        while parent[a] != -1 and parent[a] != top:
            nxt = parent[a]
            parent[a] = top
            a = nxt
        return top

    Z = np.empty((n - 1, 4), dtype=np.float64)
    lo, hi, sz = [0] * (n - 1), [0] * (n - 1), [0] * (n - 1)
    for i in range(n - 1):
        a, b = find(xs[i]), find(ys[i])
        lo[i], hi[i] = (a, b) if a < b else (b, a)
        parent[a] = parent[b] = n + i
        size[n + i] = sz[i] = size[a] + size[b]
    Z[:, 0], Z[:, 1], Z[:, 2], Z[:, 3] = lo, hi, np.asarray(distance)[order], sz
    return Z


def _hc_cut(n_clusters, children, n_leaves):
    """sklearn.cluster._agglomerative._hc_cut: a heap walk from the root that opens the youngest node n_clusters - 1 times; the labels
    follow the positions in the heap list, the leaves of a node are found as _hc_get_descendent finds them"""
    if n_clusters > n_leaves:
        raise ValueError("Cannot extract more clusters than samples: %s clusters were given for a tree with %s leaves." % (n_clusters, n_leaves))
    kids = np.asarray(children).tolist()
    nodes = [-(max(kids[-1]) + 1)]
    for _ in range(n_clusters - 1):
        these = kids[-nodes[0] - n_leaves]
        heapq.heappush(nodes, -these[0])
        heapq.heappushpop(nodes, -these[1])
    label = np.zeros(n_leaves, dtype=np.intp)
    for i, node in enumerate(nodes):
        ind, leaves = [-node], []
        while ind:
            t = ind.pop()
            if t < n_leaves:
                leaves.append(t)
            else:
                ind.extend(kids[t - n_leaves])
        label[leaves] = i
    return label


def _drop_small(labels, min_cluster_size):
    """the small-cluster rule of generate_selflabel_agglomerative: clusters of fewer than min_cluster_size samples become -1, the others
    are renumbered 0 .. k - 1 in order of first appearance"""
    labels = np.asarray(labels)
    count = np.bincount(labels, minlength=int(labels.max()) + 1 if len(labels) else 0)
    out, new = np.full(len(labels), -1, dtype=np.intp), {}
    for i, l in enumerate(labels.tolist()):
        if count[l] >= min_cluster_size:
            out[i] = new.setdefault(l, len(new))
    return out


def _merges(X, method, state=0):
    """the input checks and the device stages -> (handle, x, y, distance, size) in merge order"""
    from .rerank import DistHandle
    if hasattr(X, "tocsr") or hasattr(X, "todense"):
        raise TypeError("ssg_amd.agglomerative takes a dense precomputed distance matrix; sparse input is not supported")
    valid = getattr(X, "valid_handle", None)
    is_handle = isinstance(X, DistHandle) or (callable(valid) and isinstance(valid(), DistHandle))
    dtype = "float64"
    if not is_handle:
        if not isinstance(X, np.ndarray) and not torch.is_tensor(X):
            raise TypeError("unsupported distance matrix type %r" % type(X))
        shape = tuple(int(s) for s in X.shape)
        if len(shape) != 2:
            raise ValueError("Expected 2D array, got %dD array instead" % len(shape))
        if str(X.dtype).replace("torch.", "") in ("float16", "float32"):
            dtype = str(X.dtype).replace("torch.", "")
        if shape[0] != shape[1] or shape[0] < 2:
            # nothing here reaches the device: sklearn's refusals of such an input, in its order
            if bool(np.isnan(X).any() if isinstance(X, np.ndarray) else torch.isnan(X).any()):
                raise ValueError(_NAN)
            if bool(np.isinf(X).any() if isinstance(X, np.ndarray) else torch.isinf(X).any()):
                raise ValueError(_INF % dtype)
            if shape[0] < 2:
                raise ValueError("Found array with %d sample(s) (shape=%s) while a minimum of 2 is required by AgglomerativeClustering." % (shape[0], shape))
            raise ValueError("Distance matrix should be square, got matrix of shape %s" % (shape,))
    h = _as_handle(X)
    if hasattr(h, "validate"):
        h.validate()
    if h.group is not None or h.row0 != 0 or h.nrows != h.N:
        raise ValueError("AgglomerativeClustering runs on a single GPU: a row-sharded DistHandle is not supported")
    if h.N < 2:
        raise ValueError("Found array with %d sample(s) (shape=%s) while a minimum of 2 is required by AgglomerativeClustering." % (h.N, (h.N, h.N)))
    if method is None:                                                   # a parameter error is pending: sklearn has looked at X before it
        nan, inf = _device_counts(h)
        flag = 0
        x = y = d = s = None
    else:
        nan, inf, flag, _, x, y, d, s = _device_merges(h, method, state)
    if nan:
        raise ValueError(_NAN)
    if inf:
        raise ValueError(_INF % dtype)
    if flag:
        raise RuntimeError("ssg_agglo_nn_chain stopped with flag %d (1: the bound of 3 (N - 1) scans was reached; 2: a scan found no live slot)" % flag)
    return h, x, y, d, s


def linkage(X, method="average", state=0):
    """scipy.cluster.hierarchy.linkage(squareform-of-the-upper-triangle(X), method) for method 'average', 'complete' or 'single' ->
    Z [N - 1, 4] float64"""
    if method not in _METHODS:
        raise ValueError("ssg_amd.agglomerative.linkage implements the methods %s, got %r" % (sorted(_METHODS), method))
    _, x, y, d, _ = _merges(X, _METHODS[method], int(state))
    return _label(x, y, d)


# ------------------------------------------------------------------------------------------------------------ the estimator
def _bad(name, must, value):
    return ValueError("The %r parameter of AgglomerativeClustering must be %s. Got %r instead." % (name, must, value))


def _is_bool(x):
    return isinstance(x, (bool, np.bool_))


class AgglomerativeClustering:
    """sklearn.cluster.AgglomerativeClustering (1.7.2) look-alike for metric='precomputed', connectivity=None and linkage 'average',
    'complete' or 'single' running on the GPU: the same constructor arguments and defaults, `fit`, `fit_predict`, `children_`,
    `distances_`, `n_clusters_`, `n_leaves_`, `n_connected_components_`, `n_features_in_` and `labels_`, the same errors in the same
    order.  Any other metric and any connectivity raise.  `memory` and `pooling_func` are accepted and ignored.  With connectivity=None
    sklearn always builds the full tree, so `compute_full_tree` only takes part in validation.  One GPU only.  The class attribute
    `state` (0 auto, 1 LDS, 2 global memory) places the state of the merge loop; every placement gives the same result."""

    state = 0

    def __init__(self, n_clusters=2, *, metric="euclidean", memory=None, connectivity=None, compute_full_tree="auto", linkage="ward",
                 distance_threshold=None, compute_distances=False, pooling_func="deprecated"):
        self.n_clusters, self.distance_threshold, self.memory, self.connectivity = n_clusters, distance_threshold, memory, connectivity
        self.compute_full_tree, self.linkage, self.metric, self.compute_distances = compute_full_tree, linkage, metric, compute_distances
        self.pooling_func = pooling_func

    def _validate(self):
        """sklearn's _parameter_constraints, checked in its order; InvalidParameterError is a ValueError.  (sklearn prints the options of
        a str parameter in the order of a Python set; here they are sorted.)"""
        if self.n_clusters is not None and (not isinstance(self.n_clusters, numbers.Integral) or self.n_clusters < 1):
            raise _bad("n_clusters", "an int in the range [1, inf) or None", self.n_clusters)
        if not callable(self.metric) and not (isinstance(self.metric, str) and self.metric in _METRICS):
            raise _bad("metric", "a str among {%s} or a callable" % ", ".join(repr(o) for o in _METRICS), self.metric)
        if self.memory is not None and not isinstance(self.memory, str) and not hasattr(self.memory, "cache"):
            raise _bad("memory", "an instance of 'str', an object implementing 'cache' or None", self.memory)
        c = self.connectivity
        if c is not None and not callable(c) and not hasattr(c, "tocsr") and not (
                (hasattr(c, "__len__") or hasattr(c, "shape") or hasattr(c, "__array__")) and not isinstance(c, str)):
            raise _bad("connectivity", "an array-like, a sparse matrix, a callable or None", c)
        if not (isinstance(self.compute_full_tree, str) and self.compute_full_tree == "auto") and not _is_bool(self.compute_full_tree):
            raise _bad("compute_full_tree", "a str among {'auto'} or an instance of 'bool' or an instance of 'numpy.bool'", self.compute_full_tree)
        if not (isinstance(self.linkage, str) and self.linkage in _LINKAGES):
            raise _bad("linkage", "a str among {%s}" % ", ".join(repr(o) for o in sorted(_LINKAGES)), self.linkage)
        t = self.distance_threshold
        if t is not None and (not isinstance(t, numbers.Real) or not t >= 0):
            raise _bad("distance_threshold", "a float in the range [0.0, inf) or None", t)
        if not _is_bool(self.compute_distances):
            raise _bad("compute_distances", "an instance of 'bool' or an instance of 'numpy.bool'", self.compute_distances)

    def _fit_errors(self):
        """the refusals of sklearn's _fit, which it makes after it has validated X -> the first that applies, or None"""
        if not ((self.n_clusters is None) ^ (self.distance_threshold is None)):
            return ValueError(_ONE_OF)
        if self.distance_threshold is not None and not self.compute_full_tree:
            return ValueError(_FULL_TREE)
        if self.linkage == "ward" and self.metric != "euclidean":
            return ValueError("%s was provided as metric. Ward can only work with euclidean distances." % (self.metric,))
        if self.metric != "precomputed" or self.connectivity is not None or self.linkage == "ward":
            return ValueError("ssg_amd.agglomerative.AgglomerativeClustering implements the precomputed, unconstrained case only "
                              "(metric='precomputed', connectivity=None, linkage 'average', 'complete' or 'single'); got metric=%r, connectivity %s, "
                              "linkage=%r" % (self.metric, "None" if self.connectivity is None else "given", self.linkage))
        return None

    def fit(self, X, y=None):
        self._validate()
        err = self._fit_errors()
        h, mx, my, md, _ = _merges(X, None if err is not None else _METHODS[self.linkage], int(self.state))
        self.n_features_in_ = h.N
        if err is not None:
            raise err
        Z = _label(mx, my, md)
        self.children_ = Z[:, :2].astype(int)
        self.n_connected_components_, self.n_leaves_ = 1, h.N
        if self.distance_threshold is not None or self.compute_distances:
            self.distances_ = Z[:, 2].copy()
        if self.distance_threshold is not None:
            self.n_clusters_ = int(np.count_nonzero(Z[:, 2] >= self.distance_threshold)) + 1
        else:
            self.n_clusters_ = self.n_clusters
        self.labels_ = _hc_cut(self.n_clusters_, self.children_, self.n_leaves_)
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_
