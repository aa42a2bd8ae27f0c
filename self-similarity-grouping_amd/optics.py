"""OPTICS on MI355X for a precomputed distance matrix -- a look-alike of sklearn 1.7.2 `OPTICS(metric='precomputed')`.

The ordering (core distances, then N strictly sequential steps of O(N) work) runs on the device (csrc/optics.hip: one wave per row for
the core distances, ONE workgroup for the loop) and gives sklearn's `ordering_`, `core_distances_`, `reachability_` and `predecessor_`
bit for bit: like sklearn the matrix is widened to float64 first -- a float32 or float16 matrix gives the results of its float64 copy --
and every core distance and candidate reachability goes through `np.around(., 15)`.  The two label extractions (`cluster_optics_dbscan`:
DBSCAN-like labels at any eps from one ordering; `cluster_optics_xi`: labels with no eps at all) work on four N-long arrays and stay on
the host, restated in numpy: sklearn is not imported.

Input: whatever `cluster.as_handle` takes -- numpy, torch, a `DistHandle` or the `DeviceBackedArray` that `re_ranking` returns (read
in place through the handle's compact form, never materialised in float64).  One GPU only: a row-sharded handle is refused.
"""
import numbers
import warnings

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream


def _real(x):
    return isinstance(x, numbers.Real) and not isinstance(x, (bool, np.bool_))


def _is_int(x):
    return isinstance(x, numbers.Integral) and not isinstance(x, (bool, np.bool_))


def _check_size_param(name, v, owner, allow_none=False, lo_open=False):
    """sklearn's constraint of min_samples / min_cluster_size: an int >= 2 or a float fraction"""
    if v is None and allow_none:
        return
    if _is_int(v) and v >= 2:
        return
    if _real(v) and not _is_int(v) and (0.0 < float(v) if lo_open else 0.0 <= float(v)) and float(v) <= 1.0:
        return
    raise ValueError("The %r parameter of %s must be an int in the range [2, inf) or a float in the range %s0.0, 1.0]%s. Got %r instead."
                     % (name, owner, "(" if lo_open else "[", " or None" if allow_none else "", v))


def _validate_size(size, n_samples, param_name):
    if size > n_samples:
        raise ValueError("%s must be no greater than the number of samples (%d). Got %d" % (param_name, n_samples, size))


def _resolve_size(size, n_samples, param_name):
    """an int as it is, a fraction -> max(2, int(f * n_samples)); larger than n_samples is an error (sklearn's order: check, then scale)"""
    _validate_size(size, n_samples, param_name)
    if size <= 1:
        size = max(2, int(size * n_samples))
    return int(size)


def _check_max_eps(max_eps, owner):
    if not _real(max_eps) or not float(max_eps) >= 0.0:
        raise ValueError("The 'max_eps' parameter of %s must be a float in the range [0.0, inf]. Got %r instead." % (owner, max_eps))


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


def compute_optics_graph(X, *, min_samples, max_eps, state=0):
    """sklearn.cluster.compute_optics_graph for a precomputed matrix, on the device -> (ordering_, core_distances_, reachability_,
    predecessor_) as numpy arrays (int64, float64, float64, int64).  `state`: where the loop keeps its state -- 0 auto (LDS while
    8 N bytes fit a workgroup's 160 KB, else global memory), 1 LDS, 2 global memory; every placement gives the same bits."""
    from . import cluster
    _check_size_param("min_samples", min_samples, "compute_optics_graph")
    _check_max_eps(max_eps, "compute_optics_graph")
    if state not in (0, 1, 2):
        raise ValueError("compute_optics_graph: state must be 0 (auto), 1 (LDS) or 2 (global memory), got %r" % (state,))
    shape = getattr(X, "shape", None)
    n = X.N if isinstance(X, cluster.DistHandle) else (int(shape[0]) if shape is not None and len(shape) >= 1 else None)
    if n is not None:
        _validate_size(min_samples, n, "min_samples")          # (before anything is uploaded)
    h = cluster.as_handle(X)
    if hasattr(h, "validate"):
        h.validate()
    if h.group is not None or h.row0 != 0 or h.nrows != h.N:
        raise ValueError("OPTICS runs on a single GPU: a row-sharded DistHandle is not supported")
    if h.N < 2:
        raise ValueError("OPTICS needs at least 2 samples, got a %d x %d matrix" % (h.N, h.N))
    k = _resolve_size(min_samples, h.N, "min_samples")
    ordering, core_h, reach_h, predecessor = _device_graph(h, k, float(max_eps), int(state))
    if np.all(np.isinf(reach_h)):
        warnings.warn("All reachability values are inf. Set a larger max_eps or all data will be considered outliers.", UserWarning)
    return ordering, core_h, reach_h, predecessor


def _device_graph(h, k, max_eps, state):
    """core distances and the ordering loop of handle `h` on its device, one blocking read -> (ordering, core, reachability, predecessor)"""
    N = h.N
    L = _lib.lib()
    dev = h.device
    with torch.cuda.device(dev):
        st = stream()
        f = torch.empty(3 * N, dtype=torch.float64, device=dev)          # core | reachability | the loop's state when it lives in global memory
        i = torch.empty(2 * N, dtype=torch.int64, device=dev)            # ordering | predecessor
        core, reach, ws = f[:N], f[N:2 * N], f[2 * N:]
        check(L.ssg_optics_core_dist(ptr(h.M), ptr(h.v), N, h.mode, h.lambda_value, k, max_eps, ptr(core), st), "ssg_optics_core_dist")
        check(L.ssg_optics_order(ptr(h.M), ptr(h.v), N, h.mode, h.lambda_value, ptr(core), max_eps, state, ptr(ws), N * 8,
                                 ptr(i[:N]), ptr(reach), ptr(i[N:]), st), "ssg_optics_order")
        fh, ih = _read_back(f[:2 * N], i)                                # one blocking read for all four arrays
    return ih[:N].copy(), fh[:N].copy(), fh[N:].copy(), ih[N:].copy()


def cluster_optics_dbscan(*, reachability, core_distances, ordering, eps):
    """sklearn.cluster.cluster_optics_dbscan: DBSCAN-like labels at `eps` from one ordering, O(N).  A point that is not reachable at eps
    but is core at eps opens a cluster; a point that is neither is noise."""
    if not _real(eps) or not float(eps) >= 0.0:
        raise ValueError("The 'eps' parameter of cluster_optics_dbscan must be a float in the range [0.0, inf]. Got %r instead." % (eps,))
    reachability, core_distances, ordering = np.asarray(reachability), np.asarray(core_distances), np.asarray(ordering)
    far = reachability > eps
    core = core_distances <= eps
    labels = np.zeros(len(core_distances), dtype=int)
    labels[ordering] = np.cumsum(far[ordering] & core[ordering]) - 1
    labels[far & ~core] = -1
    return labels


def _extend_region(steep, xward, start, min_samples):
    """last steep point of the maximal region that starts at `start`: it ends at a point that goes the other way, or after more than
    min_samples consecutive points that are not steep"""
    flat, end = 0, start
    for idx in range(start, len(steep)):
        if steep[idx]:
            flat, end = 0, idx
        elif not xward[idx]:
            flat += 1
            if flat > min_samples:
                break
        else:
            break
    return end


def _filter_sdas(sdas, mib, xi_c, plot):
    """keep the steep-down areas that the maximum in between has not outgrown, and raise their own maximum to it"""
    if np.isinf(mib):
        return []
    kept = [d for d in sdas if mib <= plot[d[0]] * xi_c]
    for d in kept:
        d[2] = max(d[2], mib)
    return kept


def _correct_predecessor(plot, pred_plot, ordering, s, e):
    """Schubert & Gertz 2018, algorithm 2: drop end points whose predecessor lies outside the cluster"""
    while s < e:
        if plot[s] > plot[e]:
            return s, e
        if np.any(ordering[s:e] == pred_plot[e]):
            return s, e
        e -= 1
    return None, None


def _xi_cluster(plot, pred_plot, ordering, xi, min_samples, min_cluster_size, predecessor_correction):
    """the xi-steep extraction of the OPTICS paper (figure 19) as sklearn 1.7.2 runs it -> [n_clusters, 2] (start, end), ends inclusive"""
    plot = np.hstack((plot, np.inf))            # lets a cluster end at the end of the plot
    xi_c = 1 - xi
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = plot[:-1] / plot[1:]
        steep_up, steep_down = ratio <= xi_c, ratio >= 1 / xi_c
        down, up = ratio > 1, ratio < 1
    sdas, clusters, index, mib = [], [], 0, 0.0        # an area is [start, end, mib]
    for si in np.flatnonzero(steep_up | steep_down):
        if si < index:
            continue
        mib = max(mib, np.max(plot[index:si + 1]))
        sdas = _filter_sdas(sdas, mib, xi_c, plot)
        if steep_down[si]:
            d_end = _extend_region(steep_down, up, si, min_samples)
            sdas.append([int(si), d_end, 0.0])
            index = d_end + 1
            mib = plot[index]
            continue
        u_start = int(si)
        u_end = _extend_region(steep_up, down, u_start, min_samples)
        index = u_end + 1
        mib = plot[index]
        found = []
        for d_start, d_end, d_mib in sdas:
            c_start, c_end = d_start, u_end
            if plot[c_end + 1] * xi_c < d_mib:
                continue
            d_max = plot[d_start]
            if d_max * xi_c >= plot[c_end + 1]:
                while plot[c_start + 1] > plot[c_end + 1] and c_start < d_end:        # the start climbs down to the level of the end
                    c_start += 1
            elif plot[c_end + 1] * xi_c >= d_max:
                while plot[c_end - 1] > d_max and c_end > u_start:                    # the end climbs down to the level of the start
                    c_end -= 1
            if predecessor_correction:
                c_start, c_end = _correct_predecessor(plot, pred_plot, ordering, c_start, c_end)
            if c_start is None:
                continue
            if c_end - c_start + 1 < min_cluster_size or c_start > d_end or c_end < u_start:
                continue
            found.append((c_start, c_end))
        clusters.extend(reversed(found))               # the smaller clusters first
    return np.array(clusters)


def _xi_labels(ordering, clusters):
    """leaves of the hierarchy: a cluster gets a label when none of its points has one yet (the smaller clusters come first)"""
    labels = np.full(len(ordering), -1, dtype=int)
    label = 0
    for c in clusters:
        if not np.any(labels[c[0]:c[1] + 1] != -1):
            labels[c[0]:c[1] + 1] = label
            label += 1
    labels[ordering] = labels.copy()
    return labels


def cluster_optics_xi(*, reachability, predecessor, ordering, min_samples, min_cluster_size=None, xi=0.05, predecessor_correction=True):
    """sklearn.cluster.cluster_optics_xi -> (labels, clusters): the xi-steep clusters of the reachability plot, no eps needed.
    clusters [n_clusters, 2] holds (start, end) positions in the ordering, ends inclusive, nested smaller clusters first."""
    _check_size_param("min_samples", min_samples, "cluster_optics_xi")
    _check_size_param("min_cluster_size", min_cluster_size, "cluster_optics_xi", allow_none=True)
    if not _real(xi) or not 0.0 <= float(xi) <= 1.0:
        raise ValueError("The 'xi' parameter of cluster_optics_xi must be a float in the range [0.0, 1.0]. Got %r instead." % (xi,))
    if not isinstance(predecessor_correction, (bool, np.bool_)):
        raise ValueError("The 'predecessor_correction' parameter of cluster_optics_xi must be an instance of 'bool' or an instance of "
                         "'numpy.bool_'. Got %r instead." % (predecessor_correction,))
    reachability, predecessor, ordering = np.asarray(reachability), np.asarray(predecessor), np.asarray(ordering)
    n = len(reachability)
    min_samples = _resolve_size(min_samples, n, "min_samples")
    min_cluster_size = min_samples if min_cluster_size is None else _resolve_size(min_cluster_size, n, "min_cluster_size")
    clusters = _xi_cluster(reachability[ordering], predecessor[ordering], ordering, xi, min_samples, min_cluster_size, predecessor_correction)
    return _xi_labels(ordering, clusters), clusters


class OPTICS:
    """sklearn.cluster.OPTICS (1.7.2) look-alike for metric='precomputed' running on the GPU: the same constructor, `fit`, `fit_predict`,
    `ordering_`, `core_distances_`, `reachability_`, `predecessor_`, `labels_`, `cluster_hierarchy_` (cluster_method='xi' only) and
    `n_features_in_`, the same errors and the same warning -- and the same bits.  `p`, `metric_params`, `algorithm`, `leaf_size`, `memory`
    and `n_jobs` are accepted and ignored.  One GPU only.  The class attribute `state` (0 auto, 1 LDS, 2 global memory) places the
    loop's state, see `compute_optics_graph`; every placement gives the same result."""

    state = 0

    def __init__(self, *, min_samples=5, max_eps=np.inf, metric="minkowski", p=2, metric_params=None, cluster_method="xi", eps=None, xi=0.05,
                 predecessor_correction=True, min_cluster_size=None, algorithm="auto", leaf_size=30, memory=None, n_jobs=None):
        self.min_samples, self.max_eps, self.metric, self.p, self.metric_params = min_samples, max_eps, metric, p, metric_params
        self.cluster_method, self.eps, self.xi, self.predecessor_correction = cluster_method, eps, xi, predecessor_correction
        self.min_cluster_size, self.algorithm, self.leaf_size, self.memory, self.n_jobs = min_cluster_size, algorithm, leaf_size, memory, n_jobs

    def _validate(self):
        # sklearn raises InvalidParameterError (a ValueError) for these
        _check_size_param("min_samples", self.min_samples, "OPTICS")
        _check_max_eps(self.max_eps, "OPTICS")
        if self.metric != "precomputed":
            raise ValueError("ssg_amd.optics.OPTICS implements metric='precomputed' only (the SSG grouping path clusters a precomputed "
                             "re-rank distance); got metric=%r" % (self.metric,))
        if self.cluster_method not in ("xi", "dbscan"):
            raise ValueError("The 'cluster_method' parameter of OPTICS must be a str among {'dbscan', 'xi'}. Got %r instead." % (self.cluster_method,))
        if self.eps is not None and (not _real(self.eps) or not float(self.eps) >= 0.0):
            raise ValueError("The 'eps' parameter of OPTICS must be a float in the range [0.0, inf] or None. Got %r instead." % (self.eps,))
        if not _real(self.xi) or not 0.0 <= float(self.xi) <= 1.0:
            raise ValueError("The 'xi' parameter of OPTICS must be a float in the range [0.0, 1.0]. Got %r instead." % (self.xi,))
        if not isinstance(self.predecessor_correction, (bool, np.bool_)):
            raise ValueError("The 'predecessor_correction' parameter of OPTICS must be an instance of 'bool' or an instance of 'numpy.bool_'. "
                             "Got %r instead." % (self.predecessor_correction,))
        _check_size_param("min_cluster_size", self.min_cluster_size, "OPTICS", allow_none=True, lo_open=True)

    def fit(self, X, y=None):
        self._validate()
        eps = self.max_eps if self.eps is None else self.eps
        if self.cluster_method == "dbscan" and eps > self.max_eps:     # (sklearn raises this after the ordering; nothing is lost by raising it before)
            raise ValueError("Specify an epsilon smaller than %s. Got %s." % (self.max_eps, eps))
        self.ordering_,self.core_distances_, self.reachability_, self.predecessor_ = compute_optics_graph(
            X, min_samples=self.min_samples, max_eps=self.max_eps, state=self.state)
        self.n_features_in_ = len(self.ordering_)
        if self.cluster_method == "xi":
            labels, clusters = cluster_optics_xi(reachability=self.reachability_, predecessor=self.predecessor_, ordering=self.ordering_,
                                                 min_samples=self.min_samples, min_cluster_size=self.min_cluster_size, xi=self.xi,
                                                 predecessor_correction=self.predecessor_correction)
            self.cluster_hierarchy_ = clusters
        else:
            labels = cluster_optics_dbscan(reachability=self.reachability_, core_distances=self.core_distances_, ordering=self.ordering_, eps=eps)
        self.labels_ = labels
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_
