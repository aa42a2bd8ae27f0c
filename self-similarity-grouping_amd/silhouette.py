"""The silhouette coefficient on MI355X for a precomputed distance matrix -- look-alikes of sklearn 1.7.2 `silhouette_samples` and
`silhouette_score` for `metric='precomputed'`, and `silhouette_many`, which scores K labelings of the same matrix in ONE pass over it.

The part that touches the N x N matrix runs on the device (csrc/silhouette.hip): for every row the float64 sum of its entries per cluster,
added in ascending column order exactly as `np.bincount(labels, weights=row)` adds them, the own cluster's sum and the smallest mean of
another cluster.  They equal sklearn's `_silhouette_reduce` bit for bit: like the other estimators here the matrix is widened to float64
first, so a float32 or float16 matrix gives the result of its float64 copy, as float64 (sklearn itself returns float32 for a float32
matrix, computed in float32).  The matrix is read in place through its handle and never modified; sklearn needs the dense float64
matrix on the host (8 N^2 bytes) and refuses the re-rank matrix outright, whose diagonal is lambda * half(2 v_i), not 0.

Everything else works on N-long arrays and stays on the host: the label encoding (`np.unique`, what LabelEncoder does), the member lists
(a stable counting sort), sklearn's own four numpy lines after the reduction, the mean.  sklearn is not imported.

Input: whatever `hdbscan._as_handle` takes -- numpy, torch, a `DistHandle` or the `DeviceBackedArray` that `re_ranking` returns.  One GPU
only: a row-sharded handle is refused.  Sparse input is refused.

Beyond sklearn: `diagonal='zero'` treats the diagonal as 0 without writing it (sklearn on a copy after `np.fill_diagonal(X, 0)`);
`ignore_noise=True` drops the samples labelled -1 (sklearn on `X[keep][:, keep]`, `labels[keep]`; NaN at the dropped positions).  With
`ignore_noise` the NaN / infinity check, the diagonal check and the refusal of negative entries still cover the whole matrix, which
is stricter than sklearn on the sub-matrix.  Like sklearn (its `pairwise_distances`) a matrix with a negative entry is refused; the
kernel itself sums negative entries like any others and only counts them.
"""
import numbers

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from .hdbscan import _as_handle, _read_back

_NAN = "Input X contains NaN."
_INF = "Input X contains infinity or a value too large for dtype('%s')."
_DIAG = "The precomputed distance matrix contains non-zero elements on the diagonal. Use np.fill_diagonal(X, 0)."
_NLABELS = "Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)"
_NEGATIVE = "Negative values in data passed to `pairwise_distances`. Precomputed distance  need to have non-negative values.."
_LENGTH = "Found input variables with inconsistent numbers of samples: %r"


# ------------------------------------------------------------------------------------------------------------ the host stages
def _encode(labels, ignore_noise):
    """one labeling of the selected samples -> (enc int32 [m]: 0 .. C - 1 in sorted label order, -1 = takes no part; C)"""
    labels = np.asarray(labels)
    keep = labels != -1 if ignore_noise else np.ones(len(labels), dtype=bool)
    enc = np.full(len(labels), -1, dtype=np.int32)
    classes, inv = np.unique(labels[keep], return_inverse=True)
    enc[keep] = inv
    return enc, len(classes)


def _member_list(enc, C):
    """the positions grouped by cluster, ascending inside each cluster (a stable counting sort) -> (members int32 [m], the tail past the
    last member zero; start int32 [C + 1])"""
    pos = np.nonzero(enc >= 0)[0]
    members = np.zeros(len(enc), dtype=np.int32)
    members[:len(pos)] = pos[np.argsort(enc[pos], kind="stable")]
    start = np.zeros(C + 1, dtype=np.int32)
    start[1:] = np.cumsum(np.bincount(enc[pos], minlength=C))
    return members, start


def _finish(intra, inter, enc):
    """sklearn's lines after `_silhouette_reduce`, on the samples that take part -> float64 [m], NaN where enc < 0"""
    keep = enc >= 0
    labels = enc[keep].astype(np.intp)
    label_freqs = np.bincount(labels)
    intra_clust_dists, inter_clust_dists = intra[keep].copy(), inter[keep].copy()
    denom = (label_freqs - 1).take(labels, mode="clip")
    with np.errstate(divide="ignore", invalid="ignore"):
        intra_clust_dists /= denom
    sil_samples = inter_clust_dists - intra_clust_dists
    with np.errstate(divide="ignore", invalid="ignore"):
        sil_samples /= np.maximum(intra_clust_dists, inter_clust_dists)
    out = np.full(len(enc), np.nan, dtype=np.float64)
    out[keep] = np.nan_to_num(sil_samples)                               # (NaN: a cluster of one sample, whose silhouette is 0)
    return out


def _labels_valid(enc, C):
    """sklearn's check_number_of_labels on the samples that take part"""
    return 1 < C < int(np.count_nonzero(enc >= 0))


# ------------------------------------------------------------------------------------------------------------ the device stage
def _device(h, sel, encs, Cs, diag_zero, atol, state):
    """the NaN / infinity counts, the diagonal count (atol is not None) and, when `encs` is not empty, the sums of every labeling, queued
    behind each other, one blocking read -> (nan, inf, ndiag, negatives, intra [K, m], inter [K, m])"""
    L = _lib.lib()
    dev = h.device
    N = h.N
    m = N if sel is None else len(sel)
    K = len(encs)
    with torch.cuda.device(dev):
        st = stream()
        counts = torch.zeros(4, dtype=torch.int64, device=dev)           # nan | inf | diagonal | negative entries
        view = (ptr(h.M), ptr(h.v), N, h.mode, h.lambda_value)
        sel_h = None if sel is None else np.ascontiguousarray(sel, dtype=np.int32)
        Cmax = max(Cs) if K else 1
        parts = [sel_h if sel_h is not None else np.zeros(0, np.int32)]
        for enc, C in zip(encs, Cs):
            members, start = _member_list(enc, C)
            parts += [enc, members, np.concatenate([start, np.full(Cmax - C, start[-1], np.int32)])]
        parts.append(np.asarray(Cs, dtype=np.int32))
        ints = torch.from_numpy(np.concatenate(parts)).to(dev)           # sel | K x (labels, members, start) | ncl
        n_sel = 0 if sel is None else m
        sel_d = ints[:n_sel] if n_sel else None
        sel_p = None if sel_h is None else sel_h.ctypes.data
        check(L.ssg_agglo_check(*view, ptr(counts[:2]), st), "ssg_agglo_check")
        if atol is not None:
            check(L.ssg_silhouette_diag(*view, ptr(sel_d), sel_p, m, float(atol), ptr(counts[2:3]), st), "ssg_silhouette_diag")
        if not K:
            (c,) = _read_back(counts)
            return int(c[0]), int(c[1]), int(c[2]), 0, None, None
        # the per-labeling arrays are interleaved above for one upload; the entry point takes [K, m] / [K, Cmax + 1] blocks
        per = 2 * m + Cmax + 1
        body = ints[n_sel:n_sel + K * per].view(K, per)
        lab_d, mem_d, start_d = body[:, :m].contiguous(), body[:, m:2 * m].contiguous(), body[:, 2 * m:].contiguous()
        ncl_d = ints[n_sel + K * per:]
        f = torch.full((2, K, m), float("nan"), dtype=torch.float64, device=dev)
        lds = state == 1 or (state == 0 and m <= L.ssg_silhouette_lds_max_m())
        ws, ws_bytes = None, 0
        if not lds:
            slice_ = (m + 1) & ~1
            ws = torch.empty(min(m, 1024) * slice_, dtype=torch.float64, device=dev)
            ws_bytes = ws.numel() * 8
        check(L.ssg_silhouette_sums(*view, ptr(sel_d), sel_p, m, K, Cmax, ptr(lab_d), ptr(mem_d), ptr(start_d), ptr(ncl_d), 1 if diag_zero else 0,
                                    state, ptr(ws), ws_bytes, ptr(f[0]), ptr(f[1]), ptr(counts[3:]), st), "ssg_silhouette_sums")
        c, fh = _read_back(counts, f)                                    # one blocking read: the four counts and the two arrays of every labeling
    return int(c[0]), int(c[1]), int(c[2]), int(c[3]), fh[0], fh[1]


# ------------------------------------------------------------------------------------------------------------ the input checks
def _handle(X):
    """-> (handle, the dtype name sklearn's messages would print, the diagonal atol of sklearn's check)"""
    from .rerank import DistHandle
    if hasattr(X, "tocsr") or hasattr(X, "todense"):
        raise TypeError("ssg_amd.silhouette takes a dense precomputed distance matrix; sparse input is not supported")
    valid = getattr(X, "valid_handle", None)
    dtype = "float64"
    if not (isinstance(X, DistHandle) or (callable(valid) and isinstance(valid(), DistHandle))):
        if not isinstance(X, np.ndarray) and not torch.is_tensor(X):
            raise TypeError("unsupported distance matrix type %r" % type(X))
        shape = tuple(int(s) for s in X.shape)
        if len(shape) != 2:
            raise ValueError("Expected 2D array, got %dD array instead" % len(shape))
        if shape[0] != shape[1]:
            raise ValueError("Precomputed metric requires shape (n_queries, n_indexed). Got %s for %d indexed." % (shape, shape[0]))
        if str(X.dtype).replace("torch.", "") in ("float16", "float32"):
            dtype = str(X.dtype).replace("torch.", "")
    h = _as_handle(X)
    if hasattr(h, "validate"):
        h.validate()
    if h.group is not None or h.row0 != 0 or h.nrows != h.N:
        raise ValueError("the silhouette runs on a single GPU: a row-sharded DistHandle is not supported")
    atol = 100.0 * float(np.finfo(np.float32 if dtype == "float32" else np.float64).eps)
    return h, dtype, atol


def _check_options(metric, diagonal, state):
    if metric != "precomputed":
        raise ValueError("ssg_amd.silhouette implements metric='precomputed' only (the SSG grouping path scores a precomputed re-rank "
                         "distance); got metric=%r" % (metric,))
    if diagonal not in ("check", "zero"):
        raise ValueError("diagonal must be 'check' (sklearn's refusal of a non-zero diagonal) or 'zero' (the diagonal counts as 0), got %r" % (diagonal,))
    if state not in (0, 1, 2):
        raise ValueError("state must be 0 (auto), 1 (LDS) or 2 (global memory), got %r" % (state,))


def _as_labels(labels):
    labels = np.asarray(labels)
    if labels.ndim == 2 and labels.shape[1] == 1:
        labels = labels.ravel()
    if labels.ndim != 1:
        raise ValueError("y should be a 1d array, got an array of shape %s instead." % (labels.shape,))
    return labels


def _many(X, labelings, sel, diagonal, ignore_noise, state, single):
    """the body of every entry point.  sel: None, or the selected samples in column order (`silhouette_score(sample_size=...)`); the
    labelings are N-long and are cut down to `sel` here.  Errors in sklearn's order: NaN, infinity, the length of the labels, the
    diagonal, the number of labels, a negative entry."""
    h, dtype, atol = _handle(X)
    labelings = [_as_labels(l) for l in labelings]
    short = [k for k, l in enumerate(labelings) if len(l) != h.N]
    m = h.N if sel is None else len(sel)
    encs, Cs = [], []
    if not short:
        for l in labelings:
            enc, C = _encode(l if sel is None else l[sel], ignore_noise)
            encs.append(enc)
            Cs.append(C)
    bad = [k for k in range(len(encs)) if not _labels_valid(encs[k], Cs[k])]
    run = not short and not bad and m >= 3
    if h.N < 2:
        raise ValueError(_NLABELS % (Cs[0] if Cs else 0))
    nan, inf, ndiag, negative, intra, inter = _device(h, sel, encs if run else [], Cs if run else [], diagonal == "zero", atol if diagonal == "check" else None, state)
    if nan:
        raise ValueError(_NAN)
    if inf:
        raise ValueError(_INF % dtype)
    if short:
        raise ValueError(_LENGTH % ([h.N, len(labelings[short[0]])],))
    if ndiag:
        raise ValueError(_DIAG)
    if bad:
        raise ValueError((_NLABELS % Cs[bad[0]]) if single else ("labeling %d: " % bad[0] + _NLABELS % Cs[bad[0]]))
    if negative:
        raise ValueError(_NEGATIVE)
    return [_finish(intra[k], inter[k], encs[k]) for k in range(len(encs))]


# ------------------------------------------------------------------------------------------------------------ the public surface
def silhouette_samples(X, labels, *, metric="precomputed", diagonal="check", ignore_noise=False, state=0):
    """sklearn.metrics.silhouette_samples(X, labels, metric='precomputed') on the device -> float64 [n], sklearn's bits for a float64
    matrix.  diagonal='check': sklearn's refusal of a diagonal entry beyond 100 eps (float32's eps for a float32 matrix, else
    float64's); 'zero': no check, the diagonal counts as 0.  ignore_noise: the samples labelled -1 are dropped (NaN in the result).
    state: where the kernel stages a row -- 0 auto, 1 LDS, 2 global memory; every placement gives the same bits."""
    _check_options(metric, diagonal, state)
    return _many(X, [labels], None, diagonal, bool(ignore_noise), int(state), True)[0]


def silhouette_many(X, labelings, *, diagonal="check", ignore_noise=False, state=0):
    """`silhouette_samples` of every labeling in `labelings` -> a list of float64 [n] arrays, from ONE pass over the matrix and one
    blocking read.  With ignore_noise every labeling drops its own -1 samples.  A labeling whose number of labels is invalid raises
    with its index in the message."""
    _check_options("precomputed", diagonal, state)
    labelings = list(labelings)
    if not labelings:
        raise ValueError("silhouette_many needs at least one labeling")
    return _many(X, labelings, None, diagonal, bool(ignore_noise), int(state), False)


def _random_state(seed):
    """sklearn.utils.check_random_state"""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, numbers.Integral):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError("%r cannot be used to seed a numpy.random.RandomState instance" % seed)


def silhouette_score(X, labels, *, metric="precomputed", sample_size=None, random_state=None, diagonal="check", ignore_noise=False, state=0):
    """sklearn.metrics.silhouette_score(X, labels, metric='precomputed', sample_size, random_state): the mean of `silhouette_samples`
    (over the samples that take part, with ignore_noise) as a Python float.  With sample_size the score is that of
    `X[indices][:, indices]`, `labels[indices]` for `indices = check_random_state(random_state).permutation(n)[:sample_size]`, read in
    place; the random stream advances exactly as sklearn's does (not at all when X is refused for NaN, infinity or the labels' length)."""
    _check_options(metric, diagonal, state)
    if sample_size is None:
        sil = _many(X, [labels], None, diagonal, bool(ignore_noise), int(state), True)[0]
    else:
        if not isinstance(sample_size, numbers.Integral) or sample_size < 1:
            raise ValueError("The 'sample_size' parameter of silhouette_score must be an int in the range [1, inf) or None. Got %r instead." % (sample_size,))
        rs = _random_state(random_state)
        n = X.N if hasattr(X, "N") else int(X.shape[0])
        before = rs.get_state()
        indices = rs.permutation(n)[:sample_size]
        try:
            sil = _many(X, [labels], indices, diagonal, bool(ignore_noise), int(state), True)[0]
        except ValueError as e:
            if str(e).startswith(("Input X contains", "Found input variables")):     # sklearn refuses these before it draws
                rs.set_state(before)
            raise
    return float(np.mean(sil[~np.isnan(sil)] if ignore_noise else sil))


# ------------------------------------------------------------------------------------------------------------ the sweep's selection
def cut_is_valid(labels):
    """can the clustered samples of this cut (label != -1) be scored: between 2 and m - 1 labels among m samples"""
    labels = np.asarray(labels)
    kept = labels[labels != -1]
    return 1 < len(np.unique(kept)) < len(kept)


def select_cut(factors, cuts, scorer):
    """the choice of `generate_selflabel_sweep`, free of any device call.  cuts: one label array per factor (-1 = noise); scorer: a
    function from a list of label arrays to their per-sample silhouettes with NaN at the noise (`silhouette_many(dist, cuts,
    diagonal='zero', ignore_noise=True)`), called once with the valid cuts.  The score of a cut = the sum of the silhouettes of its
    clustered samples / N: noise counts as 0, so a cut cannot win by declaring everything noise.  A cut that cannot be scored is
    skipped (score None).  The first maximum in list order wins; with no valid cut the factor 1.0 (else the factor nearest to it) wins.
    -> (index of the chosen cut, [score or None per cut])"""
    factors = [float(f) for f in factors]
    if len(factors) != len(cuts) or not factors:
        raise ValueError("select_cut: %d factors for %d cuts" % (len(factors), len(cuts)))
    valid = [k for k, lab in enumerate(cuts) if cut_is_valid(lab)]
    scores = [None] * len(cuts)
    if valid:
        for k, sil in zip(valid, scorer([cuts[k] for k in valid])):
            sil = np.asarray(sil, dtype=np.float64)
            scores[k] = float(np.sum(np.where(np.isnan(sil), 0.0, sil))) / len(sil)
    best = None
    for k in valid:
        if best is None or scores[k] > scores[best]:
            best = k
    if best is None:
        best = min(range(len(factors)), key=lambda k: (abs(factors[k] - 1.0), k))
    return best, scores
