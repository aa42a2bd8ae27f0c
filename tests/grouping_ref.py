"""Independent reference for the grouping step -- the eps rule and DBSCAN of selftraining.py:289-306 -- at sizes the oracle cannot
hold (N = 30 000 and 128 000: 7.2 GB and 131 GB of float64).

It shares no code with csrc/eps_rule.hip and csrc/dbscan.hip.  final_dist is rebuilt row block by row block from the handle's J' and v with plain torch
element-wise ops (on the device, so that N = 128 000 needs no 32 GB host copy).  The eps rule takes numpy's mean of the sorted exact
candidate set.  The labels come from sklearn's own DBSCAN on the sparse neighbour graph.  Everything here is exact: a consumer
compares with `==`, never within a tolerance.

    mat = FinalDist(h.M, h.v, lam)           # or Dense(matrix) for an explicit float64 matrix
    e = eps_rule(mat, rho, hint=eps_dev)     # -> EpsRule(eps, count, top, ncand, cap)
    g = region_graph(mat, e.eps)             # -> Graph(counts, csr): per-row neighbour counts (self included), stored pairs
    lab, core = dbscan(g, e.eps, 4)          # sklearn 1.7.2 on the sparse graph
"""
from collections import namedtuple

import numpy as np
import torch

EpsRule = namedtuple("EpsRule", "eps count top ncand cap")
Graph = namedtuple("Graph", "counts csr nhits")


def final_rows(Jp, v, lam, lo, hi):
    """final_dist[lo:hi, :] = f64(J'[i, j]) + f64(half(v_i + v_j)) * lambda (reid/rerank.py:122), float64 [hi - lo, N].

    half(v_i + v_j) as numpy takes it: a float32 add, then one rounding to half (float32 holds the sum of two halves closely enough that
    the two roundings never differ from one).  The product and the sum are two separate torch ops, so no FMA can form."""
    s = (v[lo:hi].float()[:, None] + v.float()[None, :]).half()
    prod = torch.mul(s.double(), float(lam))
    return torch.add(Jp[lo:hi].double(), prod)


class FinalDist:
    """final_dist of a re-rank handle (J' half [N, N], v half [N], lambda) as float64 row blocks, rebuilt on every pass"""

    def __init__(self, Jp, v, lam, block_rows=2000):
        assert Jp.dim() == 2 and Jp.shape[0] == Jp.shape[1] == v.shape[0] and Jp.dtype == torch.float16 and v.dtype == torch.float16
        self.Jp, self.v, self.lam, self.N, self.block_rows = Jp, v, float(lam), int(Jp.shape[0]), int(block_rows)

    def blocks(self):
        for lo in range(0, self.N, self.block_rows):
            hi = min(self.N, lo + self.block_rows)
            yield lo, final_rows(self.Jp, self.v, self.lam, lo, hi)


class Dense:
    """an explicit square matrix (numpy or torch) as float64 row blocks"""

    def __init__(self, D, block_rows=2000):
        D = torch.as_tensor(np.asarray(D)) if not torch.is_tensor(D) else D
        assert D.dim() == 2 and D.shape[0] == D.shape[1]
        self.D, self.N, self.block_rows = D, int(D.shape[0]), int(block_rows)

    def blocks(self):
        for lo in range(0, self.N, self.block_rows):
            yield lo, self.D[lo:lo + self.block_rows].double()


def _upper(lo, F):
    """mask of the strict upper triangle in the row block F = rows [lo, lo + len(F))"""
    rows = torch.arange(lo, lo + F.shape[0], device=F.device)[:, None]
    cols = torch.arange(F.shape[1], device=F.device)[None, :]
    return cols > rows


def eps_rule(mat, rho, hint=None):
    """selftraining.py:289-293: eps = mean of the round(rho * count) smallest non-zero entries of the strict upper triangle.

    Pass 1 counts the non-zero strict-upper entries (count) and, for a ladder of caps, the entries at or below each cap.  The ladder
    starts at twice `hint` (the device's eps: only a hint) and doubles up to +inf; a few finer rungs below 2 * hint keep the collected
    set small.  Pass 2 collects every entry at or below the smallest cap that holds at least `top` of them, so the `top` smallest
    entries are all among them -- as (value, multiplicity) pairs per row block, because final_dist takes few distinct values and the
    smallest sufficient cap can still hold most of the matrix.  On the host the pairs are merged, the first `top` entries of the sorted
    array are expanded, and numpy takes their `.mean()`: the reference's own call on an array equal to the reference's first `top`
    sorted entries, hence the same mean bit for bit."""
    caps = []
    if hint is not None and np.isfinite(hint) and hint > 0:
        caps = [hint * f for f in (1.0, 1.05, 1.1, 1.25, 1.5)] + [hint * 2.0 ** k for k in range(1, 13)]
    count, le = 0, np.zeros(len(caps) + 1, np.int64)
    caps_t = None
    for lo, F in mat.blocks():
        assert not bool(torch.isnan(F).any()), "NaN in final_dist rows %d.." % lo
        up = _upper(lo, F) & (F != 0)
        count += int(up.sum())
        if caps:
            if caps_t is None:
                caps_t = torch.tensor(caps, dtype=torch.float64, device=F.device)
            b = torch.bucketize(F[up], caps_t)             # b = first c with value <= caps[c] (len(caps): above every cap)
            le[:-1] += np.cumsum(torch.bincount(b, minlength=len(caps) + 1).cpu().numpy())[:-1]
            del b
        del up
    le[-1] = count
    caps = caps + [float("inf")]
    top = int(np.round(rho * count))          # np.round: half to even, like the reference's np.round(...).astype(int)
    if top <= 0:
        return EpsRule(float("nan"), count, top, 0, None)
    c = int(np.nonzero(le >= top)[0][0])
    cap = caps[c]
    vals, mult = [], []
    for lo, F in mat.blocks():
        up = _upper(lo, F) & (F != 0) & (F <= cap)
        u, n = torch.unique(F[up], return_counts=True)
        vals.append(u.cpu().numpy()); mult.append(n.cpu().numpy())
        del up, u, n
    vals, mult = np.concatenate(vals), np.concatenate(mult)
    u, inv = np.unique(vals, return_inverse=True)
    n = np.zeros(u.shape[0], np.int64)
    np.add.at(n, inv, mult)
    assert int(n.sum()) == le[c] and le[c] >= top
    j = int(np.searchsorted(np.cumsum(n), top, side="left"))       # the top-th entry has value u[j]
    cand = np.repeat(u[:j + 1], n[:j + 1])
    return EpsRule(float(cand[:top].mean()), count, top, int(le[c]), cap)


def numpy_eps_rule(dist, rho):
    """selftraining.py:289-293 verbatim on a materialised matrix (numpy, any float dtype) -> (eps, count, top_num)"""
    tri_mat = np.triu(dist, 1)
    tri_mat = tri_mat[np.nonzero(tri_mat)]
    tri_mat = np.sort(tri_mat, axis=None)
    top_num = np.round(rho * tri_mat.size).astype(int)
    return tri_mat[:top_num].mean(), int(tri_mat.size), int(top_num)


def region_graph(mat, eps):
    """DBSCAN's region query (radius neighbours with distance <= eps; a point is its own neighbour when its diagonal entry is <= eps):
    per-row neighbour counts and the neighbour pairs as a CSR graph for sklearn.

    sklearn only treats STORED entries as neighbours, and DBSCAN.fit on a sparse matrix first calls X.setdiag(X.diagonal()): a missing
    diagonal entry is inserted as an explicit 0, which would make every point its own neighbour.  So the diagonal is always stored
    with its true value (sklearn filters it out when it exceeds eps), and off-diagonal zeros stay stored (no eliminate_zeros).  Each
    row's entries are ordered by distance, as sklearn's _check_precomputed wants them, so it does not re-sort them row by row."""
    import scipy.sparse as sp
    N = mat.N
    counts = np.zeros(N, np.int64)
    rows_l, cols_l, vals_l = [], [], []
    nhits = 0
    for lo, F in mat.blocks():
        hit = F <= eps
        counts[lo:lo + F.shape[0]] = hit.sum(1).cpu().numpy()
        nhits += int(hit.sum())
        r = torch.arange(F.shape[0], device=F.device)
        hit[r, lo + r] = True                      # the diagonal is stored whatever its value
        ri, ci = torch.nonzero(hit, as_tuple=True)
        val = F[ri, ci]
        o = torch.argsort(val, stable=True)
        o = o[torch.argsort(ri[o], stable=True)]  # by row, and by distance inside a row
        rows_l.append((ri[o] + lo).cpu().numpy()); cols_l.append(ci[o].cpu().numpy()); vals_l.append(val[o].cpu().numpy())
        del hit, ri, ci, val, o
    rows = np.concatenate(rows_l); cols = np.concatenate(cols_l); vals = np.concatenate(vals_l)
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=N), out=indptr[1:])
    csr = sp.csr_matrix((vals, cols, indptr), shape=(N, N))
    assert csr.nnz == vals.shape[0], "explicit entries must stay stored"
    return Graph(counts, csr, nhits)


def hit_keys(g, eps):
    """the neighbour pairs (i, k) with distance <= eps, self pairs included, as sorted int64 keys i * N + k"""
    csr = g.csr
    N = csr.shape[0]
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(csr.indptr))
    keep = csr.data <= eps
    keys = np.sort(rows[keep] * N + csr.indices[keep].astype(np.int64))
    assert keys.shape[0] == g.nhits
    return keys


def dbscan(g, eps, min_samples=4):
    """sklearn.cluster.DBSCAN(eps, min_samples, metric='precomputed').fit on the sparse graph -> (labels, core_sample_indices)"""
    from sklearn.cluster import DBSCAN
    est = DBSCAN(eps=float(eps), min_samples=int(min_samples), metric="precomputed").fit(g.csr)
    return est.labels_.astype(np.int64), est.core_sample_indices_
