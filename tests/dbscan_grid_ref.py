"""Case table of the DBSCAN grid and a plain restatement of sklearn's DBSCAN(metric='precomputed'): tools/make_golden.py
(dbscan_grid_fixture -> tests/golden/dbscan_grid.npz), tests/test_dbscan_grid_host.py and tests/test_gpu_dbscan_grid.py all import it.

`ssg_amd.cluster.DBSCAN` accepts any min_samples >= 1, any eps > 0, float64 / float32 / float16 matrices as numpy arrays or torch
tensors, and re-rank handles.  Inside that range the kernels (csrc/dbscan.hip, csrc/matview.h) change their control flow with N (rows on /
off the 8-element boundary, one chunk of 512, a partial last chunk, the last row's tail guard), with the dtype (three matrix modes) and
with the structure of the neighbour graph (hook, union, flatten and border passes).  Every case names what it is there to reach (`why`) and
the properties it must have (`claims`, recomputed by the generator and by the host test from the restatement).

`dbscan_ref` is the VISITING-ORDER definition (sklearn's dbscan_inner), not the components formulation the kernels use.  The fixture holds
what sklearn 1.7.2 gave on the arrays exactly as the cases pass them (same dtype, the same Python-float eps); the matrices themselves are
regenerated from their seeds (their sha256 is stored).

What sklearn compares, found on sklearn 1.7.2 and pinned by the fixture: a float32 matrix stays float32 (check_pairwise_arrays) and
`dist <= radius` then runs in float32 -- numpy casts the Python scalar to the array's dtype; every other dtype, float16 included, is
widened to float64 first.  `neighbourhood_dtype` restates that rule."""
import hashlib
from collections import namedtuple

import numpy as np

FIXTURE = "dbscan_grid.npz"
CHAIN_MS = (1, 3, 10)                        # min_samples of the eps_rule_dbscan tests
EDGES_PER_ROW = 64                           # cluster.py: the first edge list holds max(64 * rows, 65536) hits
MIN_EDGE_CAP = 1 << 16
FAR = 100.0                                  # "not a neighbour" in the crafted matrices: a small integer, exact in all three dtypes

Case = namedtuple("Case", "name gen arg seed N dtype container diag eps ms rho why claims")


def edge_capacity(rows):
    """restated from cluster.py (DBSCAN.fit: cap, eps_rule_dbscan: ecap)"""
    return max(EDGES_PER_ROW * rows, MIN_EDGE_CAP)


# ------------------------------------------------------------------------------------------------------------ the restatement
def neighbourhood_dtype(dtype):
    """the dtype in which sklearn evaluates `d <= eps` on a precomputed matrix of `dtype`"""
    return np.dtype(np.float32) if np.dtype(dtype) == np.float32 else np.dtype(np.float64)


def neighbourhoods(D, eps):
    """[columns k with D[i, k] <= eps] row by row, as sklearn's radius_neighbors finds them.  `eps` is the Python float the estimator
    was given: against a float32 row numpy compares float32(eps)."""
    D = np.asarray(D)
    dt = neighbourhood_dtype(D.dtype)
    eps = float(eps)
    return [np.nonzero(np.asarray(D[i], dtype=dt) <= eps)[0] for i in range(D.shape[0])]


def dbscan_ref(D, eps, min_samples, neigh=None):
    """sklearn's dbscan_inner restated: clusters are grown one at a time, in index order of their first core point, with a stack; only
    unlabelled points are labelled; a non-core point that is reached is labelled and not expanded -> (labels int64, core_sample_indices)"""
    neigh = neighbourhoods(D, eps) if neigh is None else neigh
    N = len(neigh)
    core = np.array([len(n) >= min_samples for n in neigh], dtype=bool)
    labels = np.full(N, -1, np.int64)
    label = 0
    for first in range(N):
        if labels[first] != -1 or not core[first]:
            continue
        i, stack = first, []
        while True:
            if labels[i] == -1:
                labels[i] = label
                if core[i]:
                    stack.extend(int(k) for k in neigh[i] if labels[k] == -1)
            if not stack:
                break
            i = stack.pop()
        label += 1
    return labels, np.nonzero(core)[0]


def hit_keys(neigh):
    """the neighbour pairs as sorted int64 keys i * N + k (what the region query's edge list holds)"""
    N = len(neigh)
    return np.sort(np.concatenate([i * N + n.astype(np.int64) for i, n in enumerate(neigh)])) if N else np.zeros(0, np.int64)


# ------------------------------------------------------------------------------------------------------------ generators
def _grid_points(N, rng, side):
    """N DISTINCT cells of a side x side integer grid"""
    cells = rng.permutation(side * side)[:N]
    return np.stack([cells // side, cells % side], axis=1).astype(np.float64)


def _gen_grid(N, rng, arg):
    """L1 distances of distinct integer grid points: small integers >= 1 off the diagonal, exact in float16"""
    side = arg or max(4, int(np.ceil(np.sqrt(4 * N))))
    p = _grid_points(N, rng, side)
    return np.abs(p[:, None, :] - p[None, :, :]).sum(-1)


def _gen_tenths(N, rng, arg):
    """the same integers times 0.1 (a float64 product, rounded once by the case's dtype): values no binary format holds exactly"""
    return _gen_grid(N, rng, arg) * 0.1


def _gen_plane(N, rng, arg):
    """Euclidean distances of uniform points in the unit square"""
    p = rng.random((N, 2))
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    return (d + d.T) / 2


def _gen_two(N, rng, arg):
    """[[0, x], [x, 0]]"""
    assert N == 2
    return np.array([[0.0, arg], [arg, 0.0]])


def _gen_dups(N, rng, arg):
    """duplicated rows: groups of 1 .. 6 identical points (zeros off the diagonal), L1 grid distances between the groups"""
    sizes = []
    while sum(sizes) < N:
        sizes.append(int(rng.integers(1, 7)))
    group = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)[:N])
    g = _gen_grid(len(sizes), rng, None)
    return g[group][:, group]


def _path_positions(N, rng, paths, doubled):
    """point i lies on path i % paths; along a path the points sit at consecutive integer positions in a random order.  `doubled`: every
    position that is a multiple of 4 holds two points"""
    path = np.arange(N) % paths
    pos = np.zeros(N, np.int64)
    for p in range(paths):
        idx = np.nonzero(path == p)[0]
        if doubled:
            slots = np.sort(np.concatenate([np.arange(len(idx)), np.arange(0, len(idx), 4)]))[:len(idx)]
            # slots = 0 0 1 2 3 4 4 5 ...: ranks along the path with every multiple of 4 twice
        else:
            slots = np.arange(len(idx))
        pos[idx] = slots[rng.permutation(len(idx))]
    return path, pos


def _gen_paths(N, rng, arg):
    """`arg` = (number of paths, doubled).  d = |pos_i - pos_j| clamped to FAR on one path, FAR between paths: at eps = 1 each path is one
    chain whose neighbours have unrelated indices"""
    paths, doubled = arg
    path, pos = _path_positions(N, rng, paths, doubled)
    d = np.minimum(np.abs(pos[:, None] - pos[None, :]), int(FAR)).astype(np.float64)
    d[path[:, None] != path[None, :]] = FAR
    return d


def _adjacency(N, pairs):
    d = np.full((N, N), FAR)
    np.fill_diagonal(d, 0.0)
    for a, b in pairs:
        d[a, b] = d[b, a] = 1.0
    return d


def ties_layout(ncl, ms):
    """The crafted border ties: `ncl` cliques of `ms` core points each and two border points.  Cluster 0 = {0} and the LAST ms - 1 core
    indices; cluster c >= 1 = a consecutive block after point 0.  Border `hi` touches one core of every cluster, in cluster 0 its
    highest-index core: its smallest-index core neighbour lies in cluster 1.  Border `lo` touches point 0 and one core of every other
    cluster: there the smallest-index core neighbour lies in cluster 0.  -> (N, clusters, hi, hi's core neighbours, lo, lo's)"""
    assert ms >= ncl + 2                                   # a border point counts itself and one core per cluster: still below ms
    clusters = [[0] + list(range(1 + (ncl - 1) * ms, ncl * ms))]
    for c in range(1, ncl):
        clusters.append(list(range(1 + (c - 1) * ms, 1 + c * ms)))
    hi, lo = ncl * ms, ncl * ms + 1
    hi_n = [clusters[0][-1]] + [cl[1] for cl in clusters[1:]]
    lo_n = [0] + [cl[2] for cl in clusters[1:]]
    return ncl * ms + 2, clusters, hi, hi_n, lo, lo_n


def _gen_ties(N, rng, arg):
    ncl, ms = arg
    n, clusters, hi, hi_n, lo, lo_n = ties_layout(ncl, ms)
    assert n == N
    pairs = [(a, b) for cl in clusters for a in cl for b in cl if a < b]
    pairs += [(hi, k) for k in hi_n] + [(lo, k) for k in lo_n]
    return _adjacency(N, pairs)


def _gen_outlier(N, rng, arg):
    """a clique of 4 cores {0..3}, border 4 next to core 3, point 5 next to the border only"""
    assert N == 6
    return _adjacency(6, [(a, b) for a in range(4) for b in range(a + 1, 4)] + [(3, 4), (4, 5)])


GENS = dict(grid=_gen_grid, tenths=_gen_tenths, plane=_gen_plane, two=_gen_two, dups=_gen_dups, paths=_gen_paths, ties=_gen_ties,
            outlier=_gen_outlier)
BIG_DIAG = 50.0


def base_matrix(case):
    """the case's symmetric float64 matrix before its dtype and container"""
    rng = np.random.default_rng(case.seed)
    d = GENS[case.gen](case.N, rng, case.arg)
    assert d.shape == (case.N, case.N) and np.array_equal(d, d.T)
    if case.diag == "above":                     # above every eps of the table: no point is its own neighbour
        np.fill_diagonal(d, BIG_DIAG if case.gen != "two" else 0.7)
    elif case.diag == "mixed":
        d[np.arange(1, case.N, 2), np.arange(1, case.N, 2)] = BIG_DIAG
    else:
        assert case.diag == "zero" and not d.diagonal().any()
    return d


_MATRICES = {}


def matrix(case):
    """the contiguous numpy matrix of the case in its dtype (what the sha256 pins); computed once per (generator, seed, N, dtype) and
    shared -- do not write to it"""
    key = (case.gen, case.arg, case.seed, case.N, case.diag, case.dtype)
    if key not in _MATRICES:
        for k in [k for k in _MATRICES if k[3] >= 1024 and k[:5] != key[:5]]:
            del _MATRICES[k]                      # (one large generator at a time: a 4096 x 4096 float64 matrix is 134 MB)
        _MATRICES[key] = np.ascontiguousarray(base_matrix(case).astype(case.dtype))
        _MATRICES[key].setflags(write=False)
    return _MATRICES[key]


def as_passed(case, device=None):
    """the object the case hands to the estimator: numpy array, CPU / GPU tensor, or a non-contiguous view with the same values.  The
    reference (sklearn, the restatement) always reads `matrix(case)` or this object as numpy: the values are the same."""
    D = matrix(case)
    c = case.container
    if c == "numpy":
        return D
    if c == "numpy_T":                            # a transposed view of a symmetric matrix: F-ordered, the same values
        out = D.T
        assert not out.flags.c_contiguous
        return out
    if c == "numpy_slice":                        # every other row and column of a 2N x 2N matrix
        big = np.zeros((2 * case.N, 2 * case.N), D.dtype) + D.dtype.type(7)
        big[::2, ::2] = D
        out = big[::2, ::2]
        assert not out.flags.c_contiguous
        return out
    import torch
    t = torch.from_numpy(np.array(D))
    if c == "cpu":
        return t
    if c == "cpu_T":
        return t.t().contiguous().t()             # strides (1, N)
    assert c == "gpu" and device is not None
    return t.to(device)


def as_numpy(X):
    return X if isinstance(X, np.ndarray) else X.cpu().numpy()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------------------ the table
def _build_table():
    cases = []

    def add(gen, N, dtype, eps, ms, why, container="numpy", diag="zero", arg=None, seed=None, rho=None, **claims):
        n = len(cases) + 1
        name = "d%02d_%s_n%d_%s_ms%d" % (n, gen, N, {"float64": "f64", "float32": "f32", "float16": "f16"}[dtype], ms)
        cases.append(Case(name, gen, arg, 700 + n if seed is None else seed, N, dtype, container, diag, float(eps), int(ms), rho, why, claims))

    f64, f32, f16 = "float64", "float32", "float16"
    # ---- the smallest matrices, min_samples against N
    add("grid", 1, f64, 0.5, 1, "N = 1: one row of one element, a singleton cluster", n_clusters=1, n_noise=0)
    add("grid", 1, f16, 0.5, 2, "N = 1, min_samples = N + 1: noise", n_clusters=0, n_noise=1)
    add("two", 2, f32, 0.1, 2, "the 2 x 2 example: float32(0.1) > 0.1, sklearn compares in float32 and hits", arg=0.1, f32_eps_matters=True, n_clusters=1)
    add("two", 2, f64, 0.1, 2, "the same values widened: float64(float32(0.1)) > 0.1, no hit, min_samples = N", arg=float(np.float32(0.1)), n_clusters=0, n_noise=2)
    add("two", 2, f16, 0.3, 2, "float16(0.3) > 0.3: sklearn widens float16 to float64, no hit", arg=0.3, f16_eps_would_matter=True, n_clusters=0)
    add("two", 2, f32, 0.7, 2, "float32(0.7) < 0.7: the rounded eps still holds the entry", arg=0.7, f32_eps_matters=False, n_clusters=1)
    add("two", 2, f64, 0.5, 2, "diagonal above eps: no point is its own neighbour, one neighbour each", arg=0.1, diag="above", n_clusters=0, n_noise=2)
    add("two", 2, f64, 0.5, 1, "the same at min_samples = 1: both core through each other", arg=0.1, diag="above", n_clusters=1)
    # ---- N around the 8-element boundary and one lane's worth; d == eps hits on small integers
    add("grid", 7, f64, 3, 2, "N < 8: every row but the first starts off the boundary", eps_equals_entries=True)
    add("grid", 7, f16, 3, 3, "the same in half: the last row's tail guard", eps_equals_entries=True)
    add("grid", 8, f32, 2, 3, "N = 8: every row is exactly one lane", eps_equals_entries=True)
    add("grid", 9, f64, 100, 9, "min_samples = N with eps above every entry: one cluster of all", all_hit=True, n_clusters=1, n_noise=0)
    add("grid", 9, f16, 100, 10, "min_samples = N + 1: N^2 hits and all noise", all_hit=True, n_clusters=0, n_noise=9)
    add("grid", 63, f16, 2, 4, "N = 63, half, rows off the boundary", container="cpu", eps_equals_entries=True)
    add("grid", 64, f32, 3, 5, "N = 64, float32", container="gpu", eps_equals_entries=True, rho=0.05)
    add("grid", 65, f64, 3, 10, "N = 65 as a GPU tensor", container="gpu", eps_equals_entries=True)
    add("grid", 65, f64, 3, 4, "a transposed (F-ordered) view of a symmetric matrix", container="numpy_T", eps_equals_entries=True, seed=716)
    add("grid", 64, f16, 3, 4, "a [::2, ::2] view of a 128 x 128 half matrix", container="numpy_slice", eps_equals_entries=True)
    add("grid", 64, f64, 3, 4, "a CPU tensor with strides (1, N)", container="cpu_T", eps_equals_entries=True)
    # ---- ordinary real-valued distances
    add("plane", 120, f64, 0.08, 4, "random points in the plane, the size of the old fixture", rho=0.02)
    add("plane", 120, f32, 0.08, 5, "the same in float32", container="cpu", seed=720)
    add("plane", 120, f16, 0.08, 5, "the same in half", seed=720, rho=0.02)
    add("plane", 120, f64, 1e-9, 1, "eps below every off-diagonal entry, min_samples = 1: N singletons", none_hit=True, n_clusters=120, n_noise=0)
    add("plane", 120, f64, 1e-9, 2, "the same at min_samples = 2: all noise", none_hit=True, seed=723, n_clusters=0, n_noise=120)
    add("plane", 120, f64, 0.2, 1, "mixed diagonal, min_samples = 1: a point above eps on its own diagonal is core through a neighbour only", diag="mixed")
    add("plane", 120, f64, 1e-9, 1, "mixed diagonal below every off-diagonal entry: the zero-diagonal points are singletons, the rest noise", diag="mixed",
        n_clusters=60, n_noise=60)
    add("plane", 120, f32, 0.1, 3, "diagonal above eps", diag="above")
    add("dups", 120, f64, 0.5, 3, "duplicated rows: zeros off the diagonal, groups of 3+ are clusters", zeros_off_diagonal=True)
    add("dups", 120, f16, 1, 2, "the same in half with d == eps hits", zeros_off_diagonal=True, eps_equals_entries=True)
    # ---- values no binary format holds: eps just below / above an entry of the rounded matrix
    add("tenths", 65, f32, 0.3, 4, "float32: entries float32(0.3) > 0.3 hit only against the rounded eps", f32_eps_matters=True)
    add("tenths", 65, f32, 0.7, 4, "float32: float32(0.7) < 0.7, rounding eps loses no hit", f32_eps_matters=False, seed=730)
    add("tenths", 65, f16, 0.3, 4, "half: entries float16(0.3) > 0.3 must NOT hit (float64 comparison)", f16_eps_would_matter=True, seed=730)
    add("tenths", 65, f16, 0.2, 4, "half: float16(0.2) < 0.2 hits", seed=730)
    # ---- N around one chunk of 512, the partial last chunk, large min_samples
    add("grid", 511, f16, 4, 10, "N = 511, half: a row spans two chunks", container="cpu", eps_equals_entries=True, rho=0.01)
    add("grid", 512, f64, 4, 10, "N = 512: exactly one chunk per row", eps_equals_entries=True, rho=0.01)
    add("grid", 512, f64, 0, 3, "(i) the eps rule's radius at rho = 0.6 holds more hits than the first edge list: the retry inside eps_rule_dbscan",
        seed=735, rho=0.6, chain_hits_above_capacity=True)
    add("grid", 513, f32, 4, 5, "N = 513: one chunk plus one element", container="gpu", eps_equals_entries=True, rho=0.01)
    add("grid", 520, f16, 12, 65, "N = 520 (N % 8 == 0, a partial second chunk); min_samples above the 64-edges-per-row budget", container="gpu",
        eps_equals_entries=True, counts_straddle=True)
    add("grid", 520, f64, 20, 200, "min_samples = 200", eps_equals_entries=True, counts_straddle=True, seed=738)
    add("grid", 1031, f64, 5, 10, "N = 1031: three chunks, odd rows", eps_equals_entries=True, rho=0.01)
    add("grid", 1031, f16, 5, 4, "the same in half as a GPU tensor", container="gpu", eps_equals_entries=True, seed=740)
    add("grid", 300, f64, 1000, 4, "(h) one clique of 300, eps above every entry: 90 000 hits against a first list of 65 536, the retry in fit", all_hit=True,
        hits_above_capacity=True, n_clusters=1, n_noise=0)
    # ---- structure: long components, numbering, borders
    add("paths", 4096, f64, 1, 3, "(c) one path of 4096 points in random index order: the deep tree of hook / union / flatten", arg=(1, False), seed=800,
        n_clusters=1, n_noise=0, border=2)
    add("paths", 4096, f16, 1, 3, "the same path as a half matrix", arg=(1, False), seed=800, n_clusters=1, n_noise=0, border=2)
    add("paths", 4096, f64, 1, 4, "(e) the same path at min_samples = 4: no core, all noise", arg=(1, False), seed=800, n_clusters=0, n_noise=4096)
    add("paths", 4096, f64, 1, 3, "(d) two interleaved paths: numbering by smallest core index", arg=(2, False), seed=801, n_clusters=2, n_noise=0, border=4)
    add("paths", 4096, f32, 1, 3, "(d) five interleaved paths", arg=(5, False), seed=802, container="gpu", n_clusters=5, n_noise=0, border=10)
    add("paths", 4096, f64, 1, 4, "(e) a path with every fourth position doubled: cores and non-cores alternate along it, each non-core a border of two clusters",
        arg=(1, True), seed=803, n_noise=2, cores_alternate=True)
    add("paths", 1031, f64, 1, 3, "three interleaved paths at N = 1031 for the one-read chain", arg=(3, False), seed=804, n_clusters=3, rho=0.002)
    add("ties", 10, f64, 1, 4, "(f) border ties between two clusters", arg=(2, 4), border_ties=2)
    add("ties", 17, f32, 1, 5, "(f) border ties between three clusters", arg=(3, 5), border_ties=3)
    add("outlier", 6, f64, 1, 4, "(g) a non-core point whose only neighbour is a border point: noise", noise_next_to_border=True)
    return tuple(cases)


CASES = _build_table()
BY_NAME = {c.name: c for c in CASES}
PLAIN = [c for c in CASES if c.eps > 0]                 # fit / fit_predict / region query at the case's own eps
CHAIN = [c for c in CASES if c.rho is not None]         # eps_rule_dbscan at the case's rho (N >= 64)


def numpy_eps_rule(dist, rho):
    """selftraining.py:289-293 on a materialised matrix -> (eps, count, top_num); the same lines as tests/grouping_ref.numpy_eps_rule
    (restated here so that the CPU suite needs no torch)"""
    tri = np.triu(dist, 1)
    tri = np.sort(tri[np.nonzero(tri)], axis=None)
    top = np.round(rho * tri.size).astype(int)
    return tri[:top].mean(), int(tri.size), int(top)


def chain_reference(case):
    """(eps, count, top) of the eps rule as the product defines it on a plain matrix: float32 is widened to float64 (the mean is a float64
    pairwise sum), half stays half (a float16 mean).  -> eps as the product returns it"""
    D = matrix(case)
    eps, cnt, top = numpy_eps_rule(D.astype(np.float64) if D.dtype == np.float32 else D, case.rho)
    return (eps if D.dtype == np.float16 else float(eps)), cnt, top


# ------------------------------------------------------------------------------------------------------------ claims
def check_claims(case, D=None):
    """assert the properties `case.claims` lists, from the restatement on the matrix as passed -> dict of what was measured"""
    D = matrix(case) if D is None else D
    N = case.N
    eps = case.eps if case.eps > 0 else float(chain_reference(case)[0])
    neigh = neighbourhoods(D, eps)
    counts = np.array([len(n) for n in neigh])
    nhits = int(counts.sum())
    labels, core = dbscan_ref(D, eps, case.ms, neigh)
    iscore = np.zeros(N, bool); iscore[core] = True
    off = D[~np.eye(N, dtype=bool)].astype(np.float64)
    m = dict(nhits=nhits, n_clusters=int(labels.max()) + 1, n_noise=int((labels < 0).sum()), border=int(((labels >= 0) & ~iscore).sum()))
    for k, want in case.claims.items():
        if k in ("n_clusters", "n_noise", "border"):
            assert m[k] == want, (case.name, k, m[k], want)
        elif k == "all_hit":
            assert nhits == N * N, (case.name, nhits)
        elif k == "none_hit":
            assert off.size and off.min() > eps and nhits == int((D.diagonal() <= eps).sum()), (case.name, nhits)
        elif k == "eps_equals_entries":
            assert int((off == eps).sum()) >= (N if N >= 16 else 4) and (off < eps).any() and (off > eps).any(), (case.name, int((off == eps).sum()))
        elif k == "zeros_off_diagonal":
            assert (off == 0).sum() >= N // 2
        elif k == "f32_eps_matters":
            assert D.dtype == np.float32 and (float(np.float32(eps)) != eps)
            wide = sum(int((D[i].astype(np.float64) <= eps).sum()) for i in range(N))
            assert (wide != nhits) == want, (case.name, wide, nhits)
            if want:
                assert not np.array_equal(dbscan_ref(D.astype(np.float64), eps, case.ms)[0], labels), (case.name, "the labels do not depend on it")
        elif k == "f16_eps_would_matter":
            assert D.dtype == np.float16 and float(np.float16(eps)) > eps
            inhalf = sum(int((D[i] <= np.float16(eps)).sum()) for i in range(N))
            assert inhalf > nhits, (case.name, inhalf, nhits)
        elif k == "counts_straddle":
            assert case.ms > EDGES_PER_ROW and (counts >= case.ms).any() and (counts < case.ms).any() and (counts == case.ms).any(), (
                case.name, counts.min(), counts.max())
        elif k == "hits_above_capacity":
            assert nhits > edge_capacity(N), (case.name, nhits, edge_capacity(N))
        elif k == "chain_hits_above_capacity":
            assert case.eps == 0 and nhits > edge_capacity(N) and 1.3 * case.rho < 1, (case.name, nhits, edge_capacity(N))
        elif k == "cores_alternate":
            # along the path (by position) core and non-core points follow each other many times; the non-cores inside it are border points
            _, pos = _path_positions(N, np.random.default_rng(case.seed), *case.arg)
            order = np.argsort(pos, kind="stable")
            flips = int((np.diff(iscore[order].astype(np.int8)) != 0).sum())
            assert flips >= N // 4 and m["border"] + m["n_noise"] == int((~iscore).sum()) and m["border"] > N // 8, (case.name, flips, m["border"])
        elif k == "border_ties":
            n, clusters, hi, hi_n, lo, lo_n = ties_layout(*case.arg)
            assert want == len(clusters) and [int(labels[cl[0]]) for cl in clusters] == list(range(want))
            for b, nb in ((hi, hi_n), (lo, lo_n)):
                assert not iscore[b] and iscore[nb].all() and sorted(int(x) for x in neigh[b]) == sorted(nb + [b])
                assert sorted(int(labels[x]) for x in nb) == list(range(want))              # one candidate id per cluster
            assert int(labels[min(hi_n)]) > 0 and int(labels[hi]) == 0                       # smallest-index core neighbour: a larger id
            assert int(labels[min(lo_n)]) == 0 and int(labels[lo]) == 0
            m["candidates"] = [sorted(int(labels[x]) for x in nb) for nb in (hi_n, lo_n)]
        elif k == "noise_next_to_border":
            assert labels.tolist() == [0, 0, 0, 0, 0, -1] and core.tolist() == [0, 1, 2, 3] and neigh[5].tolist() == [4, 5]
        else:
            raise KeyError(k)
    m.update(labels=labels, core=core, counts=counts, neigh=neigh, eps=eps)
    return m


def branches(case):
    """where the case sits relative to the size-dependent branches of the row streaming (csrc/matview.h RowStream, 8 elements per lane,
    512 per chunk)"""
    N = case.N
    return dict(rows_aligned=N % 8 == 0, below_lane=N < 8, chunks=(N + 511) // 512, exact_chunks=N % 512 == 0,
                last_row_tail_inside_lane=(N * N) % 8 != 0)
