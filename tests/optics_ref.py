"""What the OPTICS tests share (tests/test_optics_host.py, tests/test_gpu_optics.py, tools/make_optics_golden.py): the case table, the
matrices rebuilt from seeds, and a plain numpy restatement of sklearn 1.7.2's `compute_optics_graph(metric='precomputed')`,
`cluster_optics_dbscan` and `cluster_optics_xi`.  tests/golden/optics_cases.npz holds what sklearn itself gave for every case and a
sha256 of every rebuilt matrix, so a generator that drifts is noticed before anything is compared.

The matrices use elementwise IEEE operations only (no BLAS, no library reduction) and numpy's frozen `RandomState` streams, so that
every machine rebuilds the same bits.
"""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optics_cases.npz")
INF = float("inf")


def _xi(xi=0.05, mcs=None, pc=True):
    return dict(method="xi", xi=xi, min_cluster_size=mcs, predecessor_correction=pc, eps=None)


def _eps(eps):
    return dict(method="dbscan", eps=eps, xi=0.05, min_cluster_size=None, predecessor_correction=True)


# kind: 'half'  float16-derived distances (tie-heavy), a non-zero diagonal          -> handed over as float16, float32 or float64
#       'dup'   genuine float64 distances of points of which a fifth are exact copies (zeros off the diagonal)
#       'f64'   genuine float64 distances
#       'rerank' the float64 final_dist stored in another golden file
# max_eps: inf | a finite value that leaves some core distances and several reachabilities infinite | one below every distance.
# cuts: the label extractions run on the case's ordering; `full` marks the cases whose every cut must show at least 2 clusters and at
# least one noise point (the others are too small or degenerate by construction: their labels are compared all the same).
CASES = [
    dict(name="n2", N=2, kind="f64", seed=1, min_samples=2, max_eps=INF, cuts=[_xi(), _eps(10.0)], full=False),
    dict(name="n7", N=7, kind="half", seed=2, min_samples=2, max_eps=INF, cuts=[_xi(), _eps(0.5)], full=False),
    dict(name="n7_all", N=7, kind="f64", seed=3, min_samples=7, max_eps=INF, cuts=[_xi()], full=False),
    dict(name="n64_half", N=64, kind="half", seed=4, min_samples=4, max_eps=INF, cuts=[_xi(), _xi(0.01), _xi(0.3), _eps(0.4)], full=True),
    dict(name="n64_tiny", N=64, kind="half", seed=4, min_samples=4, max_eps=1e-3, cuts=[_xi(), _eps(1e-3)], full=False),       # every reachability inf
    dict(name="n65_f64", N=65, kind="f64", seed=5, min_samples=9, max_eps=INF, cuts=[_xi(mcs=5), _xi(pc=False), _eps(0.5)], full=True),
    dict(name="n65_all", N=65, kind="half", seed=6, min_samples=65, max_eps=INF, cuts=[_xi()], full=False),                     # min_samples = N
    dict(name="n257_half", N=257, kind="half", seed=7, min_samples=4, max_eps=0.45, cuts=[_xi(), _xi(0.01, mcs=0.03), _xi(0.3, pc=False), _eps(0.3), _eps(0.45)],
         full=True),
    dict(name="n257_dup", N=257, kind="dup", seed=8, min_samples=0.05, max_eps=INF, cuts=[_xi(), _xi(0.01, mcs=6, pc=False), _eps(0.35)], full=True),
    dict(name="n513_f64", N=513, kind="f64", seed=9, min_samples=9, max_eps=0.5, cuts=[_xi(), _xi(0.3, mcs=0.02), _eps(0.4)], full=True),
    dict(name="n513_half2", N=513, kind="half", seed=10, min_samples=2, max_eps=INF, cuts=[_xi(0.05, mcs=4), _eps(0.3)], full=True),
    dict(name="n3001_half", N=3001, kind="half", seed=11, min_samples=4, max_eps=INF, cuts=[_xi(), _eps(0.3)], full=True),
    dict(name="n3001_f64", N=3001, kind="f64", seed=12, min_samples=9, max_eps=0.4, cuts=[_xi(0.05, mcs=0.005), _eps(0.35)], full=True),
    # the final_dist of an existing re-rank golden (lambda 0.3): on the GPU the matrix is the mode-0 handle re_ranking_device builds from
    # that golden's features, read through its compact form
    dict(name="rerank_n256", N=256, kind="rerank", file="rerank_n256_l03_ref.npz", lambda_value=0.3, min_samples=4, max_eps=INF,
         cuts=[_xi(0.01), _xi(0.005, pc=False), _eps(0.6)], full=True),
]
BY_NAME = {c["name"]: c for c in CASES}

_MATS = {}


def points(N, seed, dim=5):
    """clustered points: tight groups of 6 to 30 around centres in a box, and a tenth of the points spread over the whole box"""
    rs = np.random.RandomState(seed)
    n_out = max(1, N // 10) if N >= 8 else 0
    n_in = N - n_out
    n_groups = max(1, min(n_in // 12, 40)) if N >= 24 else 1
    centres = rs.uniform(-2.0, 2.0, size=(n_groups, dim))
    which = rs.randint(0, n_groups, size=n_in)
    which[:n_groups] = np.arange(n_groups)[:n_in]
    pts = centres[which] + 0.05 * rs.standard_normal((n_in, dim))
    out = rs.uniform(-2.5, 2.5, size=(n_out, dim))
    allp = np.concatenate([pts, out], axis=0)
    return allp[rs.permutation(N)]


def _distances(p):
    """euclidean distances with elementwise operations only (the same bits on every machine); symmetric, zero diagonal"""
    sq = np.zeros((len(p), len(p)))
    for k in range(p.shape[1]):
        d = p[:, k, None] - p[None, :, k]
        sq += d * d
    return np.sqrt(sq)


def matrix(case):
    """the case's matrix as the tests hand it over: float16 for kind 'half' (its float64 copy is what sklearn saw), else float64"""
    key = case["name"] if BY_NAME.get(case["name"]) is case else None
    if key in _MATS:
        return _MATS[key]
    if case["kind"] == "rerank":
        with np.load(os.path.join(os.path.dirname(GOLDEN), case["file"])) as z:
            D = z["final"]
        assert D.dtype == np.float64 and D.shape == (case["N"], case["N"])
        D.setflags(write=False)
        _MATS[key] = D
        return D
    N, kind, seed = case["N"], case["kind"], case["seed"]
    p = points(N, seed)
    if kind == "dup":
        rs = np.random.RandomState(seed + 1000)
        src = rs.randint(0, N, size=N // 5)
        dst = rs.permutation(N)[:N // 5]
        p[dst] = p[src]
    D = _distances(p)
    if kind == "half":
        D = D.astype(np.float16)
        rs = np.random.RandomState(seed + 2000)
        D[np.arange(N), np.arange(N)] = (0.002 + 0.02 * rs.uniform(size=N)).astype(np.float16)      # a non-zero diagonal
    D.setflags(write=False)
    if key is not None:
        _MATS[key] = D
    return D


def sha(D):
    return hashlib.sha256(np.ascontiguousarray(D).tobytes()).hexdigest()


def resolve_size(size, n):
    """sklearn's min_samples / min_cluster_size: an int as it is, a fraction -> max(2, int(f * n))"""
    assert size <= n
    return max(2, int(size * n)) if size <= 1 else int(size)


# ---------------------------------------------------------------------------------------------------------------- the graph
def optics_graph(X, min_samples, max_eps):
    """compute_optics_graph(metric='precomputed') of sklearn 1.7.2, one vectorised numpy step per point.  The core distance is the
    min_samples-th smallest entry of the row, the diagonal entry included as it stands; np.around(., 15) is applied to the core
    distances and to every candidate reachability; the matrix is widened to float64 first."""
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    k = resolve_size(min_samples, n)
    core = np.partition(X, k - 1, axis=1)[:, k - 1].copy()
    core[core > max_eps] = np.inf
    core = np.around(core, 15)
    reach = np.full(n, np.inf)
    pred = np.full(n, -1, dtype=np.int64)
    done = np.zeros(n, dtype=bool)
    ordering = np.zeros(n, dtype=np.int64)
    for t in range(n):
        idx = np.flatnonzero(~done)
        p = idx[np.argmin(reach[idx])]             # the first minimum: the smallest index among ties, also when every value is inf
        done[p] = True
        ordering[t] = p
        if core[p] == np.inf:
            continue
        row = X[p]
        j = np.flatnonzero(~done & (row <= max_eps))
        r = np.around(np.maximum(row[j], core[p]), 15)
        better = r < reach[j]
        reach[j[better]] = r[better]
        pred[j[better]] = p
    return ordering, core, reach, pred


# ---------------------------------------------------------------------------------------------------------------- the eps cut
def cut_dbscan(reach, core, ordering, eps):
    """walk the ordering: a point that is not reachable at eps opens a new cluster when it is core at eps, else it is noise"""
    labels = np.empty(len(reach), dtype=np.int64)
    current = -1
    for p in ordering:
        if reach[p] > eps:
            if core[p] <= eps:
                current += 1
                labels[p] = current
            else:
                labels[p] = -1
        else:
            labels[p] = current
    return labels


# ---------------------------------------------------------------------------------------------------------------- xi
def cut_xi(reach, pred, ordering, min_samples, min_cluster_size=None, xi=0.05, predecessor_correction=True):
    """cluster_optics_xi of sklearn 1.7.2 in plain loops -> (labels, clusters [n, 2])"""
    n = len(reach)
    ms = resolve_size(min_samples, n)
    mcs = ms if min_cluster_size is None else resolve_size(min_cluster_size, n)
    r = np.append(reach[ordering], np.inf)
    pp = pred[ordering]
    xc = 1 - xi
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = r[:-1] / r[1:]
    s_up, s_down, up, down = ratio <= xc, ratio >= 1 / xc, ratio < 1, ratio > 1

    def extend(steep, other, start):
        end, flat, i = start, 0, start
        while i < n:
            if steep[i]:
                end, flat = i, 0
            elif other[i]:
                return end
            else:
                flat += 1
                if flat > ms:
                    return end
            i += 1
        return end

    def prune(areas, mib):
        if np.isinf(mib):
            return []
        keep = [a for a in areas if mib <= r[a["s"]] * xc]
        for a in keep:
            a["mib"] = max(a["mib"], mib)
        return keep

    areas, clusters, index, mib = [], [], 0, 0.0
    for i in range(n):
        if not (s_up[i] or s_down[i]) or i < index:
            continue
        mib = max(mib, r[index:i + 1].max())
        areas = prune(areas, mib)
        if s_down[i]:
            e = extend(s_down, up, i)
            areas.append({"s": i, "e": e, "mib": 0.0})
            index = e + 1
            mib = r[index]
            continue
        ue = extend(s_up, down, i)
        index = ue + 1
        mib = r[index]
        new = []
        for a in areas:
            cs, ce = a["s"], ue
            if r[ce + 1] * xc < a["mib"]:
                continue
            top = r[a["s"]]
            if top * xc >= r[ce + 1]:
                while r[cs + 1] > r[ce + 1] and cs < a["e"]:
                    cs += 1
            elif r[ce + 1] * xc >= top:
                while r[ce - 1] > top and ce > i:
                    ce -= 1
            if predecessor_correction:
                ok = False
                while cs < ce:
                    if r[cs] > r[ce] or pp[ce] in ordering[cs:ce]:
                        ok = True
                        break
                    ce -= 1
                if not ok:
                    continue
            if ce - cs + 1 < mcs or cs > a["e"] or ce < i:
                continue
            new.append((cs, ce))
        clusters.extend(new[::-1])
    clusters = np.array(clusters)
    plot_labels = np.full(n, -1, dtype=np.int64)
    nxt = 0
    for cs, ce in clusters:
        if (plot_labels[cs:ce + 1] == -1).all():
            plot_labels[cs:ce + 1] = nxt
            nxt += 1
    labels = np.empty(n, dtype=np.int64)
    labels[ordering] = plot_labels
    return labels, clusters


def run_cut(cut, ordering, core, reach, pred, min_samples, max_eps):
    """the restatement's labels (and hierarchy, or None) of one cut"""
    if cut["method"] == "xi":
        return cut_xi(reach, pred, ordering, min_samples, cut["min_cluster_size"], cut["xi"], cut["predecessor_correction"])
    eps = max_eps if cut["eps"] is None else cut["eps"]
    return cut_dbscan(reach, core, ordering, eps), None


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
