"""numpy restatement of sklearn 1.7.2's `_affinity_propagation` (float64, affinity='precomputed') and the inputs of the affinity
propagation tests.  It is written the way csrc/affinity.hip computes -- entry by entry, with the column sums as an explicit loop over the
rows in ascending order -- and it reproduces sklearn's `cluster_centers_indices_`, `labels_` and `n_iter_` exactly
(tests/test_affinity_host.py holds it to the recorded sklearn results of tests/golden/affinity_cases.npz, and to sklearn itself where
it can be imported).  Three facts carry it:
  1. every damped update rounds twice (`R *= d; R += tmp` with `tmp *= 1 - d` before it): no fused multiply-add;
  2. `np.sum(tmp, axis=0)` on a C-contiguous float64 matrix adds the rows in ascending order, one running sum per column;
  3. `np.argmax` takes the first maximum.
The inputs are generated from seeds; no matrix is stored."""
import hashlib
from functools import lru_cache

import numpy as np


def colsum_seq(T):
    """sum over the rows in ascending order, one running sum per column (what np.sum(T, axis=0) does on a C-contiguous matrix)"""
    s = T[0].copy()
    for r in range(1, T.shape[0]):
        s = s + T[r]
    return s


def prepare(X, preference=None, seed=0):
    """-> (S with preference and noise applied, the preference as an array)"""
    S = np.array(X, dtype=np.float64, copy=True)
    n = S.shape[0]
    if preference is None:
        preference = np.median(S)
    preference = np.asarray(preference, dtype=np.float64)
    S.flat[::n + 1] = preference
    rs = np.random.RandomState(seed)
    S += (np.finfo(np.float64).eps * S + np.finfo(np.float64).tiny * 100) * rs.standard_normal(size=(n, n))
    return S, preference


def affinity_propagation(X, damping=0.5, max_iter=200, convergence_iter=15, preference=None, seed=0, snapshots=()):
    """-> dict(centers, labels, n_iter, converged, S, A, R, snaps={count: (A, R) after that many iterations})"""
    S, _ = prepare(X, preference, seed)
    n = S.shape[0]
    A = np.zeros((n, n)); R = np.zeros((n, n)); e = np.zeros((n, convergence_iter), dtype=bool); ind = np.arange(n)
    conv, snaps = False, {}
    omd = 1 - damping
    for it in range(max_iter):
        T = A + S
        I = np.argmax(T, axis=1); Y = T[ind, I]; T[ind, I] = -np.inf; Y2 = T.max(axis=1)
        Rn = S - Y[:, None]; Rn[ind, I] = S[ind, I] - Y2
        R = R * damping + Rn * omd
        Rp = np.maximum(R, 0); Rp.flat[::n + 1] = R.flat[::n + 1]
        T = Rp - colsum_seq(Rp)
        dA = np.diag(T).copy(); T = np.clip(T, 0, np.inf); T.flat[::n + 1] = dA
        A = A * damping - T * omd
        E = (np.diag(A) + np.diag(R)) > 0; e[:, it % convergence_iter] = E; K = E.sum()
        if it + 1 in snapshots:
            snaps[it + 1] = (A.copy(), R.copy())
        if it >= convergence_iter:
            se = e.sum(axis=1)
            if ((se == convergence_iter) | (se == 0)).all() and K > 0:
                conv = True
                break
    out = dict(n_iter=it + 1, converged=conv, S=S, A=A, R=R, snaps=snaps)
    I = np.flatnonzero(E); K = I.size
    if K == 0:
        out.update(centers=np.array([], dtype=np.int64), labels=-np.ones(n, dtype=np.int64))
        return out
    c = np.argmax(S[:, I], axis=1); c[I] = np.arange(K)
    for k in range(K):
        ii = np.nonzero(c == k)[0]
        I[k] = ii[np.argmax(colsum_seq(S[ii[:, None], ii]))]
    c = np.argmax(S[:, I], axis=1); c[I] = np.arange(K); lab = I[c]
    cen = np.unique(lab)
    out.update(centers=cen, labels=np.searchsorted(cen, lab))
    return out


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


# ---- inputs
def _unit_rows(x):
    """rows scaled to unit length; the squares are added feature by feature, so that no library's summation order enters the inputs"""
    n2 = np.zeros(x.shape[0])
    for k in range(x.shape[1]):
        n2 = n2 + x[:, k] * x[:, k]
    return x / np.sqrt(n2)[:, None]


def blobs(N, P, d, noise, seed):
    """Euclidean distances of P noisy blobs on the unit sphere (the Gram matrix is accumulated feature by feature, not by a BLAS
    call: the same bits on every machine)"""
    rng = np.random.default_rng(seed)
    c = _unit_rows(rng.standard_normal((P, d)))
    x = _unit_rows(c[np.arange(N) % P] + noise * rng.standard_normal((N, d)))
    G = np.zeros((N, N))
    for k in range(d):
        G = G + np.outer(x[:, k], x[:, k])
    D = np.sqrt(np.maximum(0, 2 - 2 * G)); np.fill_diagonal(D, 0)
    return D


def jaccard_like(N, P, seed):
    """quantised distances with many exact ties and many exact 1.0 entries, like a re-ranked matrix"""
    D = blobs(N, P, 32, 0.08, seed); D = np.minimum(1.0, np.round(D * 1.2, 2))
    return (D + D.T) / 2


_INPUTS = {
    "a": lambda: -blobs(257, 16, 32, 0.05, 1),
    "b": lambda: -blobs(512, 32, 64, 0.05, 2),
    "c": lambda: -jaccard_like(384, 24, 4),
    "d": lambda: -blobs(1000, 40, 64, 0.06, 3),
    "e": lambda: -jaccard_like(640, 40, 5),
    "f": lambda: -blobs(300, 10, 16, 0.1, 6),
}


def _pref_vector():
    return -2.0 - np.random.default_rng(11).random(300)


# name -> (input key, estimator keywords).  h*: the input of (b) stopped early (max_iter 1: K = 0; 2: unconverged with many small clusters)
CASES = {
    "a": ("a", dict(random_state=0)),
    "a_seed5": ("a", dict(random_state=5)),
    "b": ("b", dict(random_state=0)),
    "c": ("c", dict(random_state=0)),
    "d": ("d", dict(damping=0.9, random_state=0)),
    "e": ("e", dict(damping=0.75, random_state=0)),
    "f": ("f", dict(preference=-3.0, random_state=0)),
    "g": ("f", dict(preference="vector", random_state=0)),
    "h1": ("b", dict(max_iter=1, random_state=0)),
    "h2": ("b", dict(max_iter=2, random_state=0)),
    "h10": ("b", dict(max_iter=10, random_state=0)),
    "h16": ("b", dict(max_iter=16, random_state=0)),
    "h20": ("b", dict(max_iter=20, random_state=0)),
}
# what the issue recorded from sklearn on the CPU: (n_iter_, K); None where it was not recorded
EXPECTED = {"a": (22, 16), "b": (23, 32), "c": (22, 31), "d": (52, 40), "e": (48, 61), "f": (27, 10), "g": None,
            "h1": (1, 0), "h2": (2, 121), "h10": (10, 32), "h16": (16, 32), "h20": (20, 32)}


@lru_cache(maxsize=None)
def case_input(key):
    X = _INPUTS[key]()
    X.setflags(write=False)
    return X


def case_kwargs(name):
    """estimator keywords of a case (the preference vector materialised)"""
    kw = dict(CASES[name][1])
    if isinstance(kw.get("preference"), str):
        kw["preference"] = _pref_vector()
    return kw


@lru_cache(maxsize=None)
def case_result(name, snapshots=(1, 2)):
    """the restatement's run of a case, computed once and shared (treat as read-only)"""
    kw = case_kwargs(name)
    return affinity_propagation(case_input(CASES[name][0]), damping=kw.get("damping", 0.5), max_iter=kw.get("max_iter", 200),
                                preference=kw.get("preference"), seed=kw["random_state"], snapshots=snapshots)
