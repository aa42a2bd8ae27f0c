"""Metric learners -- host-side mirror of reid/metric_learning/ (__init__.py:9-25, euclidean.py, kissme.py).

`get_metric('euclidean' | 'kissme')` builds the two learners the reference keeps in its own tree.  The other seven names of its factory
('itml', 'lmnn', 'lsml', 'sdml', 'nca', 'lfda', 'rca') are thin imports of the `metric_learn` library and raise a KeyError that says so.

KISSME.fit (kissme.py:33-55) on the device (csrc/kissme.hip): the reference masks two n x n int64 meshgrids to list the pairs and
multiplies the gathered difference matrices on the CPU.  Here

    ssg_kissme_index        stable counting sort of the class ids + two int64 scans: every pair is addressed by its position in the
                            reference's order (b ascending, a ascending inside b)
    one blocking read       num_matches, num_non_matches
    rng.choice(...)         on the HOST, called exactly as the reference calls it (a serial Fisher-Yates over num_non_matches elements that
                            numpy already does): the stream is consumed identically by construction
    ssg_kissme_match_pairs / ssg_kissme_unrank     the index pairs of C1 / of the sampled C0
    ssg_pairdiff_cov_f64    C = sum (x_a - x_b)(x_a - x_b)^T / num_matches in float64 on the FP64 matrix cores, twice

and the d x d tail (inv, symmetrisation, validate_cov_matrix, cholesky) in float64 numpy on the host, like the reference.  `M_` is float64, as
the reference's is even for float32 features (its `/ num_matches` divides by an np.int64).  There is no CPU fallback for the pair stage."""
import numpy as np

_METRIC_LEARN = ("itml", "lmnn", "lsml", "sdml", "nca", "lfda", "rca")

STAGE_NAMES = ("ia1", "ib1", "p", "ia0", "ib0", "C1", "C0", "M_raw")


def validate_cov_matrix(M):
    """kissme.py:7-23 with its semantics: symmetrise, then until cholesky succeeds add a multiple of the identity.  As in the reference
    the shift is NOT taken from the smallest eigenvalue: `min_eig` is the minimum of the eigenVECTOR matrix `v` of np.linalg.eig (and
    np.spacing of that value, which is negative for a negative value), scaled by k^2 in round k.  The input is not modified; the
    reference's in-place `+=` acts on its own symmetrised copy too."""
    M = (np.asarray(M) + np.asarray(M).T) * 0.5
    k = 0
    eye = np.eye(M.shape[0])
    while True:
        try:
            np.linalg.cholesky(M)
            break
        except np.linalg.LinAlgError:
            k += 1
            _, v = np.linalg.eig(M)
            min_eig = v.min()
            M += (-min_eig * k * k + np.spacing(min_eig)) * eye
    return M


def _is_tensor(x):
    import sys
    torch = sys.modules.get("torch")
    return torch is not None and torch.is_tensor(x)


class Euclidean(object):
    """euclidean.py: M = I, transform is the identity"""

    def __init__(self):
        self.M_ = None

    def metric(self):
        return self.M_

    def fit(self, X):
        self.M_ = np.eye(X.shape[1])
        self.X_ = X

    def transform(self, X=None):
        if X is None:
            return self.X_
        return X


def _stream(rng):
    """the object whose .choice the reference's line 46 calls: np.random itself, a RandomState, or a fresh RandomState(seed)"""
    if rng is np.random or isinstance(rng, np.random.RandomState):
        return rng
    if isinstance(rng, (int, np.integer)) and not isinstance(rng, (bool, np.bool_)):
        return np.random.RandomState(int(rng))
    raise TypeError("rng must be np.random, a np.random.RandomState or an int seed, not %s (np.random.Generator streams are not what the "
                    "reference consumes)" % type(rng).__name__)


def _dev():
    import torch
    from . import _lib
    if not torch.cuda.is_available():
        raise _lib.SSGError("ssg_amd.metric_learning.KISSME runs on the GPU only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def pair_index(y, dev=None):
    """ssg_kissme_index of the labels y (any integer or float array; np.unique makes the dense ids) -> dict of device tensors
    den, cls_ptr, members, rank, m_scan, nm_scan and the ints n, G"""
    import torch
    from . import _lib
    from ._lib import check, ptr, stream
    dev = _dev() if dev is None else dev
    y = np.asarray(y.detach().cpu().numpy() if _is_tensor(y) else y).reshape(-1)
    n = int(y.shape[0])
    uniq, inv = np.unique(y, return_inverse=True)
    G = int(uniq.shape[0])
    if n < 1:
        raise ValueError("KISSME: no rows")
    ix = {"n": n, "G": G,
          "den": torch.from_numpy(np.ascontiguousarray(inv.reshape(-1).astype(np.int32))).to(dev),
          "cls_ptr": torch.empty(G + 1, dtype=torch.int32, device=dev), "members": torch.empty(n, dtype=torch.int32, device=dev),
          "rank": torch.empty(n, dtype=torch.int32, device=dev),
          "scans": torch.empty((2, n + 1), dtype=torch.int64, device=dev)}
    ix["m_scan"], ix["nm_scan"] = ix["scans"][0], ix["scans"][1]
    check(_lib.lib().ssg_kissme_index(ptr(ix["den"]), n, G, ptr(ix["cls_ptr"]), ptr(ix["members"]), ptr(ix["rank"]), ptr(ix["m_scan"]),
                                      ptr(ix["nm_scan"]), stream()), "ssg_kissme_index")
    return ix


def match_pairs(ix, P1):
    import torch
    from . import _lib
    from ._lib import check, ptr, stream
    dev = ix["den"].device
    ia = torch.empty(P1, dtype=torch.int32, device=dev); ib = torch.empty(P1, dtype=torch.int32, device=dev)
    check(_lib.lib().ssg_kissme_match_pairs(ptr(ix["den"]), ptr(ix["rank"]), ptr(ix["cls_ptr"]), ptr(ix["members"]), ptr(ix["m_scan"]),
                                            ix["n"], ix["G"], P1, ptr(ia), ptr(ib), stream()), "ssg_kissme_match_pairs")
    return ia, ib


def unrank(ix, pos):
    """the non-matching pairs at the int64 positions `pos` (host array or device tensor) of the reference's order"""
    import torch
    from . import _lib
    from ._lib import check, ptr, stream
    dev = ix["den"].device
    pos = torch.as_tensor(np.ascontiguousarray(np.asarray(pos, dtype=np.int64)) if not _is_tensor(pos) else pos).to(dev, torch.int64).contiguous()
    T = int(pos.numel())
    ia = torch.empty(T, dtype=torch.int32, device=dev); ib = torch.empty(T, dtype=torch.int32, device=dev)
    check(_lib.lib().ssg_kissme_unrank(ptr(pos), T, ptr(ix["den"]), ptr(ix["rank"]), ptr(ix["cls_ptr"]), ptr(ix["members"]), ptr(ix["nm_scan"]),
                                       ix["n"], ix["G"], ptr(ia), ptr(ib), stream()), "ssg_kissme_unrank")
    return ia, ib


def pairdiff_cov(X, ia, ib, divisor):
    """C [d16, d16] float64 on the device; X [n, d16] float32 contiguous on the device with d16 % 16 == 0"""
    import torch
    from . import _lib
    from ._lib import check, ptr, stream
    n, d = X.shape
    C = torch.empty((d, d), dtype=torch.float64, device=X.device)
    check(_lib.lib().ssg_pairdiff_cov_f64(ptr(X), n, X.stride(0), ptr(ia), ptr(ib), int(ia.numel()), d, float(divisor), ptr(C), stream()),
          "ssg_pairdiff_cov_f64")
    return C


def _padded(X, dev, mult):
    """X as float32 [n, d rounded up to `mult`] on dev, zero columns appended"""
    import torch
    X = torch.as_tensor(X).to(dev, torch.float32)
    pad = (-X.shape[1]) % mult
    if pad:
        X = torch.nn.functional.pad(X, (0, pad))
    return X.contiguous()


class KISSME(object):
    """kissme.py:26-55.  fit(X, y=None, rng=np.random, stages=None): X [n, d] numpy array or tensor on any device, y any integer or
    float label array.  `rng` is np.random (the global legacy stream, what the reference consumes), a np.random.RandomState, or an int
    seed for a fresh RandomState.  `stages`, a dict, receives ia1, ib1, p, ia0, ib0 (host int arrays), C1, C0 and M_raw (float64, M before
    validate_cov_matrix)."""

    def __init__(self):
        self.M_ = None
        self._w = None

    def metric(self):
        return self.M_

    def fit(self, X, y=None, rng=np.random, stages=None):
        import torch
        rs = _stream(rng)
        if X.ndim != 2:
            raise ValueError("KISSME.fit: X must be [n, d]")
        n, d = int(X.shape[0]), int(X.shape[1])
        if y is None:
            # kissme.py:35-36 labels every row with its own class: no pair matches and C1 is 0 / 0
            raise ValueError("KISSME.fit: no matching pair (y=None gives every row a class of its own; the reference divides 0 by 0)")
        dev = _dev()
        Xd = _padded(X, dev, 16)
        ix = pair_index(y, dev)
        if ix["n"] != n:
            raise ValueError("KISSME.fit: %d labels for %d rows" % (ix["n"], n))
        totals = ix["scans"][:, n].cpu()                                    # the one blocking read
        num_matches, num_non = int(totals[0]), int(totals[1])
        if num_matches == 0:
            raise ValueError("KISSME.fit: no matching pair (every row has a class of its own; the reference divides 0 by 0)")
        p = rs.choice(num_non, num_matches, replace=False)                  # kissme.py:46; numpy's ValueError when num_non < num_matches
        ia1, ib1 = match_pairs(ix, num_matches)
        ia0, ib0 = unrank(ix, p)
        C1 = pairdiff_cov(Xd, ia1, ib1, num_matches)
        C0 = pairdiff_cov(Xd, ia0, ib0, num_matches)
        C = torch.stack([C1, C0]).cpu().numpy()[:, :d, :d]
        C1, C0 = np.ascontiguousarray(C[0]), np.ascontiguousarray(C[1])
        M_raw = np.linalg.inv(C1) - np.linalg.inv(C0)                        # a singular C1 is numpy's LinAlgError, as in the reference
        if stages is not None:
            stages.update(ia1=ia1.cpu().numpy(), ib1=ib1.cpu().numpy(), p=np.asarray(p), ia0=ia0.cpu().numpy(), ib0=ib0.cpu().numpy(),
                          C1=C1, C0=C0, M_raw=M_raw)
        self.M_ = validate_cov_matrix(M_raw)
        self.X_ = X
        self._w = None
        return self

    def transformer(self):
        """the lower Cholesky factor G of M_ = G G^T"""
        return np.linalg.cholesky(self.M_)

    def _weight(self, dev):
        """w = G^T as float32 [d, d rounded up to 32] on dev, made once per fit and device: transform is x w^T = x G"""
        import torch
        if self._w is None or self._w.device != dev:
            Gt = np.ascontiguousarray(self.transformer().T.astype(np.float32))
            self._w = _padded(torch.from_numpy(Gt), dev, 32)
        return self._w

    def transform(self, X=None):
        """X G in float32 on ssg_linear_fwd_f32 (the reference yields float64): ||(x - y) G||^2 = (x - y)^T M_ (x - y).  A tensor comes back
        on its own device, a numpy array as numpy."""
        import torch
        from . import _lib
        from ._lib import check, ptr, stream
        if self.M_ is None:
            raise ValueError("KISSME.transform: fit first")
        if X is None:
            X = self.X_
        is_t = torch.is_tensor(X)
        if X.ndim != 2 or int(X.shape[1]) != self.M_.shape[0]:
            raise ValueError("KISSME.transform: X must be [rows, %d]" % self.M_.shape[0])
        dev = _dev()
        w = self._weight(dev)
        x = _padded(X, dev, 32)
        B, K = x.shape
        N = int(self.M_.shape[0])
        out = torch.empty((B, N), dtype=torch.float32, device=dev)
        if B:
            check(_lib.lib().ssg_linear_fwd_f32(ptr(x), ptr(w), None, ptr(out), B, K, N, stream()), "ssg_linear_fwd_f32")
        return out.to(X.device) if is_t else out.cpu().numpy()


_FACTORY = {"euclidean": Euclidean, "kissme": KISSME}


def get_metric(algorithm, *args, **kwargs):
    """reid/metric_learning/__init__.py:22-25"""
    if algorithm in _FACTORY:
        return _FACTORY[algorithm](*args, **kwargs)
    if algorithm in _METRIC_LEARN:
        raise KeyError("metric %r is a thin import of the metric_learn library in the reference; only 'euclidean' and 'kissme' are built here"
                       % (algorithm,))
    raise KeyError("Unknown metric:", algorithm)
