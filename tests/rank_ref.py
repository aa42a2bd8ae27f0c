"""Exact, definitional reference of the retrieval metrics (reid/evaluation_metrics/ranking.py cmc and mean_ap, the deterministic
protocols), written for this project, and the grid of cases the ranking tests run (tests/test_rank_ref_host.py on the CPU against
oracle/eval_oracle.py and the reference's recorded outputs, tests/test_gpu_rank_metrics.py on the device against this file).

It shares nothing with oracle/eval_oracle.py: no argsort and no restatement of sklearn's array operations.  Per query the valid
gallery entries (different identity or different camera; `separate_camera_set`: different camera only) become (distance, index)
pairs, -0.0 normalised to 0.0, sorted by Python's tuple order.  From that list:
  first_rank   position of the first true match
  nm_before[s] valid non-matches ordered before the s-th match (the bin the all-shots CMC credits: its position minus s)
  nmatch       valid true matches P
  AP           sum over the distinct match distances t of (recall step) x precision, with matches and valid entries counted by
               `<= t` (equal distances form one threshold), as an exact fractions.Fraction, rounded to float64 once.
Infinities are ordered values like any other.  A NaN has no place in the order: a query with a valid true match and a NaN in a
valid entry raises ValueError (a NaN in a filtered entry is never looked at; a query without a valid true match is skipped first,
as in the reference).

AP bound.  The kernel and both references sum at most P non-zero terms, each carrying a few float64 roundings of values <= 1, so
against the exact rational value |AP - exact| <= P * 2^-51 + 2^-52 (ap_bound); for P <= 2048 that is below 1e-12."""
import bisect
from fractions import Fraction

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
DENORM = float(np.float32(2.0 ** -149))           # the smallest float32 denormal
RK_CAP = 2048                                     # matches of one query the kernel holds


def ap_bound(P):
    return P * 2.0 ** -51 + 2.0 ** -52


class Result(object):
    """first [m] int64 (-1: no valid true match), nmatch [m] int64, bins: list of m int64 arrays (nm_before), ap_exact: list of m
    Fractions (None likewise), ap [m] float64 (NaN likewise)"""

    def __init__(self, first, nmatch, bins, ap_exact):
        self.first = np.asarray(first, np.int64); self.nmatch = np.asarray(nmatch, np.int64)
        self.bins = bins; self.ap_exact = ap_exact
        self.ap = np.array([np.nan if a is None else float(a) for a in ap_exact], np.float64)


def _lists(m, n, query_ids, gallery_ids, query_cams, gallery_cams):
    """the reference's defaults (ranking.py:26-33), everything as lists of Python ints (no width to wrap at)"""
    aslist = lambda x, default: [int(v) for v in (default if x is None else np.asarray(x).reshape(-1).tolist())]      # noqa: E731
    return (aslist(query_ids, range(m)), aslist(gallery_ids, range(n)), aslist(query_cams, [0] * m), aslist(gallery_cams, [1] * n))


def per_query(distmat, query_ids=None, gallery_ids=None, query_cams=None, gallery_cams=None, separate_camera_set=False):
    dist = np.asarray(distmat)
    m, n = dist.shape
    qid, gid, qcam, gcam = _lists(m, n, query_ids, gallery_ids, query_cams, gallery_cams)
    assert len(qid) == m and len(qcam) == m and len(gid) == n and len(gcam) == n
    first, nmatch, bins, aps = [], [], [], []
    for q in range(m):
        row = (dist[q].astype(np.float64) + 0.0).tolist()                    # x + 0.0: -0.0 -> 0.0, every other value unchanged
        valid = [j for j in range(n) if (gcam[j] != qcam[q] if separate_camera_set else (gid[j] != qid[q] or gcam[j] != qcam[q]))]
        P = sum(1 for j in valid if gid[j] == qid[q])
        if P == 0:                                                           # the reference skips the query (ranking.py:51,110)
            first.append(-1); nmatch.append(0); bins.append(np.zeros(0, np.int64)); aps.append(None)
            continue
        if any(row[j] != row[j] for j in valid):
            raise ValueError("query %d: NaN distance in a valid gallery entry" % q)
        order = sorted((row[j], j) for j in valid)
        pos = [k for k, (_, j) in enumerate(order) if gid[j] == qid[q]]
        all_d = [d for d, _ in order]
        match_d = [all_d[k] for k in pos]
        ap, prev = Fraction(0), 0
        for t in sorted(set(match_d)):
            tp = bisect.bisect_right(match_d, t)                             # matches with distance <= t
            ap += Fraction(tp - prev, P) * Fraction(tp, bisect.bisect_right(all_d, t))
            prev = tp
        first.append(pos[0]); nmatch.append(P); bins.append(np.array([k - s for s, k in enumerate(pos)], np.int64)); aps.append(ap)
    return Result(first, nmatch, bins, aps)


def cmc(distmat, query_ids=None, gallery_ids=None, query_cams=None, gallery_cams=None, topk=100, separate_camera_set=False,
        first_match_break=False, result=None):
    """the reference's accumulation (ranking.py:62-79) over the bins: first_match_break credits the first match's bin with 1,
    all-shots every bin with 1/len, in order, stopping at the first bin >= topk; cumulative sums over the valid queries.
    `result`: a per_query() result of the same arguments, to save computing it again."""
    r = result if result is not None else per_query(distmat, query_ids, gallery_ids, query_cams, gallery_cams, separate_camera_set)
    ret = np.zeros(topk)
    queries = 0
    for b in r.bins:
        if len(b) == 0:
            continue
        queries += 1
        delta = 1. / len(b)
        for k in b:
            if k >= topk:
                break
            if first_match_break:
                ret[k] += 1
                break
            ret[k] += delta
    if queries == 0:
        raise RuntimeError("No valid query")
    return ret.cumsum() / queries


def mean_ap_exact(result):
    """-> (exact mean of the valid queries' APs as a Fraction, the largest match count among them)"""
    aps = [a for a in result.ap_exact if a is not None]
    if not aps:
        raise RuntimeError("No valid query")
    return sum(aps, Fraction(0)) / len(aps), int(result.nmatch.max())


# ------------------------------------------------------------------ the grid
def _case(dist, qid, gid, qcam, gcam, family, finite=True):
    arr = lambda x: None if x is None else np.asarray(x)          # noqa: E731
    return dict(dist=np.ascontiguousarray(dist, dtype=np.float32), qid=arr(qid), gid=arr(gid), qcam=arr(qcam), gcam=arr(gcam),
                family=family, finite=finite)


def args(case):
    return case["dist"], case["qid"], case["gid"], case["qcam"], case["gcam"]


def _coarse(rng, shape, levels):
    """float32 distances on a grid of `levels` values: many exact ties, a match among non-matches of the same value"""
    return (rng.integers(0, levels, shape) / 8.0).astype(np.float32)


def match_count_case(P, extra=300, seed=0):
    """query 0 (identity 7, camera 0) has exactly P valid true matches among n = P + extra gallery entries; around them same-identity
    same-camera entries (filtered), the junk pid -1, and other identities on every camera.  Query 1 is an ordinary query with a few
    matches, query 2's identity is absent from the gallery."""
    rng = np.random.default_rng(1000 + P + seed)
    n = P + extra
    gid = rng.integers(20, 40, n); gcam = rng.integers(0, 4, n)
    slots = rng.permutation(n)
    gid[slots[:P]] = 7; gcam[slots[:P]] = rng.integers(1, 4, P)                       # the P valid matches
    gid[slots[P:P + 12]] = 7; gcam[slots[P:P + 12]] = 0                               # same identity, same camera: filtered
    gid[slots[P + 12:P + 30]] = -1                                                    # junk
    gid[slots[P + 30:P + 37]] = 3; gcam[slots[P + 30:P + 37]] = [0, 1, 1, 2, 2, 3, 0]  # query 1's: 5 valid, 2 filtered
    return _case(_coarse(rng, (3, n), n), [7, 3, 999], gid, [0, 0, 2], gcam, "match_count")


def gallery_size_case(n, m, where="last"):
    """query 0's only match is the last gallery column (`where` = "first": column 0); with m = 3, query 1's only match is column 0
    and query 2 has whatever the random identities give it"""
    rng = np.random.default_rng(2000 + 7 * n + m + (where == "first"))
    gid = rng.integers(20, 24, n); gcam = rng.integers(0, 3, n)
    qid, qcam = [7, 8, 21][:m], [0, 0, 1][:m]
    gid[0] = 8; gcam[0] = 1
    col = n - 1 if where == "last" else 0
    gid[col] = 7; gcam[col] = 2
    return _case(_coarse(rng, (m, n), max(2, n // 2)), qid, gid, qcam, gcam, "gallery_size")


def _tie_ids(rng, m, n):
    """few identities on few cameras: every query has dozens of matches, filtered entries and non-matches on every side"""
    return rng.integers(0, 5, m), rng.integers(0, 5, n), rng.integers(0, 3, m), rng.integers(0, 3, n)


def tie_case(kind):
    rng = np.random.default_rng(3000 + sum(map(ord, kind)))
    m, n = 4, 600
    qid, gid, qcam, gcam = _tie_ids(rng, m, n)
    finite = True
    if kind == "constant":
        dist = np.full((m, n), 0.625, np.float32)
    elif kind == "three_values":
        dist = rng.choice(np.array([0.25, 0.5, 2.0], np.float32), (m, n))
    elif kind == "stride":
        # a match at column j with equal non-matches at j-256, j-1, j+1, j+256 (the kernel's threads walk the row with stride 256);
        # everything else distinct, half of it below the tied value
        dist = rng.permutation(m * n).reshape(m, n).astype(np.float32)
        for q, j in enumerate((256, 290, 317, 343)):
            qid[q] = 50 + q; qcam[q] = 0
            gid[j] = 50 + q; gcam[j] = 1
            for k in (j - 256, j - 1, j + 1, j + 256):
                gid[k] = 60 + q
            dist[q, [j - 256, j - 1, j, j + 1, j + 256]] = m * n / 2 + 0.5
    elif kind == "signed_zero":
        dist = rng.choice(np.array([0.0, -0.0, DENORM, -DENORM], np.float32), (m, n), p=[0.4, 0.4, 0.1, 0.1])
    elif kind == "plus_inf":
        dist = rng.choice(np.array([1.0, 3.0, np.inf], np.float32), (m, n), p=[0.3, 0.3, 0.4]); finite = False
        dist[3] = np.inf
    elif kind == "minus_inf":
        dist = rng.choice(np.array([-np.inf, -2.0, 5.0, np.inf], np.float32), (m, n)); finite = False
    elif kind == "denormal":
        dist = (rng.integers(-3, 6, (m, n)) * DENORM).astype(np.float32)
    elif kind == "flt_max":
        below = float(np.nextafter(np.float32(FLT_MAX), np.float32(0)))
        dist = rng.choice(np.array([FLT_MAX, below, -FLT_MAX, 0.0], np.float32), (m, n))
    else:
        raise KeyError(kind)
    return _case(dist, qid, gid, qcam, gcam, "ties", finite)


TIE_KINDS = ("constant", "three_values", "stride", "signed_zero", "plus_inf", "minus_inf", "denormal", "flt_max")


def validity_case(kind):
    rng = np.random.default_rng(4000 + sum(map(ord, kind)))
    if kind == "mixed":
        # queries 0, 3, 5 are ordinary; 1: identity absent; 2: identity present on the query's camera only; 4: the junk pid as a query
        n = 120
        gid = rng.integers(0, 6, n); gcam = rng.integers(0, 3, n)
        gid[rng.permutation(n)[:15]] = -1
        gcam[gid == 4] = 2
        return _case(_coarse(rng, (6, n), 40), [0, 77, 4, 1, -1, 2], gid, [0, 1, 2, 1, 0, 2], gcam, "validity")
    if kind == "int32_edges":
        names = np.array([2 ** 31 - 1, -2 ** 31, 2 ** 31 - 2, -2 ** 31 + 1, 0, -1], np.int64)
        n = 90
        gid = names[rng.integers(0, 6, n)]; gcam = rng.integers(0, 3, n)
        return _case(_coarse(rng, (6, n), 30), names, gid, [0, 1, 2, 0, 1, 2], gcam, "validity")
    if kind == "id_wrap":
        # identities that a cast to int32 would merge: 5 and 5 + 2^32; 2^31 and -2^31; -1 (junk) and 2^32 - 1
        names = np.array([5, 5 + 2 ** 32, 2 ** 31, -2 ** 31, -1, 2 ** 32 - 1, 5 - 2 ** 32], np.int64)
        n = 140
        gid = names[rng.integers(0, 7, n)]; gcam = rng.integers(0, 3, n)
        return _case(_coarse(rng, (7, n), 50), names, gid, [0, 1, 2, 0, 1, 2, 0], gcam, "validity")
    if kind == "defaults":
        # None everywhere: query i is identity i on camera 0, gallery entry j identity j on camera 1
        return _case(_coarse(rng, (5, 40), 12), None, None, None, None, "validity")
    if kind == "separate_cameras":
        # query 0 (identity 1, camera 0): same identity same camera (dropped either way), different identity same camera (dropped
        # by separate_camera_set only), matches on other cameras
        gid = [1, 1, 2, 2, 1, 3, 1, 2, 3, 3, 1, 2]
        gcam = [0, 1, 0, 1, 2, 0, 0, 2, 1, 0, 1, 0]
        dist = np.array([[3, 4, 1, 2, 6, 1, 0, 5, 4, 2, 4, 0], [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]], np.float32)
        return _case(dist, [1, 2], gid, [0, 1], gcam, "validity")
    if kind == "all_invalid":
        # no query has a valid true match: absent identity; identity on the query's own camera only
        return _case(_coarse(rng, (2, 30), 10), [50, 1], [1] * 10 + [2] * 20, [0, 0], [0] * 10 + [1] * 20, "validity")
    raise KeyError(kind)


VALIDITY_KINDS = ("mixed", "int32_edges", "id_wrap", "defaults", "separate_cameras")       # "all_invalid" raises: tested on its own
MATCH_COUNTS = (1, 2, 255, 256, 257, 1023, 2047, 2048)
GALLERY_SIZES = (1, 2, 255, 256, 257, 513)


def grid():
    """name -> builder of every case both test files run (built on demand: the large ones take a moment)"""
    g = {}
    for P in MATCH_COUNTS:
        g["count_%d" % P] = (lambda P=P: match_count_case(P))
    for n in GALLERY_SIZES:
        g["size_%d_m1_last" % n] = (lambda n=n: gallery_size_case(n, 1, "last"))
        g["size_%d_m1_first" % n] = (lambda n=n: gallery_size_case(n, 1, "first"))
        g["size_%d_m3" % n] = (lambda n=n: gallery_size_case(n, 3))
    for k in TIE_KINDS:
        g["tie_" + k] = (lambda k=k: tie_case(k))
    for k in VALIDITY_KINDS:
        g["valid_" + k] = (lambda k=k: validity_case(k))
    return g


GRID = grid()


def tied_both_sides(case, separate_camera_set=False):
    """does some query have a true match whose distance equals that of valid non-matches at a lower AND at a higher gallery index?"""
    dist = case["dist"]
    m, n = dist.shape
    qid, gid, qcam, gcam = _lists(m, n, case["qid"], case["gid"], case["qcam"], case["gcam"])
    for q in range(m):
        valid = [j for j in range(n) if (gcam[j] != qcam[q] if separate_camera_set else (gid[j] != qid[q] or gcam[j] != qcam[q]))]
        for j in valid:
            if gid[j] != qid[q]:
                continue
            same = [k for k in valid if gid[k] != qid[q] and dist[q, k] == dist[q, j]]
            if same and same[0] < j < same[-1]:
                return True
    return False
