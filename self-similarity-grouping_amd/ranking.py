"""Retrieval metrics -- host-side mirror of reid/evaluation_metrics/ranking.py:18-115 (cmc, mean_ap) and
reid/evaluators.py:88-129 (evaluate_all), :147-166 (Evaluator), computed on the GPU (csrc/ranking.hip).

`cmc(...)`, `mean_ap(...)` and `evaluate_all(...)` keep the reference signatures and return types (numpy
cumulative-match curve, float mAP, CMC top-1).  The distance block may be a numpy array, a CPU tensor or a CUDA
tensor (the Evaluator keeps it on the device).  Protocols: the deterministic ones -- 'market1501'
(`first_match_break=True`, what evaluate_all uses) and 'allshots' (every match credited with 1/len), each optionally with
`separate_camera_set` -- and the `single_gallery_shot` protocol ('cuhk03': ten random one-entry-per-identity gallery subsets per
query, ranking.py:11-16,56-61; commented out in the reference's evaluate_all).  That one draws from a numpy stream, so it takes the
stream as `rng=` (np.random for the global legacy stream, a RandomState, or an int seed; None raises NotImplementedError): the host reads
the stream's 32-bit MT19937 words from a copy of its state, csrc/cmc_sgs.hip replays np.random.choice's masked-rejection rule on them
in the reference's query -> repeat -> identity order, and the stream is left exactly where the reference's loop leaves it (curve and
following draws bit for bit: tests/test_gpu_cmc_sgs.py).  `single_shot_ranks` returns the raw bins, `evaluate_all(cmc_protocols=...)`
prints the reference's three-column table.  Limits, refused with ValueError: 131 072 gallery entries, 16 384 gallery identities, 16 384
entries of one identity.  Measured (profiles/cmc_sgs_times.txt): 0.38 s at 1 400 x 5 332 / 700 identities where the reference's loop
takes 71 s on a CPU core, 1.56 s at 3 368 x 15 913 / 751 identities; the draw stage is serial by nature (one wave) and takes 85-89 % of
the call.

Equal distances are ordered by gallery index (numpy's default argsort leaves the tie order unspecified); mAP
does not depend on it, and CMC only when a true match ties with a non-match.  No CPU fallback.

Distances are ordered values: -0.0 equals 0.0, and denormals, FLT_MAX and +-inf are accepted and take their place in the order like any
other number (the reference's CMC accepts them too; tests/rank_ref.py defines the result).  NaN is not: a NaN distance in a valid gallery
entry of a query that has a valid true match raises RankNaNError (sklearn's average_precision_score refuses such scores; the kernel
would otherwise rank it nowhere), while a NaN in an entry the id / camera filter removes is never read.  Ids and cameras are only ever
compared for equality: values outside int32 are replaced by their dense ranks, never truncated.
"""
import contextlib
import ctypes
import os
import time

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream


def _dev():
    if not torch.cuda.is_available():
        raise _lib.SSGError("ssg_amd.ranking runs on the GPU only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


class RankNaNError(_lib.SSGError):
    """A NaN distance in a valid gallery entry of a query that has a valid true match: the entry has no place in the ranking, and the
    reference's mean_ap does not return a number either (sklearn refuses non-finite scores).  Raised instead of a plausible-looking
    metric; the message names the first such query."""


def _int32_labels(query, gallery):
    """Query and gallery labels (identities, or cameras) -> two int32 numpy arrays that are equal exactly where the given labels are.
    Equality is all the metrics use, so labels outside int32 are replaced, query and gallery together, by their dense ranks; a cast
    would make two identities that differ by a multiple of 2^32 one."""
    query, gallery = np.asarray(query).reshape(-1).astype(np.int64), np.asarray(gallery).reshape(-1).astype(np.int64)
    both = np.concatenate([query, gallery])
    if both.size and (both.min() < -2 ** 31 or both.max() >= 2 ** 31):
        both = np.unique(both, return_inverse=True)[1].reshape(-1)
    both = both.astype(np.int32)
    return both[:query.size], both[query.size:]


def _prepare(distmat, query_ids, gallery_ids, query_cams, gallery_cams):
    """what both entry points take -> (float32 CUDA block with unit column stride, its row pitch ld >= n, m, n, qid, qcam, gid, gcam
    as int32 CUDA tensors); the reference's defaults for lists that are None (ranking.py:26-33)"""
    dev = _dev()
    d = torch.as_tensor(distmat).to(dev, torch.float32)
    if d.dim() != 2:
        raise ValueError("distmat must be [m, n]")
    m, n = d.shape
    if d.stride(1) != 1 or (m > 1 and d.stride(0) < n):          # a transposed or a broadcast block: the kernel reads rows of pitch ld
        d = d.contiguous()
    ld = d.stride(0) if m > 1 else n                             # (a single row has no pitch: torch reports any stride for it)
    qid, gid = _int32_labels(np.arange(m) if query_ids is None else query_ids, np.arange(n) if gallery_ids is None else gallery_ids)
    qcam, gcam = _int32_labels(np.zeros(m) if query_cams is None else query_cams, np.ones(n) if gallery_cams is None else gallery_cams)
    if qid.size != m or qcam.size != m or gid.size != n or gcam.size != n:
        raise ValueError("id / camera lists do not match the distance block")
    return (d, ld, m, n) + tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (qid, qcam, gid, gcam))


def _raise_unevaluated(first):
    """the kernel left queries unevaluated (its *overflow word is non-zero): -2 marks a NaN distance, else it is the match cap"""
    nan = torch.nonzero(first == -2)
    if nan.numel():
        raise RankNaNError("ssg_rank_metrics: query %d has a NaN distance in a valid gallery entry" % int(nan[0]))
    raise _lib.SSGError("ssg_rank_metrics: a query has more than 2048 true matches in the gallery")


def per_query(distmat, query_ids=None, gallery_ids=None, query_cams=None, gallery_cams=None, separate_camera_set=False):
    """-> (first_rank int32[m] CUDA, ap float64[m] CUDA); -1 / NaN mark queries without a valid true match."""
    L = _lib.lib()
    d, ld, m, n, qid, qcam, gid, gcam = _prepare(distmat, query_ids, gallery_ids, query_cams, gallery_cams)
    first = torch.empty(m, dtype=torch.int32, device=d.device); ap = torch.empty(m, dtype=torch.float64, device=d.device)
    ovf = torch.zeros(1, dtype=torch.int32, device=d.device)
    check(L.ssg_rank_metrics(ptr(d), m, n, ld, ptr(qid), ptr(qcam), ptr(gid), ptr(gcam), 1 if separate_camera_set else 0,
                             ptr(first), ptr(ap), ptr(ovf), stream()), "ssg_rank_metrics")
    if int(ovf.item()):
        _raise_unevaluated(first)
    return first, ap


def per_query_all(distmat, query_ids=None, gallery_ids=None, query_cams=None, gallery_cams=None, separate_camera_set=False):
    """-> (nmatch int32[m], nm_before int32[m, cap]) numpy: per query the number of valid true matches and, for its s-th match,
    the number of valid non-matching gallery entries ordered before it (the bins the all-shots CMC credits)."""
    L = _lib.lib()
    d, ld, m, n, qid, qcam, gid, gcam = _prepare(distmat, query_ids, gallery_ids, query_cams, gallery_cams)
    dev = d.device
    cap = int(min(2048, max(1, int(torch.unique(gid, return_counts=True)[1].max().item())))) if n else 1      # no query can have more matches than the largest
    # gallery identity (unique counts, not bincount: raw Market-1501 lists carry the junk pid -1, ids may be large and sparse)
    first = torch.empty(m, dtype=torch.int32, device=dev); ap = torch.empty(m, dtype=torch.float64, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    nmb = torch.zeros((m, cap), dtype=torch.int32, device=dev); nm = torch.zeros(m, dtype=torch.int32, device=dev)
    check(L.ssg_rank_metrics_all(ptr(d), m, n, ld, ptr(qid), ptr(qcam), ptr(gid), ptr(gcam), 1 if separate_camera_set else 0,
                                 ptr(first), ptr(ap), ptr(ovf), ptr(nmb), ptr(nm), cap, stream()), "ssg_rank_metrics_all")
    if int(ovf.item()):
        _raise_unevaluated(first)
    return nm.cpu().numpy(), nmb.cpu().numpy()


# ------------------------------------------------------------------ the single-gallery-shot protocol ('cuhk03', csrc/cmc_sgs.hip)
SGS_MAX_N, SGS_MAX_G, SGS_MAX_GROUP, SGS_REPEAT = 131072, 16384, 16384, 10
_SGS_WORKSPACE = 256 << 20          # bytes of device workspace: the queries are processed in chunks that fit


class _LegacyStream(object):
    """The 32-bit words of a legacy MT19937 stream (np.random itself or a RandomState), read from a copy of its state; `commit(c)`
    leaves the stream where the reference's loop leaves it after c words (the cached Gaussian untouched)."""

    def __init__(self, rng):
        if rng is None:
            raise NotImplementedError("single_gallery_shot draws its gallery subsets from a numpy stream (ranking.py:11-16,56-61): pass rng=np.random "
                                      "to consume the global legacy stream like the reference, a np.random.RandomState, or an int seed")
        if rng is np.random:
            self._get, self._set = (lambda: np.random.get_state(legacy=False)), np.random.set_state
        elif isinstance(rng, np.random.RandomState):
            self._get, self._set = (lambda: rng.get_state(legacy=False)), rng.set_state
        elif isinstance(rng, (int, np.integer)) and not isinstance(rng, (bool, np.bool_)):
            own = np.random.RandomState(int(rng))
            self._get, self._set = (lambda: own.get_state(legacy=False)), own.set_state
        else:
            raise TypeError("rng must be np.random, a np.random.RandomState or an int seed, not %s (np.random.Generator streams are not "
                            "what the reference consumes)" % type(rng).__name__)
        self.start = self._get()
        if self.start["bit_generator"] != "MT19937":
            raise TypeError("rng must be a RandomState over MT19937 (the legacy stream), not over %s" % self.start["bit_generator"])
        self._front = self._copy()          # draws the words
        self._back = self._copy()           # follows the consumed count
        self._back_at = 0
        self._base = 0                      # stream position of _buf[0]
        self._buf = np.zeros(0, np.uint32)

    def _copy(self):
        bg = np.random.MT19937()
        bg.state = {"bit_generator": "MT19937", "state": dict(self.start["state"])}
        return bg

    def _advance(self, cursor):
        while self._back_at < cursor:
            step = int(min(cursor - self._back_at, 1 << 22))
            self._back.random_raw(step, output=False)
            self._back_at += step

    def words(self, cursor, need):
        """-> uint32 array of the words from `cursor` on, at least `need` of them"""
        self._buf = self._buf[cursor - self._base:]
        self._base = cursor
        if len(self._buf) < need:
            self._buf = np.concatenate([self._buf, self._front.random_raw(int(need - len(self._buf))).astype(np.uint32)])
        return self._buf

    def commit(self, cursor):
        self._advance(cursor)
        st = dict(self._back.state)
        st["has_gauss"] = self.start["has_gauss"]; st["gauss"] = self.start["gauss"]
        self._set(st)


def _sgs_host_checks(distmat, query_ids, gallery_ids, query_cams, gallery_cams):
    """everything that is decided before the device is touched -> (m, n, numpy id / camera lists as int32, gden, qden, G, group sizes)"""
    shape = tuple(distmat.shape) if hasattr(distmat, "shape") else np.asarray(distmat).shape
    if len(shape) != 2:
        raise ValueError("distmat must be [m, n]")
    m, n = int(shape[0]), int(shape[1])

    qid, gid = _int32_labels(np.arange(m) if query_ids is None else query_ids, np.arange(n) if gallery_ids is None else gallery_ids)
    qcam, gcam = _int32_labels(np.zeros(m) if query_cams is None else query_cams, np.ones(n) if gallery_cams is None else gallery_cams)
    if qid.size != m or qcam.size != m or gid.size != n or gcam.size != n or m == 0 or n == 0:
        raise ValueError("id / camera lists do not match the distance block")
    if n > SGS_MAX_N:
        raise ValueError("single_gallery_shot: n = %d gallery entries, at most %d" % (n, SGS_MAX_N))
    names, gden, sizes = np.unique(gid, return_inverse=True, return_counts=True)
    G = int(names.size)
    if G > SGS_MAX_G:
        raise ValueError("single_gallery_shot: G = %d gallery identities, at most %d" % (G, SGS_MAX_G))
    if int(sizes.max()) > SGS_MAX_GROUP:
        raise ValueError("single_gallery_shot: the largest gallery identity has %d entries, at most %d" % (int(sizes.max()), SGS_MAX_GROUP))
    pos = np.minimum(np.searchsorted(names, qid), G - 1)
    qden = np.where(names[pos] == qid, pos, -1).astype(np.int32)
    return m, n, qid, gid, qcam, gcam, gden.reshape(-1).astype(np.int32), qden, G, sizes


def single_shot_ranks(distmat, query_ids=None, gallery_ids=None, query_cams=None, gallery_cams=None, separate_camera_set=False, rng=None):
    """The raw draws of the single-gallery-shot protocol -> int32 [m, 10] CUDA tensor: per (query, repeat) the number of other identities
    whose drawn gallery entry is ordered before the drawn true match (the bin ranking.py:66-75 credits); -1 rows mark queries without a
    valid true match.  `rng` as for cmc(); the stream is advanced by exactly the words the reference's loop consumes."""
    words = _LegacyStream(rng)
    m, n, qid, gid, qcam, gcam, gden, qden, G, sizes = _sgs_host_checks(distmat, query_ids, gallery_ids, query_cams, gallery_cams)
    L = _lib.lib()
    dev = _dev()
    d = torch.as_tensor(distmat).to(dev, torch.float32)
    if d.stride(1) != 1:
        d = d.contiguous()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)           # noqa: E731
    tq, tqc, tqd, tg, tgc, tgd = up(qid), up(qcam), up(qden), up(gid), up(gcam), up(gden)
    # development knobs, read per call: the size of every uploaded word block, the queries per chunk
    forced = int(os.environ.get("SSG_CMC_SGS_WORDS", "0") or 0)
    chunk = int(os.environ.get("SSG_CMC_SGS_CHUNK", "0") or 0)
    if chunk <= 0:
        chunk = max(1, _SGS_WORKSPACE // int(L.ssg_cmc_sgs_workspace_bytes(1, n, G)))
    chunk = min(chunk, m)
    ws_bytes = int(L.ssg_cmc_sgs_workspace_bytes(chunk, n, G))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    # words one query is expected to consume: a group of s > 1 entries accepts a word with probability s / 2^bit_length(s - 1)
    s = sizes[sizes > 1].astype(np.int64)
    per_query = SGS_REPEAT * float(np.sum(2.0 ** np.ceil(np.log2(s)) / s)) if s.size else 0.0
    k = torch.empty((m, SGS_REPEAT), dtype=torch.int32, device=dev)
    state = torch.zeros(4, dtype=torch.int64, device=dev)
    cursor = 0
    for q0 in range(0, m, chunk):
        mq = min(chunk, m - q0)
        with _stage("groups"):
            check(L.ssg_cmc_sgs_groups(_at(d, q0 * d.stride(0)), mq, n, d.stride(0), _at(tq, q0), _at(tqc, q0), _at(tqd, q0), ptr(tg), ptr(tgc), ptr(tgd),
                                       G, 1 if separate_camera_set else 0, ptr(ws), ws_bytes, stream()), "ssg_cmc_sgs_groups")
        state[1:] = 0
        left = mq
        while True:
            with _stage("words"):
                block = forced if forced > 0 else int(left * per_query * 1.02) + 1024
                buf = words.words(cursor, block)
                if forced > 0:
                    buf = buf[:forced]
                wdev = torch.from_numpy(buf.view(np.int32)).to(dev)
            with _stage("draws"):
                check(L.ssg_cmc_sgs_draws(ptr(ws), ws_bytes, mq, n, G, ptr(wdev), cursor, int(buf.size), ptr(state), stream()), "ssg_cmc_sgs_draws")
                st = state.cpu().numpy()                 # (waits for the launch: wdev stays alive until here)
            cursor = int(st[0])
            if not int(st[3]):
                break
            left = mq - int(st[1])                       # the words ran out: top up and resume where the kernel stopped
        with _stage("counts"):
            check(L.ssg_cmc_sgs_counts(ptr(ws), ws_bytes, mq, n, G, _at(k, q0 * SGS_REPEAT), stream()), "ssg_cmc_sgs_counts")
    torch.cuda.current_stream().synchronize()
    with _stage("commit"):
        words.commit(cursor)
    single_shot_ranks.last_consumed = cursor             # the words the call took from the stream (read by the tests and the timing tool)
    return k


single_shot_ranks.stage_times = None          # a dict here (tools/time_cmc_sgs.py) collects seconds per stage, at the price of a device
#                                               synchronise around each


@contextlib.contextmanager
def _stage(name):
    acc = single_shot_ranks.stage_times
    if acc is None:
        yield
        return
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    acc[name] = acc.get(name, 0.0) + time.perf_counter() - t0


def _at(t, offset):
    """device pointer of element `offset` of a tensor"""
    return ctypes.c_void_p(t.data_ptr() + int(offset) * t.element_size())


def cmc(distmat, query_ids=None, gallery_ids=None, query_cams=None, gallery_cams=None, topk=100,
        separate_camera_set=False, single_gallery_shot=False, first_match_break=False, rng=None):
    """ranking.py:18-79.  `rng` is read by the single_gallery_shot protocol only: np.random replays and advances the global legacy stream
    exactly like the reference's loop, a np.random.RandomState does the same on that instance, an int seeds a fresh RandomState (the global
    stream stays untouched); None raises NotImplementedError (nothing here consumes the global stream unasked)."""
    if single_gallery_shot:
        k = single_shot_ranks(distmat, query_ids, gallery_ids, query_cams, gallery_cams, separate_camera_set, rng=rng).cpu().numpy()
        valid = k[:, 0] >= 0
        if not valid.any():
            raise RuntimeError("No valid query")
        ret = np.zeros(topk)
        bins = k[valid].reshape(-1)                      # (query, repeat) order: the reference's float64 adds in the reference's order (ranking.py:62-75)
        np.add.at(ret, bins[bins < topk], 1 if first_match_break else 1. / SGS_REPEAT)
        return ret.cumsum() / int(valid.sum())
    if not first_match_break:
        nm, nmb = per_query_all(distmat, query_ids, gallery_ids, query_cams, gallery_cams, separate_camera_set)
        valid = nm > 0
        if not valid.any():
            raise RuntimeError("No valid query")
        ret = np.zeros(topk)
        for q in np.nonzero(valid)[0]:           # sequential adds in query / rank order, like the reference loop (ranking.py:68-75)
            bins = nmb[q, :nm[q]]
            bins = bins[: int(np.searchsorted(bins, topk, side="left"))]
            np.add.at(ret, bins, 1. / nm[q])
        return ret.cumsum() / int(valid.sum())
    first, _ = per_query(distmat, query_ids, gallery_ids, query_cams, gallery_cams, separate_camera_set)
    first = first.cpu().numpy()
    valid = first >= 0
    if not valid.any():
        raise RuntimeError("No valid query")
    ret = np.zeros(topk)
    hit = first[valid & (first < topk)]
    np.add.at(ret, hit, 1)
    return ret.cumsum() / int(valid.sum())


def mean_ap(distmat, query_ids=None, gallery_ids=None, query_cams=None, gallery_cams=None):
    """ranking.py:82-115."""
    _, ap = per_query(distmat, query_ids, gallery_ids, query_cams, gallery_cams)
    ap = ap.cpu().numpy()
    aps = ap[~np.isnan(ap)]
    if aps.size == 0:
        raise RuntimeError("No valid query")
    return np.mean(aps)


def evaluate_all(distmat, query=None, gallery=None, query_ids=None, gallery_ids=None, query_cams=None, gallery_cams=None,
                 cmc_topk=(1, 5, 10), cmc_protocols=None, rng=None):
    """reid/evaluators.py:88-129: prints mAP and the market1501 CMC scores, returns CMC top-1.  With `cmc_protocols`, a tuple out of
    ('allshots', 'cuhk03', 'market1501'), it prints the score table the reference keeps commented out (:120-126) for the listed protocols
    (computed, and set in columns, in that order; only 'cuhk03' reads `rng`, see cmc()) and returns the market1501 top-1 when that protocol
    is listed, else the top-1 of the first one listed."""
    if query is not None and gallery is not None:
        query_ids = [pid for _, pid, _ in query]; gallery_ids = [pid for _, pid, _ in gallery]
        query_cams = [cam for _, _, cam in query]; gallery_cams = [cam for _, _, cam in gallery]
    else:
        assert (query_ids is not None and gallery_ids is not None and query_cams is not None and gallery_cams is not None)
    if cmc_protocols is not None:
        return _evaluate_protocols(distmat, query_ids, gallery_ids, query_cams, gallery_cams, cmc_topk, tuple(cmc_protocols), rng)
    first, ap = per_query(distmat, query_ids, gallery_ids, query_cams, gallery_cams)     # one device pass serves both metrics
    first = first.cpu().numpy(); ap = ap.cpu().numpy()
    valid = first >= 0
    if not valid.any():
        raise RuntimeError("No valid query")
    mAP = np.mean(ap[valid])
    print('Mean AP: {:4.1%}'.format(mAP))
    ret = np.zeros(100)
    np.add.at(ret, first[valid & (first < 100)], 1)
    scores = ret.cumsum() / int(valid.sum())
    print('CMC Scores{:>12}'.format('market1501'))
    for k in cmc_topk:
        print('top-{:<4}{:12.1%}'.format(k, scores[k - 1]))
    return scores[0]


CMC_CONFIGS = {     # reid/evaluators.py:106-115
    'allshots': dict(separate_camera_set=False, single_gallery_shot=False, first_match_break=False),
    'cuhk03': dict(separate_camera_set=True, single_gallery_shot=True, first_match_break=False),
    'market1501': dict(separate_camera_set=False, single_gallery_shot=False, first_match_break=True)}


def _evaluate_protocols(distmat, query_ids, gallery_ids, query_cams, gallery_cams, cmc_topk, protocols, rng):
    unknown = [p for p in protocols if p not in CMC_CONFIGS]
    if unknown or not protocols:
        raise ValueError("cmc_protocols must name some of %s, got %r" % (tuple(CMC_CONFIGS), protocols))
    if 'cuhk03' in protocols:
        _LegacyStream(rng)                                 # refuse a missing / unusable stream before anything is printed
    distmat = torch.as_tensor(distmat).to(_dev(), torch.float32)           # one upload serves every protocol
    mAP = mean_ap(distmat, query_ids, gallery_ids, query_cams, gallery_cams)
    print('Mean AP: {:4.1%}'.format(mAP))
    names = [p for p in CMC_CONFIGS if p in protocols]
    cmc_scores = {name: cmc(distmat, query_ids, gallery_ids, query_cams, gallery_cams, rng=rng if name == 'cuhk03' else None, **CMC_CONFIGS[name])
                  for name in names}
    print('CMC Scores' + ''.join('{:>12}'.format(name) for name in names))
    for k in cmc_topk:
        print('  top-{:<4}'.format(k) + ''.join('{:12.1%}'.format(cmc_scores[name][k - 1]) for name in names))
    return cmc_scores['market1501' if 'market1501' in protocols else protocols[0]][0]


def evaluate_same_cams_all(distmat, query=None, gallery=None, query_ids=None, gallery_ids=None, cmc_topk=(1, 5, 10)):
    """reid/evaluators.py:137-180: evaluate_all with the camera filter switched off (every query on camera 0, every gallery entry on
    camera 1).  The reference's branch that takes the id lists directly leaves the cameras undefined (:145-149, a NameError); the
    same 0 / 1 cameras are used here."""
    if query is not None and gallery is not None:
        query_ids = [pid for _, pid, _ in query]; gallery_ids = [pid for _, pid, _ in gallery]
    else:
        assert (query_ids is not None and gallery_ids is not None)
    return evaluate_all(distmat, query_ids=query_ids, gallery_ids=gallery_ids, query_cams=[0] * len(query_ids),
                        gallery_cams=[1] * len(gallery_ids), cmc_topk=cmc_topk)


class Evaluator(object):
    """reid/evaluators.py:183-207: features -> query x gallery distance block -> metrics, all on the GPU."""

    def __init__(self, model, print_freq=1):
        self.model = model
        self.print_freq = print_freq

    def evaluate(self, data_loader, query, gallery, metric=None):
        from .evaluators import extract_features, pairwise_distance_device
        features, _ = extract_features(self.model, data_loader, print_freq=self.print_freq)
        distmat = pairwise_distance_device(features, query, gallery, metric=metric)
        return evaluate_all(distmat, query=query, gallery=gallery)

    def evaluate_same_cams(self, data_loader, query, gallery, metric=None):
        """reid/evaluators.py:194-207: the verification protocol (ssg_amd.verification.find_metric_threshold), then mAP / CMC without
        the camera filter.  The distance block is computed once and stays on the device for both; as in the reference the
        verification step sees the features without `metric`, so a metric costs a second block."""
        from .evaluators import extract_features, pairwise_distance_device
        from .verification import find_metric_threshold
        features, _ = extract_features(self.model, data_loader)
        query_ids = [pid for _, pid, _ in query]; gallery_ids = [pid for _, pid, _ in gallery]
        distmat = pairwise_distance_device(features, query, gallery, metric=metric)
        plain = distmat if metric is None else pairwise_distance_device(features, query, gallery)
        find_metric_threshold(None, query_ids, None, gallery_ids, dist=plain)
        return evaluate_same_cams_all(distmat, query=query, gallery=gallery)
