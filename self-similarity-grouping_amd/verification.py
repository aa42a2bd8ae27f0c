"""Verification metrics -- host-side mirror of reid/evaluation_metrics/eval_far_gar.py:61-202 (CalClassificationError_MPI,
findMetricThreshold_MPI), computed on the GPU (csrc/verify.hip) from the query x gallery block of squared distances.

`find_metric_threshold(...)` (alias `findMetricThreshold_MPI`) prints the reference's lines -- intra / inter distance statistics, the
pair counts of the ten-threshold classification step (or `The Metric Feature Is Too Bad!`), one `thr / FAR / GAR` line per FAR -- and
returns the values behind them as a `VerificationResult`.  `cal_classification_error(...)` (alias `CalClassificationError_MPI`)
keeps the reference's return value.

What differs from the reference, on purpose:
  * `dist` (numpy array, CPU tensor or CUDA tensor of SQUARED distances) is only read; the reference clamps its caller's array.
  * the sums are float64 (the reference accumulates float32); counts, minima, maxima, order statistics and threshold counts are exact.
  * the per-element FAR / GAR dump that the reference writes to `fid` (one text line per inter pair) is not produced; `fid` receives
    the log lines.  For a curve pass a longer `far` list (at most 64 values per call).
  * a query without an intra or without an inter element, and a NaN in the block, raise ValueError (the reference dies in min() of
    an empty array, or prints NaN).
  * one GPU, one process: there is no MPI and no `group=` argument.
No CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

MAX_PER_CALL = 64
DEFAULT_FAR = (1e-2, 1e-3, 1e-4, 1e-5)


class VerificationResult(object):
    """intra_* / inter_*: num (int), avg, std (float, from float64 sums), min, max (np.float32); thresholds: the ten float64
    thresholds with pos_err_rate / neg_err_rate (None when intra_avg >= inter_avg: `too_bad`); per FAR: far, num, thr (np.float32),
    cnt, GAR; lines: what was printed."""

    def __repr__(self):
        return "VerificationResult(%s)" % ", ".join("%s=%r" % kv for kv in sorted(self.__dict__.items()) if kv[0] != "lines")


def _dev():
    if not torch.cuda.is_available():
        raise _lib.SSGError("ssg_amd.verification runs on the GPU only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _labels(x, what):
    a = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)
    if a.ndim != 1 or a.size == 0:
        raise ValueError("%s: a non-empty 1-d list of labels is needed, got shape %r" % (what, a.shape))
    if a.dtype.kind not in "iub":
        raise ValueError("%s: integer labels are needed, got %s" % (what, a.dtype))
    a = a.astype(np.int64)
    if a.min() < -2 ** 31 or a.max() >= 2 ** 31:
        raise ValueError("%s: labels must fit int32" % what)
    return a.astype(np.int32)


def _rows(feat, what):
    if feat is None:
        return None
    shape = tuple(feat.shape)
    if len(shape) != 2 or shape[0] == 0 or shape[1] == 0:
        raise ValueError("%s: a non-empty [rows, d] feature matrix is needed, got shape %r" % (what, shape))
    return shape[0]


class _Block(object):
    """the block and its labels on the device, plus the workspace of the three passes"""

    def __init__(self, qry_feat, qry_label, ref_feat, ref_label, dist):
        ql = _labels(qry_label, "qry_label"); rl = _labels(ref_label, "ref_label")
        mq, nr = _rows(qry_feat, "qry_feat"), _rows(ref_feat, "ref_feat")
        if dist is None and (mq is None or nr is None):
            raise ValueError("features are needed when dist is not given")
        if dist is not None:
            dshape = tuple(dist.shape)
            if len(dshape) != 2 or dshape[0] == 0 or dshape[1] == 0:
                raise ValueError("dist must be a non-empty [m, n] block, got shape %r" % (dshape,))
            if (mq is not None and mq != dshape[0]) or (nr is not None and nr != dshape[1]):
                raise ValueError("dist %r does not match the features (%r x %r)" % (dshape, mq, nr))
            mq, nr = dshape
        if ql.size != mq or rl.size != nr:
            raise ValueError("label lists (%d, %d) do not match the block (%d x %d)" % (ql.size, rl.size, mq, nr))
        # everything above runs without a GPU
        self.L = _lib.lib()
        dev = _dev()
        if dist is None:
            from .evaluators import _sqdist
            d = _sqdist(torch.as_tensor(qry_feat), torch.as_tensor(ref_feat))
        else:
            d = torch.as_tensor(dist).to(dev, torch.float32)      # no copy for a CUDA float32 tensor; never written to
            if d.stride(1) != 1 or (d.stride(0) < d.shape[1] and d.shape[0] > 1):
                d = d.contiguous()
        self.d, self.m, self.n = d, int(mq), int(nr)
        self.ld = int(d.stride(0)) if self.m > 1 else max(int(d.stride(0)), self.n)
        self.ql = torch.from_numpy(ql).to(dev); self.rl = torch.from_numpy(rl).to(dev)
        self.ws_bytes = int(self.L.ssg_verify_workspace_bytes(self.m, self.n))
        self.ws = torch.empty((self.ws_bytes + 7) // 8, dtype=torch.int64, device=dev)

    def _head(self):
        return (ptr(self.d), self.m, self.n, self.ld, ptr(self.ql), ptr(self.rl))

    def stats(self):
        dev = self.d.device
        counts = torch.empty(2, dtype=torch.int64, device=dev); sums = torch.empty(4, dtype=torch.float64, device=dev)
        minmax = torch.empty(4, dtype=torch.float32, device=dev); status = torch.empty(2, dtype=torch.int32, device=dev)
        check(self.L.ssg_verify_stats_f32(*self._head(), ptr(self.ws), self.ws_bytes, ptr(counts), ptr(sums), ptr(minmax), ptr(status), stream()),
              "ssg_verify_stats_f32")
        return counts.cpu().numpy(), sums.cpu().numpy(), minmax.cpu().numpy(), status.cpu().numpy()

    def select(self, ranks):
        """np.sort(inter s)[ranks] -> float32 array"""
        dev = self.d.device
        out = np.empty(len(ranks), dtype=np.float32)
        for c0 in range(0, len(ranks), MAX_PER_CALL):
            chunk = [int(r) for r in ranks[c0:c0 + MAX_PER_CALL]]
            host = (ctypes.c_int64 * len(chunk))(*chunk)
            values = torch.empty(len(chunk), dtype=torch.float32, device=dev); status = torch.empty(1, dtype=torch.int32, device=dev)
            check(self.L.ssg_verify_select_f32(*self._head(), host, len(chunk), ptr(self.ws), self.ws_bytes, ptr(values), ptr(status), stream()),
                  "ssg_verify_select_f32")
            if int(status.item()):
                raise ValueError("ssg_verify_select_f32: a rank is not below the number of inter elements")
            out[c0:c0 + len(chunk)] = values.cpu().numpy()
        return out

    def count(self, thresholds, is_sq):
        """-> (intra_ge, inter_lt, intra_lt int64 [len(thresholds)], (intra_num, inter_num))"""
        dev = self.d.device
        thresholds = [float(t) for t in thresholds]
        res = np.empty((3, len(thresholds)), dtype=np.int64)
        totals = None
        for c0 in range(0, len(thresholds), MAX_PER_CALL):
            chunk = thresholds[c0:c0 + MAX_PER_CALL]
            host = (ctypes.c_double * len(chunk))(*chunk)
            counts = torch.empty((3, len(chunk)), dtype=torch.int64, device=dev); tot = torch.empty(2, dtype=torch.int64, device=dev)
            check(self.L.ssg_verify_count_f32(*self._head(), 1 if is_sq else 0, host, len(chunk), ptr(self.ws), self.ws_bytes, ptr(counts), ptr(tot),
                                              stream()), "ssg_verify_count_f32")
            res[:, c0:c0 + len(chunk)] = counts.cpu().numpy()
            totals = tot.cpu().numpy()
        return res[0], res[1], res[2], (int(totals[0]), int(totals[1]))


def _emit(lines, text, fid=None, to_fid=None):
    print(text)
    lines.extend(text.split("\n"))
    if fid is not None:
        fid.write(text + "\n" if to_fid is None else to_fid)


def _classification(blk, threshold_l, is_sq, lines, fid):
    thr = np.asarray(threshold_l, dtype=np.float64).reshape(-1)
    if thr.size == 0:
        raise ValueError("threshold_l is empty")
    if np.isnan(thr).any():
        raise ValueError("threshold_l holds a NaN")
    pos_err, neg_err, _, (pos_num, neg_num) = blk.count(thr, is_sq)
    if pos_num == 0 or neg_num == 0:
        raise ValueError("the block has no %s pair" % ("intra" if pos_num == 0 else "inter"))
    pos_err_rate = pos_err.astype('float') / pos_num
    neg_err_rate = neg_err.astype('float') / neg_num
    log = 'pos pair num {}, neg pair num {}\n'.format(pos_num, neg_num)
    _emit(lines, log, fid, log + '\n')
    return pos_err_rate, neg_err_rate


def cal_classification_error(qry_feat, qry_label, ref_feat, ref_label, threshold_l, dist=None, fid=None):
    """eval_far_gar.py:61-100.  As there, `dist` is compared AS GIVEN (no clamp, no sqrt); without `dist` the squared distances of the
    features are compared.  -> (pos_err_rate_arr, neg_err_rate_arr): the shares of intra pairs with dist >= t and inter pairs with dist < t."""
    if len(np.asarray(threshold_l, dtype=np.float64).reshape(-1)) == 0:
        raise ValueError("threshold_l is empty")
    blk = _Block(qry_feat, qry_label, ref_feat, ref_label, dist)
    return _classification(blk, threshold_l, False, [], fid)


def find_metric_threshold(qry_feat, qry_label, ref_feat, ref_label, dist=None, fid=None, far=DEFAULT_FAR):
    """eval_far_gar.py:103-202 on the device.  dist: the SQUARED distance block [m, n] (read only); None: computed from the features
    (ssg_pairwise_sqdist_f32).  far: up to 64 false-accept rates in [0, 1)."""
    far = tuple(float(f) for f in far)
    if not 0 < len(far) <= MAX_PER_CALL:
        raise ValueError("far: 1 .. %d values per call, got %d" % (MAX_PER_CALL, len(far)))
    if any(not (0.0 <= f < 1.0) for f in far):
        raise ValueError("far values must lie in [0, 1)")
    blk = _Block(qry_feat, qry_label, ref_feat, ref_label, dist)
    counts, sums, minmax, status = blk.stats()
    if int(status[1]):
        raise ValueError("find_metric_threshold: NaN in the distance block")
    if int(status[0]):
        raise ValueError("find_metric_threshold: a query has no intra (same label) or no inter (other label) gallery element")
    res = VerificationResult()
    res.lines = lines = []
    res.intra_num, res.inter_num = int(counts[0]), int(counts[1])
    res.intra_min, res.intra_max, res.inter_min, res.inter_max = (np.float32(v) for v in minmax)
    with np.errstate(invalid="ignore"):
        res.intra_avg = float(sums[0]) / res.intra_num
        res.intra_std = float(np.sqrt(np.float64(float(sums[1]) / res.intra_num - res.intra_avg ** 2)))
        res.inter_avg = float(sums[2]) / res.inter_num
        res.inter_std = float(np.sqrt(np.float64(float(sums[3]) / res.inter_num - res.inter_avg ** 2)))
    _emit(lines, 'Intra Distance: {}, {:.4f}+-{:.4f}, min {:.4f}, max {:.4f}'.format(res.intra_num, res.intra_avg, res.intra_std,
                                                                                    res.intra_min, res.intra_max), fid)
    _emit(lines, 'Inter Distance: {}, {:.4f}+-{:.4f}, min {:.4f}, max {:.4f}'.format(res.inter_num, res.inter_avg, res.inter_std,
                                                                                    res.inter_min, res.inter_max), fid)
    res.too_bad = res.intra_avg >= res.inter_avg
    if res.too_bad:
        _emit(lines, 'The Metric Feature Is Too Bad!', fid)
        res.thresholds = res.pos_err_rate = res.neg_err_rate = None
    else:
        res.thresholds = np.linspace(res.intra_avg, res.inter_avg, 10)
        res.pos_err_rate, res.neg_err_rate = _classification(blk, res.thresholds, True, lines, fid)
    res.far = far
    res.num = [int(f * res.inter_num) for f in far]
    res.thr = blk.select(res.num)
    _, _, below, _ = blk.count([float(t) for t in res.thr], True)
    res.cnt = [int(c) for c in below]
    res.GAR = [float(c) / res.intra_num for c in res.cnt]
    for k in range(len(far)):
        _emit(lines, "thr:%.4f  FAR:%.5f(%d/%d)  GAR:%.5f(%d/%d)" % (res.thr[k], far[k], res.num[k], res.inter_num, res.GAR[k], res.cnt[k], res.intra_num), fid)
    return res


findMetricThreshold_MPI = find_metric_threshold
CalClassificationError_MPI = cal_classification_error
