"""Hausdorff re-ranking -- host-side mirror of reid/rerank_hausdorff.py:7-65 `re_ranking`.

`re_ranking(input_feature_source, input_feature, k=20, lambda_value=0.1, MemorySave=False, Minibatch=2000)` keeps the reference
signature and returns `(euclidean_dist float16 [N, N], final_dist float64 [N, N])` as numpy arrays, bit for bit what the reference
returns.  `re_ranking_hausdorff_device` is the device path: it returns a mode 2 `DistHandle` (M = the float64 final matrix,
euclid = the normalised half matrix) that `eps_rule` / `DBSCAN` / `generate_selflabel` consume like the handles of the other variants.

Stages: half original distance and kNN sets exactly as rerank_plain.py (the reference's lines are identical) on the kernels of that
path; source vector, float64 target distance matrix E, directed distances, their symmetric maximum H and the blend in
csrc/hausdorff.hip.  Memory: E and H (8 N^2 bytes each) + the half matrix (2 N^2, the normalised copy replaces it) = about 18 N^2
bytes at the peak.  Single GPU, N * N < 2^31.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from .rerank import DeviceBackedArray, DistHandle, ReRankNaNError, _as_dev_f32, _original_distance, range_stats

MAX_ENTRIES = 2 ** 31      # N * N must stay below it (entry indices of the row kernels)


def check_limits(N, k):
    """the argument refusals of the variant (no GPU work has been queued when they raise)"""
    if not (2 <= k <= min(N, 64)):
        raise ValueError("re_ranking (hausdorff): need 2 <= k <= min(N, 64), got k=%d N=%d" % (k, N))
    if N * N >= MAX_ENTRIES:
        raise ValueError("re_ranking (hausdorff): need N * N < 2^31 (N <= 46340), got N=%d" % N)


def re_ranking_hausdorff_device(src, tgt, k=20, lambda_value=0.1, stages=None, memory_save=False):
    N = int(tgt.shape[0])
    check_limits(N, k)
    L = _lib.lib()
    dev = tgt.device if torch.is_tensor(tgt) and tgt.is_cuda else torch.device("cuda", torch.cuda.current_device())
    src = _as_dev_f32(src, dev); tgt = _as_dev_f32(tgt, dev)     # (zero padding of d adds +0.0 to every sum: no bit changes)
    Ns, d = src.shape[0], tgt.shape[1]
    st = stream()
    stats = range_stats(tgt, src)
    D, rowmax, flag = _original_distance(L, tgt, 0, N, stats[0], st, memory_save)
    # k-th smallest entry of every row and the sets S_i (rerank_hausdorff.py:43-49), as in the kNN-set variant
    ones = torch.full((N,), 0x3C00, dtype=torch.int32, device=dev)      # rowmax = half(1): keys are the raw values
    rank = torch.empty((N, k), dtype=torch.int32, device=dev)
    check(L.ssg_topk_rank(ptr(D), ptr(ones), N, N, k, ptr(rank), st), "ssg_topk_rank")
    cap = max(64, 4 * k)
    while True:
        a_idx = torch.empty((N, cap), dtype=torch.int32, device=dev); a_val = torch.empty((N, cap), dtype=torch.float16, device=dev)
        a_nnz = torch.empty(N, dtype=torch.int32, device=dev); ovf = torch.zeros(1, dtype=torch.int32, device=dev)
        check(L.ssg_knn_sets(ptr(D), ptr(rank), N, 0, N, k, cap, ptr(a_idx), ptr(a_val), ptr(a_nnz), ptr(ovf), st), "ssg_knn_sets")
        if not int(ovf.item()):
            break
        cap = min(N, cap * 8)          # many exact ties at the k-th distance: retry with room for them
    del a_val
    # source-domain term (:13-15)
    status = torch.zeros(2, dtype=torch.float64, device=dev)            # [max(vec), max(H)]
    rowmin = torch.empty(N, dtype=torch.float64, device=dev); vec = torch.empty(N, dtype=torch.float64, device=dev)
    check(L.ssg_seqdist_rowmin_f64(ptr(tgt), N, ptr(src), Ns, d, ptr(rowmin), st), "ssg_seqdist_rowmin_f64")
    check(L.ssg_hausdorff_source_finish(ptr(rowmin), N, ptr(vec), ptr(status[0:1]), st), "ssg_hausdorff_source_finish")
    # normalised half matrix (:41)
    euclid = torch.empty_like(D); dmax = torch.empty(1, dtype=torch.int32, device=dev)
    check(L.ssg_half_div_max(ptr(D), ptr(rowmax), N, ptr(euclid), ptr(dmax), st), "ssg_half_div_max")
    if stages is None:
        del D
    # float64 target distances and Hausdorff rows (:52-58)
    E = torch.empty((N, N), dtype=torch.float64, device=dev)
    check(L.ssg_seqdist_self_f64(ptr(tgt), N, d, 1, ptr(E), N, st), "ssg_seqdist_self_f64")
    H = torch.empty((N, N), dtype=torch.float64, device=dev)
    nws = int(L.ssg_hausdorff_workspace_bytes(N, N))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    check(L.ssg_hausdorff_directed_rows(ptr(E), ptr(a_idx), ptr(a_nnz), cap, N, 0, N, ptr(H), ptr(ws), nws, st), "ssg_hausdorff_directed_rows")
    check(L.ssg_hausdorff_symmetrize(ptr(H), N, ptr(status[1:2]), st), "ssg_hausdorff_symmetrize")
    if stages is not None:
        stages.update(D=D, vec=vec, a_idx=a_idx, a_nnz=a_nnz, E=E, H=H.clone())
    del E
    # blend (:60-62), over H in place
    check(L.ssg_hausdorff_blend(ptr(H), ptr(status[1:2]), ptr(vec), N, 0, N, 1.0 - float(lambda_value), float(lambda_value), ptr(H), st),
          "ssg_hausdorff_blend")
    # the blocking read of the status words (the others of a call: range_stats' and one per attempt of the set capacity loop)
    words = torch.cat([status, (flag if flag is not None else torch.zeros(1, dtype=torch.int32, device=dev)).to(torch.float64)]).tolist()
    if words[2]:
        raise _lib.SSGError("ssg_gram_i8_encode: a feature did not fit the digit count chosen from max|feat| (internal error)")
    if words[0] == 0:
        raise ReRankNaNError("max(source_dist_vec) == 0: every target row is also a source row; the reference "
                             "(reid/rerank_hausdorff.py:15) would return an all-NaN final_dist")
    if words[1] == 0:
        raise ReRankNaNError("max(hausdorff_dist) == 0: all neighbour sets coincide (identical target rows); the reference "
                             "(reid/rerank_hausdorff.py:60) would return an all-NaN final_dist")
    return DistHandle(N, 2, H, lambda_value=lambda_value, euclid=euclid)


def re_ranking(input_feature_source, input_feature, k=20, lambda_value=0.1, MemorySave=False, Minibatch=2000, device=None):
    """Drop-in for reid/rerank_hausdorff.py:7 re_ranking (numpy in, numpy out).  Minibatch only sizes the reference's row chunks
    and changes no value: accepted and ignored."""
    check_limits(int(input_feature.shape[0]), k)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    print('computing source distance...')
    print('computing original distance...')
    h = re_ranking_hausdorff_device(_as_dev_f32(np.asarray(input_feature_source), device), _as_dev_f32(np.asarray(input_feature), device),
                                    k=k, lambda_value=lambda_value, memory_save=MemorySave)
    from . import hostio
    euclid = hostio.to_host(h.euclid, wait=False)
    final = DeviceBackedArray.attach(hostio.final_dist_to_host(h).numpy(), h)      # (waits for the copy stream: both copies have landed)
    return euclid.numpy(), final
