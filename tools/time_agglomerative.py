#!/usr/bin/env python3
"""Write profiles/agglomerative_times.txt (run on the MI355X, e.g. `timeout -k 10 900 python tools/time_agglomerative.py`): agglomerative
clustering of a precomputed distance (ssg_amd.agglomerative, csrc/agglomerative.hip) on the re-rank distance of the survey's synthetic
target set (tools/synth.py hard_clustered, 2048 features; source set of 4 000).

Per N in 4 000 and 16 000, on the mode-0 re-rank handle:
  * `fit` for each linkage, cut at the rho rule's eps (rho 1.6e-3), wall clock with the blocking read in it, and the host stage (stable
    sort, label, cut) on its own: one warm-up, then the median of ROUNDS round medians of FITS calls and their min-max;
  * the kernels, each call timed with events (median of CALLS calls, ROUNDS rounds: median of the round medians and their min-max): the
    check pass and the expand pass against a device-to-device copy's rate on the bytes each moves; the merge loop for every method with
    its state in LDS and in global memory (the working square is expanded afresh, untimed, before every call), with the time per scan
    and per merge;
  * sklearn's AgglomerativeClustering on the host's CPU on the float64 copy where sklearn is installed (`--no-sklearn` skips it), with
    the comparison of labels_ to the device's."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT,):
    if p not in sys.path:
        sys.path.insert(0, p)

from _timing import CELL, rounds, timed  # noqa: E402 (tools/ is the script's own directory)
import synth  # noqa: E402

CALLS, ROUNDS, WARMUP, FITS = 3, 3, 1, 3
SIZES = (4000, 16000)
NS = 4000
RHO = 1.6e-3
LINKAGES = ("average", "complete", "single")


def wall(fn, sync, n=FITS, nrounds=ROUNDS):
    """seconds of one call with the blocking work in it: one warm-up, then (median, min, max) of the medians of `nrounds` rounds of n calls"""
    fn()
    meds = []
    for _ in range(nrounds):
        ts = []
        for _ in range(n):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts.append(time.perf_counter() - t0)
        meds.append(statistics.median(ts))
    return statistics.median(meds), min(meds), max(meds)


def handle(torch, dev, N):
    from ssg_amd import rerank
    tgt = torch.from_numpy(synth.hard_clustered(N, 2048, 1)).to(dev)
    src = torch.from_numpy(synth.hard_clustered(NS, 2048, 2, intra=0.7)).to(dev)
    return rerank.re_ranking_device(src, tgt, k1=20, k2=6, lambda_value=0.1)


def main():
    import numpy as np
    import torch
    from ssg_amd import AgglomerativeClustering, _lib, agglomerative, cluster
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    class Lines(list):
        def append(self, line):                 # (progress: every line is shown as soon as it is measured)
            print(line, flush=True)
            list.append(self, line)

    out = Lines()
    out.append("Agglomerative clustering on %s; cut at the rho rule's eps (rho %g); every figure: median of %d round medians of %d calls, (min-max of the "
               "round medians); kernels in milliseconds" % (torch.cuda.get_device_name(0), RHO, ROUNDS, CALLS))
    sk_jobs = []
    for N in SIZES:
        h = handle(torch, dev, N)
        eps = float(cluster.eps_rule(h, RHO)[0])
        out.append("\nN = %d (eps %.6f; the loop's state fits LDS up to N = %d)" % (N, eps, L.ssg_agglo_lds_max_n()))
        labels = {}
        for linkage in LINKAGES:
            est = AgglomerativeClustering(n_clusters=None, distance_threshold=eps, metric="precomputed", linkage=linkage)
            m, lo, hi = wall(lambda: est.fit(h), torch.cuda.synchronize)
            labels[linkage] = est.labels_.copy()
            out.append("  fit, %-8s linkage, on the mode-0 re-rank handle: %8.4f s (%.4f-%.4f); %d clusters" % (linkage, m, lo, hi, est.n_clusters_))
            x, y, d = (a.copy() for a in agglomerative._device_merges(h, agglomerative._METHODS[linkage])[4:7])
            out.append("    of which the host stage (stable sort, label, cut): %.4f s (%.4f-%.4f)" % wall(
                lambda: agglomerative._hc_cut(est.n_clusters_, agglomerative._label(x, y, d)[:, :2].astype(int), N), lambda: None))
        ld = (N + 3) & ~3
        W = torch.empty((N, ld), dtype=torch.float64, device=dev)
        W2 = torch.empty_like(W)
        i = torch.empty(4 + 3 * N, dtype=torch.int64, device=dev)
        f = torch.empty(N, dtype=torch.float64, device=dev)
        ws = torch.empty(ld, dtype=torch.float64, device=dev)
        copy_dst = torch.empty_like(h.M)
        a = (ptr(h.M), ptr(h.v), N, h.mode, h.lambda_value)
        expand = lambda: check(L.ssg_agglo_expand(*a, ptr(W), ld, stream()), "ssg_agglo_expand")      # noqa: E731
        res = rounds([lambda: check(L.ssg_agglo_check(*a, ptr(i[:2]), stream()), "ssg_agglo_check"), lambda: copy_dst.copy_(h.M), expand, lambda: W2.copy_(W)],
                     CALLS, ROUNDS, WARMUP)
        rbytes, wbytes = h.M.numel() * h.M.element_size(), W.numel() * 8
        out.append("  check pass (NaN and inf)                  " + CELL % res[0] + "   reads %.0f MB: %.0f GB/s" % (rbytes / 1e6, rbytes / res[0][0] / 1e6))
        out.append("  device copy of the same matrix            " + CELL % res[1] + "   reads %.0f MB: %.0f GB/s; the check pass runs at %.2f of the copy's rate on "
                   "the bytes it reads" % (rbytes / 1e6, rbytes / res[1][0] / 1e6, res[1][0] / res[0][0]))
        out.append("  expand pass (upper triangle -> float64 W) " + CELL % res[2] + "   reads %.0f MB, writes %.0f MB: %.0f GB/s written" % (
            rbytes / 2e6, wbytes / 1e6, wbytes / res[2][0] / 1e6))
        out.append("  device copy of W                          " + CELL % res[3] + "   writes %.0f MB: %.0f GB/s; the expand pass runs at %.2f of the copy's rate "
                   "on the bytes it writes" % (wbytes / 1e6, wbytes / res[3][0] / 1e6, res[3][0] / res[2][0]))
        n1 = N - 1
        for linkage in LINKAGES:
            for state, place in ((1, "LDS"), (2, "global memory")):
                loop = lambda: check(L.ssg_agglo_nn_chain(ptr(W), N, ld, agglomerative._METHODS[linkage], state, ptr(i[:2]), ptr(ws), ld * 8, ptr(i[4:4 + n1]),      # noqa: E731
                                                          ptr(i[4 + N:4 + N + n1]), ptr(f), ptr(i[4 + 2 * N:4 + 2 * N + n1]), ptr(i[2:4]), stream()), "ssg_agglo_nn_chain")
                meds = []
                for r in range(ROUNDS + 1):
                    ts = []
                    for _ in range(CALLS if r else WARMUP):
                        expand()
                        ts.append(timed(loop))
                    if r:
                        meds.append(statistics.median(ts))
                flag, scans = (int(v) for v in i[2:4].cpu())
                assert flag == 0
                med = (statistics.median(meds), min(meds), max(meds))
                out.append("  merge loop, %-8s state in %-14s" % (linkage + ",", place + ":") + CELL % med + "   %d %s: %.3f us per %s, %.3f us per merge" % (
                    scans, "steps" if linkage == "single" else "scans", med[0] * 1e3 / scans, "step" if linkage == "single" else "scan", med[0] * 1e3 / n1))
        if "--no-sklearn" not in sys.argv:
            sk_jobs.append((N, eps, h.final_dist().cpu().numpy(), labels))
        del h, W, W2, copy_dst
        torch.cuda.empty_cache()
    if sk_jobs:
        try:
            import sklearn
            from sklearn.cluster import AgglomerativeClustering as Sk
        except ImportError:
            out.append("\nsklearn is not installed here: its CPU time was not measured")
        else:
            out.append("")
            for N, eps, X, labels in sk_jobs:
                for linkage in LINKAGES:
                    t0 = time.perf_counter()
                    sk = Sk(n_clusters=None, distance_threshold=eps, metric="precomputed", linkage=linkage).fit(X)
                    t = time.perf_counter() - t0
                    out.append("sklearn %s on the host's CPU, N = %d, %-8s linkage: fit %.2f s on the float64 copy; labels_ identical to the device's: %s" % (
                        sklearn.__version__, N, linkage, t, np.array_equal(sk.labels_, labels[linkage])))
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "agglomerative_times.txt"), "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
