#!/usr/bin/env python3
"""Write profiles/optics_times.txt (run on the MI355X, e.g. `timeout -k 10 900 python tools/time_optics.py`): OPTICS on a precomputed
distance (ssg_amd.optics.OPTICS, csrc/optics.hip) on the re-rank distance of the survey's synthetic target set (tools/synth.py
hard_clustered, 2048 features; source set of 4 000).

Per N in 4 000 and 16 000:
  * `fit` (cluster_method='xi', min_samples=4) on the mode-0 re-rank handle and on its float64 final_dist, wall clock with the blocking
    read in it: one warm-up, then the median and min-max of FITS fits; the host's xi extraction on its own;
  * the two kernels, each call timed with events: core distances, and the ordering loop with its state in LDS and in global memory
    (median of CALLS calls, ROUNDS rounds: median of the round medians and their min-max), and the loop's time per step;
  * `DBSCAN.fit` at the rho rule's eps on the same handle, the same way.
sklearn's OPTICS(metric='precomputed', min_samples=4) on the host's CPU at N = 2 000 and 4 000 where sklearn is installed
(`--no-sklearn` skips it), with the comparison of all four arrays to the device's."""
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT,):
    if p not in sys.path:
        sys.path.insert(0, p)

from _timing import CELL, rounds  # noqa: E402 (tools/ is the script's own directory)
import synth  # noqa: E402

CALLS, ROUNDS, WARMUP, FITS = 5, 3, 1, 5
SIZES = (4000, 16000)
SK_SIZES = (2000, 4000)
NS, RHO = 4000, 1.6e-3


def wall(fn, torch, n=FITS):
    fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def handle(torch, dev, N):
    from ssg_amd import rerank
    tgt = torch.from_numpy(synth.hard_clustered(N, 2048, 1)).to(dev)
    src = torch.from_numpy(synth.hard_clustered(NS, 2048, 2, intra=0.7)).to(dev)
    return rerank.re_ranking_device(src, tgt, k1=20, k2=6, lambda_value=0.1)


def main():
    import numpy as np
    import torch
    from ssg_amd import DBSCAN, OPTICS, _lib, cluster, optics
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    class Lines(list):
        def append(self, line):                 # (progress: every line is shown as soon as it is measured)
            print(line, flush=True)
            list.append(self, line)

    out = Lines()
    out.append("OPTICS on %s; min_samples 4, max_eps inf; kernels: medians of %d round medians of %d calls, (min-max of the round medians), milliseconds"
               % (torch.cuda.get_device_name(0), ROUNDS, CALLS))
    finals = {}
    for N in sorted(set(SIZES + SK_SIZES)):
        h = handle(torch, dev, N)
        F = h.final_dist()
        if N in SK_SIZES and "--no-sklearn" not in sys.argv:
            finals[N] = F.cpu().numpy()
        if N not in SIZES:
            continue
        out.append("\nN = %d" % N)
        est = OPTICS(metric="precomputed", min_samples=4)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for what, X in (("mode-0 re-rank handle", h), ("float64 matrix", F)):
                m, lo, hi = wall(lambda: est.fit(X), torch)
                out.append("  fit on the %-22s %8.4f s (%.4f-%.4f), median of %d; %d xi clusters, %d noise points" % (
                    what + ":", m, lo, hi, FITS, est.labels_.max() + 1, int((est.labels_ < 0).sum())))
            t0 = time.perf_counter()
            optics.cluster_optics_xi(reachability=est.reachability_, predecessor=est.predecessor_, ordering=est.ordering_, min_samples=4)
            out.append("    of which the xi extraction on the host: %.4f s" % (time.perf_counter() - t0))
        core = torch.empty(N, dtype=torch.float64, device=dev)
        ws = torch.empty(N, dtype=torch.float64, device=dev)
        o, p = torch.empty(N, dtype=torch.int64, device=dev), torch.empty(N, dtype=torch.int64, device=dev)
        r = torch.empty(N, dtype=torch.float64, device=dev)
        inf = float("inf")
        for what, (M, v, mode, lam) in (("handle", (h.M, h.v, h.mode, h.lambda_value)), ("float64", (F, None, 2, 0.0))):
            fns = [lambda: check(L.ssg_optics_core_dist(ptr(M), ptr(v), N, mode, lam, 4, inf, ptr(core), stream()), "ssg_optics_core_dist")]
            for state in (1, 2):
                fns.append(lambda state=state: check(L.ssg_optics_order(ptr(M), ptr(v), N, mode, lam, ptr(core), inf, state, ptr(ws), N * 8, ptr(o), ptr(r), ptr(p),
                                                                        stream()), "ssg_optics_order"))
            fns[0]()
            res = rounds(fns, CALLS, ROUNDS, WARMUP)
            out.append("  %-8s core distances            " % what + CELL % res[0])
            for (med, lo, hi), place in zip(res[1:], ("LDS", "global memory")):
                out.append("  %-8s ordering loop, state in %-14s" % (what, place + ":") + CELL % (med, lo, hi) + "   %.3f us per step" % (med * 1e3 / N))
        eps = float(cluster.eps_rule(h, RHO)[0])
        db = DBSCAN(eps=eps, min_samples=4, metric="precomputed")
        m, lo, hi = wall(lambda: db.fit(h), torch)
        out.append("  DBSCAN.fit on the handle at eps %.4f (rho %.1e): %8.4f s (%.4f-%.4f); %d clusters, %d noise points" % (
            eps, RHO, m, lo, hi, db.labels_.max() + 1, int((db.labels_ < 0).sum())))
        del h, F
    if finals:
        try:
            import sklearn
            from sklearn.cluster import OPTICS as SkOPTICS
        except ImportError:
            out.append("\nsklearn is not installed here: its CPU time was not measured")
        else:
            out.append("")
            for N, X in finals.items():
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    t0 = time.perf_counter()
                    sk = SkOPTICS(metric="precomputed", min_samples=4).fit(X)
                    t = time.perf_counter() - t0
                    est = OPTICS(metric="precomputed", min_samples=4).fit(X)
                same = all(np.array_equal(getattr(sk, a), getattr(est, a)) for a in ("ordering_", "core_distances_", "reachability_", "predecessor_", "labels_"))
                out.append("sklearn %s on the host's CPU, N = %d: fit %.2f s; ordering_, core_distances_, reachability_, predecessor_ and labels_ "
                           "identical to the device's: %s" % (sklearn.__version__, N, t, same))
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "optics_times.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
