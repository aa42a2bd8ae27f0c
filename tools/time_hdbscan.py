#!/usr/bin/env python3
"""Write profiles/hdbscan_times.txt (run on the MI355X, e.g. `timeout -k 10 900 python tools/time_hdbscan.py`): HDBSCAN on a precomputed
distance (ssg_amd.hdbscan.HDBSCAN, csrc/hdbscan.hip) on the re-rank distance of the survey's synthetic target set (tools/synth.py
hard_clustered, 2048 features; source set of 4 000).

Per N in 4 000 and 16 000, on the mode-0 re-rank handle:
  * `fit` (min_cluster_size 4), wall clock with the blocking read in it, and the host stage (sort, single linkage, condensed tree,
    selection, labels, probabilities) on its own: one warm-up, then the median of ROUNDS round medians of FITS calls and their min-max;
  * the kernels, each call timed with events (median of CALLS calls, ROUNDS rounds: median of the round medians and their min-max):
    the check pass, the core distances, the spanning-tree loop with its state in LDS and in global memory, with the time per step;
  * in the same rounds, on the same matrix, `ssg_optics_order` in both placements -- the yardstick: code of the parent commit that does
    strictly more arithmetic per element -- and the verdict per placement (a side wins when its median is lower by more than the larger
    of the two spreads);
  * a device-to-device copy of the matrix, and the check pass's rate on the bytes it reads as a fraction of the copy's.
Where a build of the library with the core distances in LDS exists (_ab/libssg_hip_corelds.so: the hipcc line of __graft_entry__.py with
-DSSG_HDBSCAN_CORE_LDS=1), the loop of both builds is timed in fresh child processes at N = 4 000 and 10 000 (the larger build holds
10 223 nodes).  sklearn's HDBSCAN(metric='precomputed', min_cluster_size=4) on the host's CPU at N = 2 000 and 4 000 where sklearn is
installed (`--no-sklearn` skips it), with the comparison of labels_ and probabilities_ to the device's."""
import os
import statistics
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT,):
    if p not in sys.path:
        sys.path.insert(0, p)

from _timing import CELL, rounds, verdict  # noqa: E402 (tools/ is the script's own directory)
import synth  # noqa: E402

CALLS, ROUNDS, WARMUP, FITS = 5, 3, 1, 5
SIZES = (4000, 16000)
SK_SIZES = (2000, 4000)
AB_SIZES = (4000, 10000)
NS = 4000
AB_LIB = os.path.join(ROOT, "_ab", "libssg_hip_corelds.so")


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


def mst_call(L, h, core, state, bufs):
    from ssg_amd._lib import check, ptr, stream
    ws, cur, nxt, dist = bufs
    return lambda: check(L.ssg_hdbscan_mst(ptr(h.M), ptr(h.v), h.N, h.mode, h.lambda_value, ptr(core), 1.0, state, ptr(ws), h.N * 8, ptr(cur), ptr(nxt), ptr(dist),
                                           stream()), "ssg_hdbscan_mst")


def buffers(torch, dev, N):
    return (torch.empty(N + 1, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int64, device=dev), torch.empty(N, dtype=torch.int64, device=dev),
            torch.empty(N, dtype=torch.float64, device=dev))


def child():
    """--mst-only: the loop of whatever build SSG_LIB_PATH names, state in LDS, one line per size"""
    import torch
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for N in AB_SIZES:
        h = handle(torch, dev, N)
        core = torch.empty(N, dtype=torch.float64, device=dev)
        check(L.ssg_hdbscan_core_dist(ptr(h.M), ptr(h.v), N, h.mode, h.lambda_value, 4, 1.0, ptr(core), stream()), "ssg_hdbscan_core_dist")
        (res,) = rounds([mst_call(L, h, core, 1, buffers(torch, dev, N))], CALLS, ROUNDS, WARMUP)
        print("AB N = %5d  loop, state in LDS (this build holds %5d nodes there): " % (N, L.ssg_hdbscan_lds_max_n()) + CELL % res
              + "   %.3f us per step" % (res[0] * 1e3 / (N - 1)), flush=True)


def main():
    import numpy as np
    import torch
    from ssg_amd import HDBSCAN, _lib, hdbscan
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    class Lines(list):
        def append(self, line):                 # (progress: every line is shown as soon as it is measured)
            print(line, flush=True)
            list.append(self, line)

    out = Lines()
    out.append("HDBSCAN on %s; min_cluster_size 4 (min_samples 4), alpha 1; every figure: median of %d round medians of %d calls, (min-max of the round medians); "
               "kernels in milliseconds" % (torch.cuda.get_device_name(0), ROUNDS, CALLS))
    finals = {}
    for N in sorted(set(SIZES + SK_SIZES)):
        h = handle(torch, dev, N)
        if N in SK_SIZES and "--no-sklearn" not in sys.argv:
            finals[N] = (h.final_dist().cpu().numpy(), HDBSCAN(metric="precomputed", min_cluster_size=4).fit(h))
        if N not in SIZES:
            continue
        out.append("\nN = %d" % N)
        est = HDBSCAN(metric="precomputed", min_cluster_size=4)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m, lo, hi = wall(lambda: est.fit(h), torch.cuda.synchronize)
        out.append("  fit on the mode-0 re-rank handle:   %8.4f s (%.4f-%.4f); %d clusters, %d noise points" % (
            m, lo, hi, est.labels_.max() + 1, int((est.labels_ < 0).sum())))
        out.append("    of which the host stage (sort, single linkage, condensed tree, selection, labels): %.4f s (%.4f-%.4f)"
                   % wall(lambda: hdbscan._tree_from_mst(*est._mst, 4), lambda: None))
        core = torch.empty(N, dtype=torch.float64, device=dev)
        ocore = torch.empty(N, dtype=torch.float64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        bufs = buffers(torch, dev, N)
        ws, o, p, r = bufs
        copy_dst = torch.empty_like(h.M)
        a = (ptr(h.M), ptr(h.v), N, h.mode, h.lambda_value)
        inf = float("inf")
        check(L.ssg_hdbscan_core_dist(*a, 4, 1.0, ptr(core), stream()), "ssg_hdbscan_core_dist")
        check(L.ssg_optics_core_dist(*a, 4, inf, ptr(ocore), stream()), "ssg_optics_core_dist")
        fns = [lambda: check(L.ssg_hdbscan_check(*a, ptr(counts), stream()), "ssg_hdbscan_check"),
               lambda: copy_dst.copy_(h.M),
               lambda: check(L.ssg_hdbscan_core_dist(*a, 4, 1.0, ptr(core), stream()), "ssg_hdbscan_core_dist"),
               mst_call(L, h, core, 1, bufs), mst_call(L, h, core, 2, bufs)]
        for state in (1, 2):
            fns.append(lambda state=state: check(L.ssg_optics_order(*a, ptr(ocore), inf, state, ptr(ws), N * 8, ptr(o), ptr(r), ptr(p), stream()), "ssg_optics_order"))
        res = rounds(fns, CALLS, ROUNDS, WARMUP)
        nbytes = h.M.numel() * h.M.element_size()
        out.append("  check pass (NaN and symmetry)          " + CELL % res[0] + "   reads %.0f MB: %.0f GB/s" % (nbytes / 1e6, nbytes / res[0][0] / 1e6))
        out.append("  device copy of the same matrix         " + CELL % res[1] + "   reads %.0f MB: %.0f GB/s; the check pass runs at %.2f of the copy's rate "
                   "on the bytes it reads" % (nbytes / 1e6, nbytes / res[1][0] / 1e6, res[1][0] / res[0][0]))
        out.append("  core distances                         " + CELL % res[2])
        for i, place in ((3, "LDS"), (4, "global memory")):
            out.append("  spanning-tree loop, state in %-14s" % (place + ":") + CELL % res[i] + "   %.3f us per step" % (res[i][0] * 1e3 / (N - 1)))
        for i, place in ((5, "LDS"), (6, "global memory")):
            out.append("  ssg_optics_order,   state in %-14s" % (place + ":") + CELL % res[i] + "   %.3f us per step" % (res[i][0] * 1e3 / N))
        for i, j, place in ((3, 5, "LDS"), (4, 6, "global memory")):
            ps = [tuple(x / (N - 1) for x in res[i]), tuple(x / N for x in res[j])]
            out.append("  per step, state in %s: %s" % (place, verdict(ps[0], ps[1], "the spanning-tree loop is faster than the OPTICS loop",
                                                                      "the spanning-tree loop is SLOWER than the OPTICS loop", "no difference beyond the spread")))
        del h
    if os.path.exists(AB_LIB):
        out.append("\nwhere core[] lives: the committed build (read from global memory) against a build with a copy in LDS, fresh processes, state in LDS")
        for what, env in (("core[] from global memory / L2", {}), ("core[] copied into LDS", {"SSG_LIB_PATH": AB_LIB})):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mst-only"], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("AB ")]
            if r.returncode != 0 or not lines:
                out.append("  %s: the child failed (%d): %s" % (what, r.returncode, r.stderr.strip()[-300:]))
            for ln in lines:
                out.append("  %-32s %s" % (what + ":", ln[3:]))
    else:
        out.append("\n(no build with the core distances in LDS at _ab/libssg_hip_corelds.so: that comparison was not measured)")
    if finals:
        try:
            import sklearn
            from sklearn.cluster import HDBSCAN as SkHDBSCAN
        except ImportError:
            out.append("\nsklearn is not installed here: its CPU time was not measured")
        else:
            out.append("")
            for N, (X, est) in finals.items():
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    t0 = time.perf_counter()
                    sk = SkHDBSCAN(metric="precomputed", min_cluster_size=4, copy=True).fit(X)
                    t = time.perf_counter() - t0
                same = np.array_equal(sk.labels_, est.labels_) and sk.probabilities_.tobytes() == est.probabilities_.tobytes()
                out.append("sklearn %s on the host's CPU, N = %d: fit %.2f s (with its copy of the float64 matrix); labels_ and probabilities_ identical to the "
                           "device's on this machine: %s" % (sklearn.__version__, N, t, same))
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "hdbscan_times.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    if "--mst-only" in sys.argv:
        child()
    else:
        main()
