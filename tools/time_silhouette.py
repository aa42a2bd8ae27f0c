#!/usr/bin/env python3
"""Write profiles/silhouette_times.txt (run on the MI355X, e.g. `timeout -k 10 900 python tools/time_silhouette.py`): the silhouette
coefficient of labelings of a precomputed distance (ssg_amd.silhouette, csrc/silhouette.hip) on the re-rank distance of the survey's
synthetic target set (tools/synth.py hard_clustered, 2048 features; source set of 4 000).

Per N in 4 000 and 16 000, on the mode-0 re-rank handle, with eight labelings -- the labels of `generate_selflabel` (rho 1.6e-3) and
the cuts of one OPTICS ordering at the seven multiples of that eps nearest to it that can be scored, each without its noise -- every
call timed with events (median of CALLS calls, ROUNDS rounds: median of the round medians and their min-max), all in the same rounds:
  * ssg_silhouette_sums with K = 1 (the labels of generate_selflabel), each of the eight labelings on its own (their sum is what eight
    separate calls cost), and all eight in one call (K = 8);
  * a device-to-device copy of the matrix, and the rate of the K = 1 and K = 8 passes on the bytes they read against the copy's;
  * the worst-case labeling, two clusters of N / 2: one chain of N / 2 dependent adds per thread, two threads busy per workgroup;
  * `silhouette_many` as called by the sweep, wall clock with the upload, the checks and the blocking read in it.
At N = 4 000 sklearn's silhouette_samples on the host's CPU on the float64 copy with its diagonal zeroed, without the noise, where
sklearn is installed (`--no-sklearn` skips it), with the comparison of its result to the device's, bit for bit."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT,):
    if p not in sys.path:
        sys.path.insert(0, p)

from _timing import CELL, rounds  # noqa: E402 (tools/ is the script's own directory)
import synth  # noqa: E402

CALLS, ROUNDS, WARMUP = 3, 3, 1
SIZES = (4000, 16000)
NS = 4000
RHO = 1.6e-3
CANDIDATES = [1.0 + 0.05 * k * sign for k in range(0, 13) for sign in ((1, -1) if k else (1,))]     # 1.0, 1.05, 0.95, ... 1.6, 0.4
K_MANY = 8


def handle(torch, dev, N):
    from ssg_amd import rerank
    tgt = torch.from_numpy(synth.hard_clustered(N, 2048, 1)).to(dev)
    src = torch.from_numpy(synth.hard_clustered(NS, 2048, 2, intra=0.7)).to(dev)
    return rerank.re_ranking_device(src, tgt, k1=20, k2=6, lambda_value=0.1)


def main():
    import numpy as np
    import torch
    from ssg_amd import OPTICS, _lib, cluster, cluster_optics_dbscan, silhouette, silhouette_many
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    class Lines(list):
        def append(self, line):                 # (progress: every line is shown as soon as it is measured)
            print(line, flush=True)
            list.append(self, line)

    def launcher(h, encs, state=0):
        """-> a function that queues one ssg_silhouette_sums call for these encoded labelings (diag = 1), its arrays already on the device"""
        N, K = h.N, len(encs)
        Cs = [int(e.max()) + 1 for e in encs]
        Cmax = max(Cs)
        lists = [silhouette._member_list(e, C) for e, C in zip(encs, Cs)]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)      # noqa: E731
        lab, mem = up(np.stack(encs)), up(np.stack([l[0] for l in lists]))
        start = up(np.stack([np.concatenate([l[1], np.full(Cmax - C, l[1][-1])]) for l, C in zip(lists, Cs)]))
        ncl = up(np.array(Cs))
        out = torch.empty((2, K, N), dtype=torch.float64, device=dev)
        neg = torch.empty(1, dtype=torch.int64, device=dev)
        keep = (lab, mem, start, ncl, out, neg)
        return lambda: check(L.ssg_silhouette_sums(ptr(h.M), ptr(h.v), N, h.mode, h.lambda_value, None, None, N, K, Cmax, ptr(lab), ptr(mem), ptr(start), ptr(ncl),
                                                   1, state, None, 0, ptr(out[0]), ptr(out[1]), ptr(neg), stream()), "ssg_silhouette_sums") and keep

    out = Lines()
    out.append("Silhouette on %s; labelings cut at multiples of the rho rule's eps (rho %g); every figure: median of %d round medians of %d calls, (min-max of the "
               "round medians); kernels in milliseconds" % (torch.cuda.get_device_name(0), RHO, ROUNDS, CALLS))
    sk_job = None
    for N in SIZES:
        h = handle(torch, dev, N)
        eps, _, _, dbscan_labels, _ = cluster.eps_rule_dbscan(h, RHO, min_samples=4)
        est = OPTICS(metric="precomputed", cluster_method="dbscan", eps=eps, min_samples=4).fit(h)
        labelings, factors = [np.asarray(dbscan_labels)], []
        for f in CANDIDATES:                                     # the cuts nearest to eps that can be scored, until there are K_MANY labelings
            cut = cluster_optics_dbscan(reachability=est.reachability_, core_distances=est.core_distances_, ordering=est.ordering_, eps=eps * f)
            if len(labelings) < K_MANY and silhouette.cut_is_valid(cut):
                labelings.append(cut)
                factors.append(f)
        assert len(labelings) == K_MANY and silhouette.cut_is_valid(labelings[0])
        encs = [silhouette._encode(l, True)[0] for l in labelings]
        K = len(encs)
        out.append("\nN = %d (eps %.6f; a row's stage fits LDS up to m = %d); %d labelings: generate_selflabel's and the OPTICS cuts at eps x %s; clusters / "
                   "clustered samples: %s" % (N, eps, L.ssg_silhouette_lds_max_m(), K, ", ".join("%.2f" % f for f in factors),
                                              ", ".join("%d / %d" % (int(e.max()) + 1, int((e >= 0).sum())) for e in encs)))
        halves = (np.arange(N) >= N // 2).astype(np.int32)
        copy_dst = torch.empty_like(h.M)
        fns = [launcher(h, encs[:1]), launcher(h, encs), lambda: copy_dst.copy_(h.M), launcher(h, [halves])] + [launcher(h, [e]) for e in encs]
        res = rounds(fns, CALLS, ROUNDS, WARMUP)
        rbytes = h.M.numel() * h.M.element_size()
        one, many, copy, worst, each = res[0], res[1], res[2], res[3], res[4:]
        out.append("  K = 1, the labels of generate_selflabel     " + CELL % one + "   reads %.0f MB: %.0f GB/s" % (rbytes / 1e6, rbytes / one[0] / 1e6))
        out.append("  K = %d, one pass over the matrix             " % K + CELL % many + "   reads %.0f MB: %.0f GB/s" % (rbytes / 1e6, rbytes / many[0] / 1e6))
        total = sum(e[0] for e in each)
        out.append("  the same %d labelings in %d calls of K = 1: %9.4f in all (%s); K = %d in one call takes %.2f of that" % (
            K, K, total, ", ".join("%.4f" % e[0] for e in each), K, many[0] / total))
        out.append("  device copy of the same matrix              " + CELL % copy + "   reads %.0f MB: %.0f GB/s; the K = 1 pass runs at %.2f and the K = %d pass at %.2f "
                   "of the copy's rate on the bytes they read" % (rbytes / 1e6, rbytes / copy[0] / 1e6, copy[0] / one[0], K, copy[0] / many[0]))
        out.append("  worst case, two clusters of N / 2, K = 1    " + CELL % worst + "   one chain of %d dependent adds per thread and row, two threads busy per "
                   "workgroup: %.2f times the K = 1 pass" % (N // 2, worst[0] / one[0]))
        walls = []
        for _ in range(ROUNDS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sils = silhouette_many(h, labelings, diagonal="zero", ignore_noise=True)
            walls.append(time.perf_counter() - t0)
        out.append("  silhouette_many(K = %d, diagonal='zero', ignore_noise=True), wall clock with upload, checks and the blocking read: %.4f s (%.4f-%.4f)" % (
            K, statistics.median(walls[1:]), min(walls[1:]), max(walls[1:])))
        if N == SIZES[0] and "--no-sklearn" not in sys.argv:
            sk_job = (N, h.final_dist().cpu().numpy(), labelings[0], sils[0])
        del h, copy_dst, fns
        torch.cuda.empty_cache()
    if sk_job:
        try:
            import sklearn
            from sklearn.metrics import silhouette_samples
        except ImportError:
            out.append("\nsklearn is not installed here: its CPU time was not measured")
        else:
            N, X, lab, got = sk_job
            np.fill_diagonal(X, 0.0)
            keep = lab != -1
            sub = np.ascontiguousarray(X[keep][:, keep])
            t0 = time.perf_counter()
            want = silhouette_samples(sub, lab[keep], metric="precomputed")
            t = time.perf_counter() - t0
            same = np.array_equal(want.view(np.uint64), np.ascontiguousarray(got[keep]).view(np.uint64))
            out.append("\nsklearn %s on the host's CPU, N = %d, the labels of generate_selflabel without their noise (%d samples): silhouette_samples %.3f s on the "
                       "float64 copy with its diagonal zeroed; result identical to the device's bit for bit: %s" % (sklearn.__version__, N, int(keep.sum()), t, same))
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "silhouette_times.txt"), "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
