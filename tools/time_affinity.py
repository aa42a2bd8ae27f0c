#!/usr/bin/env python3
"""Write profiles/affinity_times.txt (run on the MI355X, e.g. `timeout -k 10 900 python tools/time_affinity.py`): affinity propagation
(ssg_amd.cluster.AffinityPropagation, csrc/affinity.hip) on the negated Euclidean distances of noisy unit-sphere blobs (N / 25 blobs of 25
points, 64 features, generated on the device).

Per N in 4 000 and 16 000:
  * the two loop kernels, each call timed on its own with events after 5 warm-up iterations of the loop: the row kernel (A update of one
    iteration + R update of the next) and the column walk (the ordered column sums), interleaved with a device-to-device copy of one
    N x N float64 matrix; a round takes the median of CALLS calls of each in turn, ROUNDS rounds; the table shows the median of the round
    medians and their min-max (the spread);
  * the bytes of the floor model (row kernel: read R, A, S, write A, R and one more read of S = 6 x 8 N^2; column walk: 8 N^2) over the
    time, as a fraction of the copy's rate (the copy moves 2 x 8 N^2 bytes) measured in the same rounds;
  * the host's noise generation (numpy RandomState.standard_normal) and its upload, separately;
  * a whole fit, wall clock with a final synchronisation: the first (noise drawn and uploaded) and the median of three more (noise cached).
sklearn's fit on the host's CPU is timed at N = 4 000 only (`--no-sklearn` skips it).

`--sweep`: after the table, every tile of the column walk (`ssg_ap_colsum_cfg_f64`, index 0 .. ssg_ap_colsum_configs() - 1) and the
automatic choice, at both sizes and at N = 8 192 and 8 208 (the two sides of the choice), on a seeded matrix, with a sha256 of the sums:
every tile must give the same bits."""
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

CALLS, ROUNDS, WARMUP = 7, 5, 3
SIZES = (4000, 16000)


def similarities(torch, dev, N, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    P, d = max(N // 25, 1), 64
    c = torch.randn((P, d), device=dev, dtype=torch.float64, generator=g)
    c /= c.norm(dim=1, keepdim=True)
    x = c[torch.arange(N, device=dev) % P] + 0.06 * torch.randn((N, d), device=dev, dtype=torch.float64, generator=g)
    x /= x.norm(dim=1, keepdim=True)
    D = (2 - 2 * (x @ x.T)).clamp_(min=0).sqrt_()
    D.fill_diagonal_(0)
    return D.neg_()


def sweep(torch, dev):
    """one line per size and tile of the column walk, on a seeded matrix"""
    import hashlib
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    out = []
    for N in (SIZES[0], 8192, 8208, SIZES[1]):
        R = torch.randn((N, N), device=dev, dtype=torch.float64, generator=torch.Generator(device=dev).manual_seed(1))
        cs, ctrl = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(8, dtype=torch.int64, device=dev)
        cfgs = [-1] + list(range(int(L.ssg_ap_colsum_configs())))
        fns = [lambda c=c: check(L.ssg_ap_colsum_cfg_f64(ptr(R), N, ptr(cs), ptr(ctrl), c, stream()), "ssg_ap_colsum_cfg_f64") for c in cfgs]
        res = rounds(fns, CALLS, ROUNDS, WARMUP)
        for c, fn, r in zip(cfgs, fns, res):
            cs.fill_(float("nan"))
            fn()
            out.append("  N = %5d  tile %4s  " % (N, "auto" if c < 0 else c) + CELL % r + "  sums sha256 %s" % hashlib.sha256(cs.cpu().numpy().tobytes()).hexdigest()[:12])
        del R
    return out


def main():
    import numpy as np
    import torch
    from ssg_amd import _lib, hostio
    from ssg_amd._lib import check, ptr, stream
    from ssg_amd.cluster import AffinityPropagation, _AP_NOISE
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = ["affinity propagation on %s; medians of %d round medians of %d calls, (min-max of the round medians), milliseconds"
             % (torch.cuda.get_device_name(0), ROUNDS, CALLS)]
    for N in SIZES:
        X = similarities(torch, dev, N)
        # ---- noise: host generation and upload
        t0 = time.perf_counter()
        noise_h = np.random.RandomState(0).standard_normal(size=(N, N))
        t_gen = time.perf_counter() - t0
        pin = hostio.pinned_empty((N, N), torch.float64)
        t0 = time.perf_counter()
        pin.numpy()[...] = noise_h
        t_stage = time.perf_counter() - t0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        noise = pin.to(dev, non_blocking=True)
        torch.cuda.synchronize()
        t_up = time.perf_counter() - t0
        del noise_h, pin
        # ---- the loop's state after 5 iterations
        S = X.clone()
        pref = torch.empty(1, dtype=torch.float64, device=dev)
        wb = int(L.ssg_ap_median_workspace_bytes())
        ws = torch.empty(wb // 8, dtype=torch.int64, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(L.ssg_ap_median_f64(ptr(S), N * N, ptr(ws), wb, ptr(pref), stream()), "ssg_ap_median_f64")
        e1.record(); e1.synchronize()
        t_median = e0.elapsed_time(e1)
        check(L.ssg_ap_prepare_f64(ptr(S), N, ptr(pref), 1, ptr(noise), stream()), "ssg_ap_prepare_f64")
        del noise
        A, R = torch.zeros((N, N), dtype=torch.float64, device=dev), torch.zeros((N, N), dtype=torch.float64, device=dev)
        cs, E = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev)
        win, ctrl = torch.zeros((N, 15), dtype=torch.uint8, device=dev), torch.zeros(8, dtype=torch.int64, device=dev)
        check(L.ssg_ap_iterate_f64(ptr(S), ptr(A), ptr(R), ptr(cs), ptr(win), ptr(E), ptr(ctrl), N, 0.5, 15, 0, 5, stream()), "ssg_ap_iterate_f64")
        dst = torch.empty_like(S)

        def row():
            check(L.ssg_ap_row_f64(ptr(S), ptr(A), ptr(R), ptr(cs), N, 0.5, 5, 1, ptr(ctrl), stream()), "ssg_ap_row_f64")

        def col():
            check(L.ssg_ap_colsum_f64(ptr(R), N, ptr(cs), ptr(ctrl), stream()), "ssg_ap_colsum_f64")

        def copy():
            dst.copy_(S)

        r_row, r_col, r_copy = rounds([row, col, copy], CALLS, ROUNDS, WARMUP)
        assert int(ctrl[0].item()) == 0
        copy_rate = 2 * 8 * N * N / (r_copy[0] * 1e-3)
        lines.append("")
        lines.append("N = %d" % N)
        lines.append("  copy of one N x N float64 matrix   " + CELL % r_copy + "   %.2f TB/s" % (copy_rate / 1e12))
        for name, r, nmat in (("row kernel (A of t, R of t+1)     ", r_row, 6), ("column walk (ordered sums)        ", r_col, 1)):
            rate = nmat * 8 * N * N / (r[0] * 1e-3)
            lines.append("  " + name + " " + CELL % r + "   %.2f TB/s of the floor model's %d x 8 N^2 bytes = %.2f of the copy rate"
                         % (rate / 1e12, nmat, rate / copy_rate))
        lines.append("  one iteration = row + column walk + check: %.3f ms of kernels; the column walk is %.0f %% of it"
                     % (r_row[0] + r_col[0], 100 * r_col[0] / (r_row[0] + r_col[0])))
        lines.append("  exact median of the N^2 entries (10 launches): %.3f ms" % t_median)
        lines.append("  noise on the host: standard_normal %.2f s, into page-locked memory %.2f s, upload %.3f s (%.1f GB/s)"
                     % (t_gen, t_stage, t_up, 8 * N * N / t_up / 1e9))
        del A, R, S, dst, win
        # ---- whole fits
        _AP_NOISE.clear()
        est = AffinityPropagation(affinity="precomputed", random_state=0)
        fits = []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                est.fit(X)
            torch.cuda.synchronize()
            fits.append(time.perf_counter() - t0)
        lines.append("  fit (copy=True, poll_every=16): first %.2f s (noise drawn and uploaded), then %.3f s (median of 3, noise cached); "
                     "n_iter_ %d, %d clusters" % (fits[0], statistics.median(fits[1:]), est.n_iter_, len(est.cluster_centers_indices_)))
        if N == SIZES[0] and "--no-sklearn" not in sys.argv:
            try:
                from sklearn.cluster import AffinityPropagation as SkAP
            except ImportError:
                lines.append("  sklearn is not installed: no CPU time")
            else:
                Xh = X.cpu().numpy()
                t0 = time.perf_counter()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    sk = SkAP(affinity="precomputed", random_state=0).fit(Xh)
                t_sk = time.perf_counter() - t0
                same = sk.n_iter_ == est.n_iter_ and np.array_equal(sk.labels_, est.labels_)
                lines.append("  sklearn %s on the host's CPU: fit %.2f s, n_iter_ %d; labels and n_iter_ identical to the device's: %s"
                             % (__import__("sklearn").__version__, t_sk, sk.n_iter_, same))
        del X, est
        _AP_NOISE.clear()
        torch.cuda.empty_cache()
    if "--sweep" in sys.argv:
        lines += ["", "column-walk tiles (ssg_ap_colsum_cfg_f64; columns x row lanes x rows per lane: 0 16x32x4, 1 16x16x8, 2 16x32x8, 3 32x16x4; "
                  "auto: 0 up to 512 workgroups, N <= 8192, else 1):"] + sweep(torch, dev)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(ROOT, "profiles", "affinity_times.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
