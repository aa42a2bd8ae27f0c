"""Times KISSME.fit / transform (ssg_amd/metric_learning.py, csrc/kissme.hip) and writes profiles/kissme_times.txt:

    python tools/time_kissme.py                          the device section (without a GPU: "not yet timed")
    python tools/time_kissme.py --reference /path/to/ref the reference section: the reference's own fit on this host's CPU
    (--out FILE writes there instead)

Market-1501-sized: n = 12 936 rows in 751 ragged identities (3 to 60 rows), features = class centre + unit noise, d = 2048 and d = 512.
Device stages are timed one call at a time with events, as medians of round medians with their min-max spread; the host stages (the draw
of the non-matching positions, the d x d factorisation) with the host clock.  The covariance launches are also given as a share of the FP64
matrix peak (78.6 TFLOP/s): executed = the 128 x 128 tiles on or above the diagonal, useful = 2 d^2 P.  The section that is not being
written is kept as it stands."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "kissme_times.txt")
N, IDS, DIMS, ROWS_T = 12936, 751, (2048, 512), 19281
PEAK_FP64_MFMA_TF = 78.6
MARK = {"device": "== device ==", "reference": "== reference fit =="}
REF_ROWS = (12936, 6000, 3000)                                # tried in this order: the first that fits in memory is reported


def data(n, ids, d, seed=9):
    """-> X float32 [n, d], y float32 [n]: ragged identities (3 .. 60 rows), centre (spread 2) + unit noise, shuffled"""
    rs = np.random.RandomState(seed)
    sizes = np.full(ids, 3)
    extra = n - sizes.sum()
    while extra > 0:                                            # ragged: hand the rest out in random lumps, at most 60 rows per identity
        i = rs.randint(ids); k = min(int(rs.randint(1, 40)), 60 - sizes[i], extra)
        sizes[i] += k; extra -= k
    cls = np.repeat(np.arange(ids), sizes)[rs.permutation(n)]
    X = (2.0 * rs.standard_normal((ids, d)).astype(np.float32))[cls] + rs.standard_normal((n, d)).astype(np.float32)
    return X, cls.astype(np.float32)


def host_clock(fn, runs):
    t = []
    for _ in range(runs):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return "%9.4f (%.4f-%.4f)" % (statistics.median(t), min(t), max(t))


def device_section():
    import torch
    if not torch.cuda.is_available():
        return ["not yet timed"]
    import _timing
    from ssg_amd import metric_learning as ml
    lines = ["KISSME on %s: n = %d rows, %d ragged identities.  Device stages: milliseconds, median (min-max) of 5 round medians of 3 calls after "
             "2 warm-up calls; host stages: seconds on this host's CPU, median (min-max) over the runs" % (torch.cuda.get_device_name(0), N, IDS)]
    for d in DIMS:
        X, y = data(N, IDS, d)
        Xd = ml._padded(X, torch.device("cuda"), 16)
        ix = ml.pair_index(y)
        tot = ix["scans"][:, N].cpu()
        P, NN = int(tot[0]), int(tot[1])
        rs = np.random.RandomState(1)
        p = rs.choice(NN, P, replace=False)
        pd = torch.from_numpy(p).cuda()
        ia1, ib1 = ml.match_pairs(ix, P); ia0, ib0 = ml.unrank(ix, pd)
        res = _timing.rounds([lambda: ml.pair_index(y), lambda: ml.match_pairs(ix, P), lambda: ml.unrank(ix, pd),
                              lambda: ml.pairdiff_cov(Xd, ia1, ib1, P), lambda: ml.pairdiff_cov(Xd, ia0, ib0, P)], 3, 5, 2)
        T = (d + 127) // 128
        executed, useful = 2.0 * P * 128 * 128 * T * (T + 1) / 2, 2.0 * P * d * d
        lines += ["", "d = %d: %d matching pairs, %d non-matching pairs to draw from" % (d, P, NN)]
        for what, r in zip(("ssg_kissme_index (with np.unique and the upload of the ids)", "ssg_kissme_match_pairs", "ssg_kissme_unrank",
                            "ssg_pairdiff_cov_f64, C1 (matching pairs: rows of one class)", "ssg_pairdiff_cov_f64, C0 (sampled pairs)"), res):
            lines.append("  %-62s %s ms" % (what, _timing.CELL % r))
        for what, r in zip(("C1", "C0"), res[3:]):
            lines.append("  %s: %.3f TFLOP executed -> %.1f TFLOP/s = %.1f %% of the FP64 matrix peak; useful 2 d^2 P = %.3f TFLOP -> %.1f TFLOP/s"
                         % (what, executed / 1e12, executed / r[0] / 1e9, 100 * executed / r[0] / 1e9 / PEAK_FP64_MFMA_TF, useful / 1e12, useful / r[0] / 1e9))
        lines.append("  %-62s %s s" % ("host: RandomState.choice(%d, %d, replace=False)" % (NN, P), host_clock(lambda: rs.choice(NN, P, replace=False), 3)))
        C = torch.stack([ml.pairdiff_cov(Xd, ia1, ib1, P), ml.pairdiff_cov(Xd, ia0, ib0, P)]).cpu().numpy()
        eig, calls = np.linalg.eig, [0]

        def counting(*a, **k):
            calls[0] += 1
            return eig(*a, **k)
        k = ml.KISSME()

        def factor():
            np.linalg.eig = counting
            try:
                k.M_ = ml.validate_cov_matrix(np.linalg.inv(C[0]) - np.linalg.inv(C[1]))
                k.transformer()
            finally:
                np.linalg.eig = eig
        lines.append("  %-62s %s s" % ("host: inv, inv, validate_cov_matrix, cholesky (one run)", host_clock(factor, 1)))
        lines.append("    (the validate loop took %d eigendecompositions of the %d x %d matrix)" % (calls[0], d, d))
        Q = torch.randn(ROWS_T, d, device="cuda")
        r = _timing.rounds([lambda: k.transform(Q)], 3, 5, 2)[0]
        lines.append("  %-62s %s ms" % ("transform of %d rows (tensor on the device, ssg_linear_fwd_f32)" % ROWS_T, _timing.CELL % r))
        if d == min(DIMS):                                      # (at d = 2048 the factorisation above is the whole call but for a second)
            t0 = time.perf_counter(); ml.KISSME().fit(Xd[:, :d], y, rng=1); whole = time.perf_counter() - t0
            lines.append("  %-62s %9.2f s (one run)" % ("KISSME.fit, whole call", whole))
        print("d = %d done" % d, file=sys.stderr, flush=True)
    return lines


def reference_section(ref_root):
    from make_golden_kissme import load_reference
    mod = load_reference(ref_root)
    lines = ["the reference's KISSME.fit on this host's CPU (%d cores), numpy %s; seconds, one run.  The reference is not installed where the GPU "
             "is, so this section and the device section may come from two hosts" % (os.cpu_count(), np.__version__)]
    for d in sorted(DIMS):
        for n in REF_ROWS:
            X, y = data(n, max(2, IDS * n // N), d)
            np.random.seed(1)
            t0 = time.perf_counter()
            try:
                mod.KISSME().fit(X, y)
            except MemoryError:
                lines += ["", "n = %d, d = %d: MemoryError (two n x n int64 meshgrids and their masks)" % (n, d)]
                continue
            lines += ["", "n = %d, %d identities, d = %d: fit %.1f s" % (n, max(2, IDS * n // N), d, time.perf_counter() - t0)]
            print(lines[-1], file=sys.stderr, flush=True)
            break
    return lines


def main():
    which = "reference" if "--reference" in sys.argv else "device"
    new = reference_section(sys.argv[sys.argv.index("--reference") + 1]) if which == "reference" else device_section()
    kept = {"device": ["not yet timed"], "reference": ["not yet timed"]}
    if os.path.exists(OUT):
        cur = None
        for line in open(OUT).read().split("\n"):
            if line in MARK.values():
                cur = [k for k, v in MARK.items() if v == line][0]; kept[cur] = []
            elif cur:
                kept[cur].append(line)
    kept[which] = new
    with open(OUT, "w") as f:
        for k in ("device", "reference"):
            f.write(MARK[k] + "\n" + "\n".join(kept[k]).strip("\n") + "\n\n")
    print(open(OUT).read())


if __name__ == "__main__":
    main()
