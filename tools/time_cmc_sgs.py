"""Times the single-gallery-shot CMC protocol (ssg_amd.ranking.cmc(..., single_gallery_shot=True, rng=...), csrc/cmc_sgs.hip) and writes
profiles/cmc_sgs_times.txt:

    python tools/time_cmc_sgs.py                          the device section: the whole call and its stages (without a GPU: "not yet timed")
    python tools/time_cmc_sgs.py --reference /path/to/ref the reference section: the reference's own loop on this host's CPU
    (--out FILE writes there instead)

Two synthetic blocks: 1 400 x 5 332 with 700 identities on 2 cameras (CUHK03's new protocol) and 3 368 x 15 913 with 751 identities on 6
cameras, one of them a distractor identity of 2 798 entries (Market-sized).  Both are scored with the 'cuhk03' settings
(separate_camera_set=True).  The reference runs the smaller block whole and the first REF_SUBSET queries of the larger one, scaled to all
of them and marked as such.  Each section carries the sha256 of its curve for the smaller block, so that the two can be compared even
when they were written on different hosts; the section that is not being written is kept as it stands."""
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "cmc_sgs_times.txt")
SIZES = [("CUHK03-sized", 1400, 5332, 700, 2, 0), ("Market-sized", 3368, 15913, 751, 6, 2798)]
REF_SUBSET = 60
STREAM = 20260
MARK = {"device": "== device ==", "reference": "== reference loop =="}


def block(m, n, G, ncam, distractors, seed=5):
    """-> dist float32 [m, n], qid, gid, qcam, gcam: every identity at least once in the gallery, true matches nearer on average"""
    rs = np.random.RandomState(seed)
    lo = 1 if distractors else 0                       # identity 0 is the distractor identity when there is one
    gid = np.concatenate([np.zeros(distractors, np.int64), np.arange(lo, G), rs.randint(lo, G, n - distractors - (G - lo))])
    gid = gid[rs.permutation(n)]
    gcam = rs.randint(0, ncam, n)
    qid = rs.randint(lo, G, m); qcam = rs.randint(0, ncam, m)
    dist = rs.random_sample((m, n)).astype(np.float32)
    dist[gid[None, :] == qid[:, None]] -= np.float32(0.4)
    # ranks instead of the values: no two entries of a row are equal (the reference's argsort leaves the order of ties open)
    dist = (np.argsort(np.argsort(dist, axis=1, kind="stable"), axis=1) / np.float32(64)).astype(np.float32)
    return dist, qid, gid, qcam, gcam


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]


def device_section():
    import torch
    if not torch.cuda.is_available():
        return ["not yet timed"]
    from ssg_amd import ranking
    lines = ["single-gallery-shot CMC on %s; seconds, median (min-max) over the runs after one warm-up call; stages timed with a device "
             "synchronise around each, the whole call without" % torch.cuda.get_device_name(0)]
    for name, m, n, G, ncam, distractors in SIZES:
        dist, qid, gid, qcam, gcam = block(m, n, G, ncam, distractors)
        d = torch.from_numpy(dist).cuda()
        runs = 5 if m * n < 2e7 else 3

        def call():
            return ranking.cmc(d, qid, gid, qcam, gcam, separate_camera_set=True, single_gallery_shot=True, rng=STREAM)
        t0 = time.perf_counter()
        curve = call()
        print("%s: first call %.2f s" % (name, time.perf_counter() - t0), file=sys.stderr, flush=True)
        whole = []
        for _ in range(runs):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            assert np.array_equal(call(), curve)
            whole.append(time.perf_counter() - t0)
        stages = {}
        for _ in range(runs):
            ranking.single_shot_ranks.stage_times = acc = {}
            try:
                call()
            finally:
                ranking.single_shot_ranks.stage_times = None
            for k, v in acc.items():
                stages.setdefault(k, []).append(v)
        cell = lambda v: "%8.4f (%.4f-%.4f)" % (statistics.median(v), min(v), max(v))       # noqa: E731
        med = {k: statistics.median(v) for k, v in stages.items()}
        total = sum(med.values())
        lines += ["", "%s: %d x %d, %d identities, %d cameras; %d words consumed, %d runs" % (name, m, n, G, ncam, ranking.single_shot_ranks.last_consumed, runs),
                  "  whole call (distance block on the device)   %s" % cell(whole)]
        for k, what in (("groups", "groups stage (one workgroup per query)"), ("words", "words drawn on the host and uploaded"),
                        ("draws", "draws stage (one wave, serial) + read-back"), ("counts", "counts stage (query x repeat)"),
                        ("commit", "stream advanced on the host")):
            lines.append("  %-44s %s" % (what, cell(stages[k])))
        lines.append("  the serial draws stage is %.0f %% of the staged call (%.4f of %.4f s)" % (100 * med["draws"] / total, med["draws"], total))
        lines.append("  top-1 %.4f top-5 %.4f; curve sha256 %s" % (curve[0], curve[4], sha(curve)))
    return lines


def reference_section(ref_root):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_golden_cmc_sgs import load_reference
    mod = load_reference(ref_root)
    lines = ["the reference's cmc(single_gallery_shot=True, separate_camera_set=True) on this host's CPU (%d cores, one used), numpy %s; "
             "seconds, one run each.  The reference is not installed where the GPU is, so this section and the device section may come from "
             "two hosts; the curve digests of the smaller block tie them together" % (os.cpu_count(), np.__version__)]
    for name, m, n, G, ncam, distractors in SIZES:
        dist, qid, gid, qcam, gcam = block(m, n, G, ncam, distractors)
        sub = m if m * n < 2e7 else REF_SUBSET
        np.random.seed(STREAM)
        t0 = time.perf_counter()
        curve = mod.cmc(dist[:sub], qid[:sub], gid, qcam[:sub], gcam, separate_camera_set=True, single_gallery_shot=True)
        t = time.perf_counter() - t0
        if sub == m:
            lines += ["", "%s: %d x %d: whole call %.1f s; curve sha256 %s" % (name, m, n, t, sha(curve))]
        else:
            lines += ["", "%s: %d x %d: the first %d queries took %.1f s; SCALED to %d queries: %.0f s (not measured whole)" % (name, m, n, sub, t, m, t * m / sub)]
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
