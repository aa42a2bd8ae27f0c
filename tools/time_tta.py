"""Times the test-time extraction (ssg_amd/extract_feature.py, csrc/tta.hip) and writes profiles/tta_times.txt (--out FILE: there):

  1. ten_crop_batch on 64 Market-sized images (128 x 64 -> 288 x 144 -> ten 256 x 128 crops) against preprocess_batch(288, 144) + ten
     torch slices / flips + stack
  2. the extraction of one 64-image batch with test-time augmentation: five crops + the stem's flip on two streams against the ten
     materialised crops in one forward (resnet50, seeded weights)
  3. multi_query_pool at Market-1501's size, 25 259 gt_bbox rows x 2048 and 3 368 queries, against the script's loop (a dict of lists,
     sklearn normalize, np.max / np.mean per query) on this host's CPU

Device calls are timed one at a time with events and given as the median (min-max) of round medians, the two sides of a comparison
in turn within every round (tools/_timing.py); a side wins when its median is lower by more than the larger spread.  Needs a GPU."""
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "tta_times.txt")
B, M, Q, D = 64, 25259, 3368, 2048
KEEP = "== figures printed by tests/test_gpu_tta.py (pytest -s) =="


def market_names(rng):
    """gt_bbox-like names: 1501 identities x up to 6 cameras, ragged; queries: one file per (identity, camera) pair met, 3 368 of them"""
    keys = ["%04d_c%d" % (i + 1, c + 1) for i in range(1501) for c in range(6)]
    keys = [keys[i] for i in rng.permutation(len(keys))[:Q]]
    member = np.concatenate([np.arange(Q), rng.integers(0, Q, M - Q)])
    member = member[rng.permutation(M)]
    rows = ["%ss1_%06d_00.jpg" % (keys[g], i) for i, g in enumerate(member)]
    queries = ["%ss1_000000_00.jpg" % k for k in keys]
    return rows, queries


def script_loop(x, rows, queries):
    from sklearn.preprocessing import normalize
    d = {}
    for f, r in zip(rows, x):
        d.setdefault(f[:7], []).append(r)
    hmax, havg = [], []
    for q in queries:
        multi = normalize(d[q[:7]])
        hmax.append(np.max(multi, axis=0)); havg.append(np.mean(multi, axis=0))
    return np.array(hmax), np.array(havg)


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_tta.py measures on the GPU; none is visible")
    import _timing
    import ssg_amd
    from ssg_amd import extract_feature as xf
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    lines = ["Test-time extraction on %s.  Milliseconds, median (min-max) of 5 round medians of 3 calls after 2 warm-up calls, the sides of a "
             "comparison in turn within each round." % torch.cuda.get_device_name(0), ""]

    # 1. the crops
    src = torch.from_numpy(rng.integers(0, 255, (B, 128, 64, 3), dtype=np.uint8)).to(dev)
    boxes = xf.crop_table((288, 144), (256, 128))

    def torch_crops():
        r = ssg_amd.preprocess_batch(src, 288, 144)
        f = r.flip(-1)
        return torch.stack([im[:, :, t:t + 256, l:l + 128] for im in (r, f) for t, l in boxes], dim=1)

    assert torch.equal(torch_crops(), xf.ten_crop_batch(src))
    a, b, c = _timing.rounds([lambda: xf.ten_crop_batch(src), torch_crops, lambda: xf.ten_crop_batch(src, ncrops=5)], 3, 5, 2)
    out_mb = B * 10 * 3 * 256 * 128 * 4 / 1e6
    lines += ["1. ten crops of %d images of 128 x 64 (%.0f MB written; equal bit for bit)" % (B, out_mb),
              "   ten_crop_batch (ssg_tencrop_u8)                              %s ms  = %.0f GB/s written" % (_timing.CELL % a, out_mb / a[0]),
              "   preprocess_batch(288, 144) + 10 slices / flips + stack       %s ms" % (_timing.CELL % b),
              "   ten_crop_batch(ncrops=5), what the five-crop route makes     %s ms" % (_timing.CELL % c),
              "   -> %s" % _timing.verdict(a, b, "the kernel is faster", "the torch composition is faster"), ""]

    # 2. the two extraction routes
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = ssg_amd.create("resnet50", dropout=0.0, num_features=2048, num_classes=632, seed=1).cuda().eval()
    names = ["%04d_c1s1_%06d_00.jpg" % (i + 1, i) for i in range(B)]

    def fused():
        return xf.extract_feature_matrix(m, [(xf.FiveCrops(xf.ten_crop_batch(src, ncrops=5)), names)], print_freq=0, tta=True)[0]

    def literal():
        return xf.extract_feature_matrix(m, [(xf.ten_crop_batch(src), names)], print_freq=0, tta=True)[0]

    def plain():
        return xf.extract_feature_matrix(m, [(ssg_amd.preprocess_batch(src, 256, 128), names)], print_freq=0)[0]

    diff = float((fused() - literal()).abs().max())
    a, b, c = _timing.rounds([fused, literal, plain], 3, 5, 2)
    lines += ["2. one batch of %d images through resnet50 with test-time augmentation (transform + %d forwards + mean; the range flag read once)" % (B, 10 * B),
              "   five crops + stem flip, two streams                          %s ms" % (_timing.CELL % a),
              "   ten materialised crops, one forward                          %s ms" % (_timing.CELL % b),
              "   no augmentation (Resize((256, 128)), %d forwards)             %s ms" % (B, _timing.CELL % c),
              "   largest |five-crop route - ten-crop route| over the %d x 2048 features: %.3g%s" % (B, diff, " (bit-identical)" if diff == 0.0 else ""),
              "   augmentation costs %.1f x a plain extraction" % (min(a[0], b[0]) / c[0]),
              "   -> %s" % _timing.verdict(a, b, "the five-crop route is faster: it is the default for the ResNet family",
                                           "the ten-crop route is faster: TestBatchLoader(tta='literal') is the one to use",
                                           "no difference beyond the spread: the five-crop route stays the default for the ResNet family (half the crop memory)"), ""]

    # 3. multi-query pooling
    rows, queries = market_names(rng)
    x = (rng.standard_normal((M, D)) * rng.uniform(0.5, 2.0, (M, 1))).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    order, offs, qgroup = xf.group_index(rows, queries)
    t0 = time.perf_counter(); xf.group_index(rows, queries); t_index = time.perf_counter() - t0
    (a,) = _timing.rounds([lambda: xf.multi_query_pool(xd, rows, queries)], 3, 5, 2)
    host = []
    for _ in range(3):
        t0 = time.perf_counter(); rmax, ravg = script_loop(x, rows, queries); host.append(time.perf_counter() - t0)
    hmax, havg = xf.multi_query_pool(xd, rows, queries)
    dmax = float(np.abs(hmax.cpu().numpy() - rmax).max()); davg = float(np.abs(havg.cpu().numpy() - ravg).max())
    sizes = np.diff(offs)
    lines += ["3. multi_query_pool: %d rows x %d in %d groups of %d..%d rows, %d queries" % (M, D, len(sizes), sizes.min(), sizes.max(), Q),
              "   multi_query_pool, rows on the device (host index build included)  %s ms" % (_timing.CELL % a),
              "     of which the host index build (group_index)                    %9.4f ms" % (1e3 * t_index),
              "   the script's loop on this host (%d cores visible), numpy %s        %9.1f (%.1f-%.1f) ms, 3 runs"
              % (os.cpu_count(), np.__version__, 1e3 * statistics.median(host), 1e3 * min(host), 1e3 * max(host)),
              "   (the script's list of rows makes scikit-learn compute in float64: results %s; largest |device - script|: Hist_max %.3g, Hist_avg %.3g)"
              % (rmax.dtype, dmax, davg), ""]
    kept = ""                                   # the section the tests' printed figures were copied into stays as it stands
    if os.path.exists(OUT) and KEEP in open(OUT).read():
        kept = KEEP + open(OUT).read().split(KEEP, 1)[1]
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n" + kept)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
