#!/usr/bin/env python
"""Time the verification metrics at Market-1501 evaluation size (m = 3 368 queries, n = 15 913 gallery entries) on the MI355X and,
next to it in the same process, the `exact` numpy restatement (tests/verify_ref.py) on the host.  Writes profiles/verify_times.txt.

    python tools/time_verify.py [out.txt]

Device times are medians of 20 timed calls after 3 warm-up calls, taken with events around the call on an otherwise idle stream (the
per-pass figures include the pass's small scan / reduction launches, not the read-back).  The whole call is wall time around
find_metric_threshold(dist=device block) with stdout redirected, read-backs and printing included.  Each pass must read the
4 * m * n bytes of the block once per sweep: the achieved rate is that byte count times the number of sweeps over the median."""
import contextlib
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import verify_ref  # noqa: E402

import ssg_amd  # noqa: E402,F401
from ssg_amd import verification  # noqa: E402
from ssg_amd.evaluators import _sqdist  # noqa: E402


def device_median(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "verify_times.txt")
    m, n, d, ids = 3368, 15913, 2048, 751
    rng = np.random.default_rng(0)
    c = rng.standard_normal((ids, d)).astype(np.float32)
    rl = rng.integers(0, ids, n); ql = rng.integers(0, ids, m)
    rl[:ids] = np.arange(ids)                                     # every identity is in the gallery
    y = c[rl] + 0.9 * rng.standard_normal((n, d)).astype(np.float32); y /= np.linalg.norm(y, axis=1, keepdims=True)
    x = c[ql] + 0.9 * rng.standard_normal((m, d)).astype(np.float32); x /= np.linalg.norm(x, axis=1, keepdims=True)
    torch.cuda.set_device(0)
    block = _sqdist(torch.from_numpy(x), torch.from_numpy(y))
    torch.cuda.synchronize()
    nbytes = 4.0 * m * n
    lines = ["verification metrics, m = %d, n = %d, ld = %d (block %.1f MB), %s, torch %s" % (m, n, block.stride(0), nbytes / 1e6,
                                                                                              torch.cuda.get_device_name(0), torch.__version__)]
    blk = verification._Block(None, ql, None, rl, block)
    L, head = blk.L, blk._head()
    from ssg_amd._lib import ptr, stream
    dev = block.device
    counts = torch.empty(2, dtype=torch.int64, device=dev); sums = torch.empty(4, dtype=torch.float64, device=dev)
    mm = torch.empty(4, dtype=torch.float32, device=dev); st = torch.empty(2, dtype=torch.int32, device=dev)
    vals = torch.empty(64, dtype=torch.float32, device=dev); c3 = torch.empty((3, 64), dtype=torch.int64, device=dev); tot = torch.empty(2, dtype=torch.int64, device=dev)
    import ctypes
    with contextlib.redirect_stdout(io.StringIO()):
        res = verification.find_metric_threshold(None, ql, None, rl, dist=block)
    ranks4 = (ctypes.c_int64 * 4)(*res.num)
    ranks64 = (ctypes.c_int64 * 64)(*[int(f * res.inter_num) for f in np.logspace(-6, -0.01, 64)])
    thr10 = (ctypes.c_double * 10)(*[float(t) for t in res.thresholds])
    thr64 = (ctypes.c_double * 64)(*[float(t) for t in np.linspace(res.intra_min, res.inter_max, 64)])
    passes = [
        ("pass A  statistics", 1, lambda: L.ssg_verify_stats_f32(*head, ptr(blk.ws), blk.ws_bytes, ptr(counts), ptr(sums), ptr(mm), ptr(st), stream())),
        ("pass B  4 ranks (FAR 1e-2 .. 1e-5)", 4, lambda: L.ssg_verify_select_f32(*head, ranks4, 4, ptr(blk.ws), blk.ws_bytes, ptr(vals), ptr(st), stream())),
        ("pass B  64 ranks over the whole range", 4, lambda: L.ssg_verify_select_f32(*head, ranks64, 64, ptr(blk.ws), blk.ws_bytes, ptr(vals), ptr(st), stream())),
        ("pass C  10 thresholds", 1, lambda: L.ssg_verify_count_f32(*head, 1, thr10, 10, ptr(blk.ws), blk.ws_bytes, ptr(c3), ptr(tot), stream())),
        ("pass C  64 thresholds", 1, lambda: L.ssg_verify_count_f32(*head, 1, thr64, 64, ptr(blk.ws), blk.ws_bytes, ptr(c3), ptr(tot), stream())),
    ]
    for name, sweeps, fn in passes:
        assert fn() == 0
        med, lo, hi = device_median(fn)
        lines.append("%-40s median %8.3f ms  (min %.3f, max %.3f)  %d sweep(s) of the block  %7.1f GB/s" % (name, med, lo, hi, sweeps, sweeps * nbytes / med / 1e6))
    ws = []
    for _ in range(13):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            verification.find_metric_threshold(None, ql, None, rl, dist=block)
        ws.append((time.perf_counter() - t0) * 1e3)
    ws = ws[3:]
    lines.append("%-40s median %8.3f ms  (min %.3f, max %.3f)  wall, A + C(10) + B(4) + C(4), read-backs and printing included"
                 % ("find_metric_threshold(dist=device block)", statistics.median(ws), min(ws), max(ws)))
    host = block.cpu().numpy()
    hs = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref = verify_ref.find_metric_threshold(ql, rl, host, mode="exact")
        hs.append(time.perf_counter() - t0)
        if hs[-1] > 40:
            break
    lines.append("%-40s median %8.3f s   (%d run(s): %s)  numpy %s, block already in host memory" % ("host restatement, exact mode", statistics.median(hs), len(hs),
                                                                                                  ", ".join("%.2f" % t for t in hs), np.__version__))
    same = (ref["lines"] == res.lines)
    lines.append("printed lines of the device call and of the host restatement are %s" % ("identical" if same else "DIFFERENT"))
    lines += ["  " + ln for ln in res.lines if ln]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
