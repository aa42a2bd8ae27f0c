#!/usr/bin/env python3
"""Stage times of the Hausdorff re-ranking variant (ssg_amd.rerank_hausdorff, csrc/hausdorff.hip) -> profiles/hausdorff_times.txt.

Track G inputs at N = 2 000 and N = 16 000, Ns = min(N, 12 936), d = 2048, k = 20.  Every stage is timed with device
events around the call, median over repeated calls after a warm-up call.  Beside the times: float64 subtract-multiply-add triples per
second of the two distance passes against the vector float64 rate (3 operations per triple; 78.6 TFLOP/s counts a fused multiply-add
as two, so separately rounded operations can reach half of it: 39.3 T operations/s), and the bytes of the Hausdorff rows per second.
The reference's own time is measured where that is feasible (N <= 200, needs scipy and the reference tree, --reference PATH) and
extrapolated from its cost per pair, labelled as such, beyond.

Usage: python tools/time_hausdorff.py [--sizes 2000,16000] [--reps 5] [--reference /path/to/reference] [--out profiles/hausdorff_times.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
F64_OPS_PEAK = 39.3e12     # separately rounded vector float64 operations per second (half of the 78.6 TFLOP/s fma figure)


def timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()                      # warm-up
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def device_stages(N, d, k, reps, lines):
    import torch
    from synth import clustered
    from ssg_amd import _lib, rerank_hausdorff as rh
    from ssg_amd._lib import check, ptr
    L = _lib.lib()
    Ns = min(N, 12936)
    tgt, src = torch.from_numpy(clustered(N, d, seed=1)).cuda(), torch.from_numpy(clustered(Ns, d, seed=2)).cuda()
    stages = {}
    whole = timed(lambda: rh.re_ranking_hausdorff_device(src, tgt, k=k), max(1, reps // 2))
    rh.re_ranking_hausdorff_device(src, tgt, k=k, stages=stages)
    a_idx, a_nnz, cap = stages["a_idx"], stages["a_nnz"], stages["a_idx"].shape[1]
    st = _lib.stream()
    rowmin = torch.empty(N, dtype=torch.float64, device="cuda"); vec = torch.empty_like(rowmin); status = torch.zeros(2, dtype=torch.float64, device="cuda")
    E = torch.empty((N, N), dtype=torch.float64, device="cuda"); H = torch.empty_like(E)
    nws = int(L.ssg_hausdorff_workspace_bytes(N, N)); ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    t_src = timed(lambda: check(L.ssg_seqdist_rowmin_f64(ptr(tgt), N, ptr(src), Ns, d, ptr(rowmin), st)), reps)
    t_fin = timed(lambda: check(L.ssg_hausdorff_source_finish(ptr(rowmin), N, ptr(vec), ptr(status[0:1]), st)), reps)
    t_self = timed(lambda: check(L.ssg_seqdist_self_f64(ptr(tgt), N, d, 1, ptr(E), N, st)), reps)
    t_dir = timed(lambda: check(L.ssg_hausdorff_directed_rows(ptr(E), ptr(a_idx), ptr(a_nnz), cap, N, 0, N, ptr(H), ptr(ws), nws, st)), reps)
    t_sym = timed(lambda: check(L.ssg_hausdorff_symmetrize(ptr(H), N, ptr(status[1:2]), st)), reps)
    t_bl = timed(lambda: check(L.ssg_hausdorff_blend(ptr(H), ptr(status[1:2]), ptr(vec), N, 0, N, 0.9, 0.1, ptr(H), st)), reps)
    members = int(a_nnz.sum().item())
    tri_src, tri_self = N * Ns * d, (N * (N + 64) // 2) * d
    panel = 8 * members * N                       # rows E[S_i, :] read for the column minima
    gathers = 8 * members * N                     # N rows x sum |S_j| gathers out of the cached minima row
    lines.append("N = %d, Ns = %d, d = %d, k = %d (set members: %d, %.1f per row); median of %d calls after a warm-up" % (N, Ns, d, k, members, members / N, reps))
    lines.append("  whole re_ranking_hausdorff_device (with the half matrix, ranking and sets)   %10.2f ms" % whole)
    lines.append("  source distance pass, row minima (ssg_seqdist_rowmin_f64)                   %10.2f ms   %.2f T triples/s = %.1f %% of the vector float64 rate"
                 % (t_src, tri_src / t_src / 1e9, 100 * 3 * tri_src / (t_src * 1e-3) / F64_OPS_PEAK))
    lines.append("  source vector finish (ssg_hausdorff_source_finish)                          %10.3f ms" % t_fin)
    lines.append("  target distance pass, upper tiles + mirror (ssg_seqdist_self_f64)           %10.2f ms   %.2f T triples/s = %.1f %% of the vector float64 rate"
                 % (t_self, tri_self / t_self / 1e9, 100 * 3 * tri_self / (t_self * 1e-3) / F64_OPS_PEAK))
    lines.append("  directed rows (ssg_hausdorff_directed_rows)                                 %10.2f ms   panel reads %.2f GB + gathers %.2f GB + %.2f GB written: %.2f TB/s"
                 % (t_dir, panel / 1e9, gathers / 1e9, 8 * N * N / 1e9, (panel + gathers + 8 * N * N) / (t_dir * 1e-3) / 1e12))
    lines.append("  symmetric maximum + global max (ssg_hausdorff_symmetrize)                   %10.2f ms   %.2f TB/s" % (t_sym, 16 * N * N / (t_sym * 1e-3) / 1e12))
    lines.append("  blend in place (ssg_hausdorff_blend)                                        %10.2f ms   %.2f TB/s" % (t_bl, 16 * N * N / (t_bl * 1e-3) / 1e12))
    return whole


def reference_time(ref_root, lines, sizes):
    import importlib.util
    from synth import clustered
    spec = importlib.util.spec_from_file_location("ref_rerank_hausdorff", os.path.join(ref_root, "reid", "rerank_hausdorff.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m); m.print = lambda *a, **k: None
    N, Ns, d, k = 160, 64, 256, 20
    t0 = time.time(); m.re_ranking(clustered(Ns, d, seed=2), clustered(N, d, seed=1), k=k); dt = time.time() - t0
    per_pair = dt / (N * (N - 1) / 2)
    lines.append("reference on the CPU (scipy directed_hausdorff in a Python double loop), MEASURED: N = %d, Ns = %d, d = %d, k = %d: %.2f s = %.3f ms per pair"
                 % (N, Ns, d, k, dt, per_pair * 1e3))
    for n in sizes:
        lines.append("  EXTRAPOLATED from that cost per pair (not measured; d = %d, a wider feature costs more): N = %d -> %.0f s (%.1f h)"
                     % (d, n, per_pair * n * (n - 1) / 2, per_pair * n * (n - 1) / 2 / 3600))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,16000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hausdorff_times.txt"))
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    lines = ["Hausdorff re-ranking variant: stage times (tools/time_hausdorff.py)", ""]
    if a.reference:
        reference_time(a.reference, lines, sizes)
        lines.append("")
    import torch
    if torch.cuda.is_available():
        lines.insert(1, "device: %s" % torch.cuda.get_device_name(0))
        for n in sizes:
            device_stages(n, 2048, 20, a.reps, lines)
            lines.append("")
            torch.cuda.empty_cache()
    else:
        lines.append("(no GPU in this run: device stages not measured)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
