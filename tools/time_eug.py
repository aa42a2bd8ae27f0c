#!/usr/bin/env python3
"""SSG++ label step (ssg_amd.eug) at Market-1501 scale (Nu = 12 185 unlabelled, Nl = 751 labelled): GPU time of every stage between
HIP events, median of R calls after one warm-up, for d = 2048 (num_split = 0) and 6144 (num_split = 2).  One JSON line per width.

Stages: (a) exact nearest labelled neighbour (ssg_eug_nn_f32, rerank=False); (rr) re_ranking_init on the device (cosine Gram +
sparse stages, [Nu+Nl]^2); (b) row argmin + column max + confidence on the [Nu, Nl] result (ssg_eug_dist_label_f32); (c) top-k
mask over Nu float64 scores (ssg_eug_select_top; also at 128 000).  The floor of (a) is the VALU bound of its exact order:
sub + mul + add per element, no FMA, at 32 single-op lanes/clk/SIMD (= 64 FLOP/clk/SIMD counting an FMA as two), 2.4 GHz."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ssg_amd  # noqa: E402,F401
from ssg_amd import _lib  # noqa: E402
from ssg_amd._lib import check, ptr, stream  # noqa: E402
from ssg_amd.rerank import re_ranking_init_device  # noqa: E402

R = int(os.environ.get("R", 5))
NU, NL = 12185, 751


def timed(fn, r=R):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(r):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return round(statistics.median(ts), 4)


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = _lib.lib()
    for d in (2048, 6144):
        gen = torch.Generator(device=dev).manual_seed(d)
        c = torch.nn.functional.normalize(torch.randn(NL, d, device=dev, generator=gen), dim=1)
        pid = torch.randint(0, NL, (NU,), device=dev, generator=gen)
        u = torch.nn.functional.normalize(c[pid] + 0.6 * torch.randn(NU, d, device=dev, generator=gen) / d ** 0.5, dim=1)
        lf = torch.nn.functional.normalize(c + 0.6 * torch.randn(NL, d, device=dev, generator=gen) / d ** 0.5, dim=1)
        lab = torch.arange(NL, device=dev, dtype=torch.int64)
        ns = int(L.ssg_eug_nn_splits(NU, NL))
        pv = torch.empty(ns * NU, device=dev); pi = torch.empty(ns * NU, device=dev, dtype=torch.int32)
        am = torch.empty(NU, device=dev, dtype=torch.int32); mv = torch.empty(NU, device=dev)
        lo = torch.empty(NU, device=dev, dtype=torch.int64); sc = torch.empty(NU, device=dev, dtype=torch.float64)
        conf = torch.empty(NU, device=dev, dtype=torch.float64); ws = torch.empty(65 * NL, device=dev)
        mask = torch.empty(128000, device=dev, dtype=torch.uint8)
        big = torch.rand(128000, device=dev, dtype=torch.float64)

        def a():
            check(L.ssg_eug_nn_f32(ptr(u), NU, ptr(lf), NL, d, ptr(lab), ns, ptr(pv), ptr(pi), ptr(am), ptr(mv), ptr(lo), ptr(sc), stream()), "nn")
        D = re_ranking_init_device(u, lf)

        def b():
            check(L.ssg_eug_dist_label_f32(ptr(D), NU, NL, ptr(lab), ptr(ws), ptr(am), ptr(lo), ptr(sc), ptr(conf), stream()), "b")

        def c_nu():
            check(L.ssg_eug_select_top(ptr(sc), NU, NU // 3, None, ptr(mask), stream()), "c")

        def c_big():
            check(L.ssg_eug_select_top(ptr(big), 128000, 40000, None, ptr(mask), stream()), "c")
        elems = NU * NL * d
        floor_a = 3.0 * elems / (256 * 4 * 32 * 2.4e9) * 1e3
        res = {"d": d, "Nu": NU, "Nl": NL, "nn_splits": ns,
               "a_nearest_ms": timed(a), "a_floor_ms_estimated": round(floor_a, 3),
               "rerank_init_ms": timed(lambda: re_ranking_init_device(u, lf), r=3),
               "b_dist_label_ms": timed(b), "c_select_top_nu_ms": timed(c_nu), "c_select_top_128k_ms": timed(c_big)}
        res["a_fraction_of_floor"] = round(floor_a / res["a_nearest_ms"], 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
