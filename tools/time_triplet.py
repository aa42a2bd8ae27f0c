#!/usr/bin/env python3
"""Per-call time of the fine-tune phase's TripletLoss, forward + backward, at the trainer's batch (n = 128, num_instances = 4),
d in {128, 2048}, both mining branches, for three variants:
  (a) the reference's loss (reid/loss/triplet.py:19-77) run by torch on the GPU;
  (b) the product before the device loss: ssg_amd.triplet.pairwise_dist for lines :28-31, the reference's loop for the rest;
  (c) ssg_amd.triplet.TripletLoss.
Device events around `iters` calls after `warmup` calls; the median of `reps` such runs.

--calls N --variant V --d D --mode M: run just N calls of one variant (inputs built on the host and copied, so that a
`rocprofv3 --kernel-trace --stats` run of it counts only the loss's own dispatches: total / N = launches per call)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from ssg_amd import triplet  # noqa: E402


def ref_dist(x):
    n = x.size(0)
    dist = torch.pow(x, 2).sum(dim=1, keepdim=True).expand(n, n)
    dist = dist + dist.t()
    dist = dist.addmm(x, x.t(), beta=1, alpha=-2)
    return dist.clamp(min=1e-12).sqrt()


def ref_rest(dist, targets, K, margin, semi):
    """reid/loss/triplet.py:32-77 (w is None)"""
    n = dist.size(0)
    mask = targets.expand(n, n).eq(targets.expand(n, n).t())
    dist_ap, dist_an = [], []
    if semi:
        for i in range(n // K):
            for j in range(K):
                neg_examples = dist[i * K + j][mask[i * K + j] == 0]
                for pair in range(j + 1, K):
                    dist_ap.append(dist[i * K + j][i * K + pair].view(1))
                    dist_an.append(neg_examples.min().view(1))
    else:
        for i in range(n):
            dist_ap.append(dist[i][mask[i]].max().view(1))
            dist_an.append(dist[i][mask[i] == 0].min().view(1))
    dist_ap, dist_an = torch.cat(dist_ap), torch.cat(dist_an)
    loss = torch.nn.functional.margin_ranking_loss(dist_an, dist_ap, torch.ones_like(dist_an), margin=margin)
    prec = (dist_an.data > dist_ap.data).sum() * 1. / dist_an.size(0)
    return loss, prec


def make_call(variant, K, margin, semi):
    crit = triplet.TripletLoss(margin=margin, num_instances=K, use_semi=semi)

    def call(x, t):
        if variant == "a":
            loss, _ = ref_rest(ref_dist(x), t, K, margin, semi)
        elif variant == "b":
            loss, _ = ref_rest(triplet.pairwise_dist(x), t, K, margin, semi)
        else:
            loss, _ = crit(x, t, 0)
        loss.backward()
    return call


def inputs(n, d, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, d, generator=g) * 0.05).cuda().requires_grad_(True)
    t = (torch.arange(n) // K).cuda()
    return x, t


def time_variant(variant, n, d, K, margin, semi, warmup, iters, reps):
    x, t = inputs(n, d, K)
    call = make_call(variant, K, margin, semi)
    for _ in range(warmup):
        call(x, t)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call(x, t)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--margin", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--variant", default="c")
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--mode", default="semi")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.calls:
        x, t = inputs(args.n, args.d, args.K)
        call = make_call(args.variant, args.K, args.margin, args.mode == "semi")
        for _ in range(args.calls):
            call(x, t)
        torch.cuda.synchronize()
        print("ran %d calls of variant %s (n=%d d=%d %s)" % (args.calls, args.variant, args.n, args.d, args.mode))
        return
    print("TripletLoss forward + backward per call, n=%d num_instances=%d margin=%g, %s; median (min-max) of %d runs of %d calls after %d"
          % (args.n, args.K, args.margin, torch.cuda.get_device_name(0), args.reps, args.iters, args.warmup))
    for d in (128, 2048):
        for semi in (True, False):
            res = {v: time_variant(v, args.n, d, args.K, args.margin, semi, args.warmup, args.iters, args.reps) for v in "abc"}
            print("d=%4d %-4s  (a) reference loop %8.3f ms (%.3f-%.3f)  (b) pairwise_dist + loop %8.3f ms (%.3f-%.3f)  "
                  "(c) TripletLoss %7.4f ms (%.4f-%.4f)  b/c %.0fx" % ((d, "semi" if semi else "hard") + res["a"] + res["b"] + res["c"]
                                                                   + (res["b"][0] / res["c"][0],)), flush=True)


if __name__ == "__main__":
    main()
