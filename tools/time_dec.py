#!/usr/bin/env python3
"""Per-call time of the DEC term of the fine-tune step, forward + backward, at (B, K, D) = (128, 32, 2048):
  (a) the torch op chain of tests/dec_ref.py in float32 on the GPU -- what a user of the reference runs;
  (b) ssg_amd.dce.ClusterAssignment + ssg_amd.dce.kl_loss.
Both in one process, interleaved: per repetition device events around `iters` calls of (a), then of (b), after `warmup` calls of each;
the medians of `reps` repetitions.  Writes the lines to the file given as first argument (default profiles/dec_times.txt)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import dec_ref  # noqa: E402
from ssg_amd import dce  # noqa: E402

B, K, D, SCALE, SEED = 128, 32, 2048, 0.05, 301
WARMUP, ITERS, REPS = 20, 50, 9


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dec_times.txt")
    torch.cuda.set_device(0)
    x0, c0 = dec_ref.case_inputs(B, K, D, SEED, SCALE)
    x = x0.cuda().requires_grad_(True)
    c = c0.cuda().requires_grad_(True)
    m = dce.ClusterAssignment(K, D, cluster_centers=c0.cuda())

    def torch_chain():
        x.grad = c.grad = None
        q, _ = dec_ref.soft_assignment(x, c)
        (3 * dec_ref.kl_loss(q)).backward()

    def device():
        x.grad = m.cluster_centers.grad = None
        (3 * dce.kl_loss(m(x))).backward()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / ITERS

    for _ in range(WARMUP):
        torch_chain(); device()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REPS):
        ta.append(timed(torch_chain)); tb.append(timed(device))
    ta.sort(); tb.sort()
    med = lambda v: v[len(v) // 2]      # noqa: E731
    lines = ["DEC term forward + backward per call, (B, K, D) = (%d, %d, %d), %s; median (min-max) of %d interleaved runs of %d calls after %d"
             % (B, K, D, torch.cuda.get_device_name(0), REPS, ITERS, WARMUP),
             "(a) torch float32 op chain     %8.4f ms (%.4f-%.4f)" % (med(ta), ta[0], ta[-1]),
             "(b) ssg_amd.dce (csrc/dec.hip) %8.4f ms (%.4f-%.4f)" % (med(tb), tb[0], tb[-1]),
             "a / b = %.2f" % (med(ta) / med(tb))]
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
