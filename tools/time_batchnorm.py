#!/usr/bin/env python3
"""Write profiles/batchnorm_times.txt (run on the MI355X, e.g. `timeout -k 10 900 python tools/time_batchnorm.py`): train-mode batch
norm forward + backward at the BatchNorm shapes of ResNet-50 for B = 128 images of 256 x 128 (one line per distinct shape and variant,
plus feat_bn), three implementations in one process, run alternately:

  (a) torch   F.batch_norm(training=True) [-> + residual] [-> relu] under autograd, float32 on the same GPU
  (b) fused   ssg_amd.batch_norm_train(relu=, residual=)                      (csrc/batchnorm.hip)
  (c) swap    ssg_amd.batch_norm_train() followed by torch's add / relu       (what use_device_batchnorm(fuse=False) runs)

One call = forward, then torch.autograd.grad of y with a fixed upstream gradient towards x, weight, bias (and the residual).  Every call
is timed on its own with events; a round takes the median of CALLS calls of each implementation in turn, ROUNDS rounds; the table shows
the median of the round medians and their min-max (the spread).  GB/s: the tensor passes the fused form needs (forward 3, backward 5;
+2 for the ReLU mask read from y in both backward passes; +2 for the residual read and the d_residual store) times the tensor's
bytes, over the time -- beside the 6290 GB/s a float4 copy reaches on this chip.

The last lines say whether (b) beats (c) by more than the spread on every line with a ReLU: only then is fuse=True the default of
use_device_batchnorm."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from _timing import CELL, rounds, verdict  # noqa: E402 (tools/ is the script's own directory)

B = 128
CALLS, ROUNDS, WARMUP = 5, 7, 3
COPY_GBS = 6290.0
# (C, H, W, variants) of torchvision's ResNet-50 at 256 x 128 input: the stem, then per layer bn1 (before the strided conv2), bn2, and
# bn3 / the downsample's norm
SHAPES = [
    (64, 128, 64, ("relu",)),
    (64, 64, 32, ("relu",)),
    (256, 64, 32, ("plain", "relu_res")),
    (128, 64, 32, ("relu",)),
    (128, 32, 16, ("relu",)),
    (512, 32, 16, ("plain", "relu_res")),
    (256, 32, 16, ("relu",)),
    (256, 16, 8, ("relu",)),
    (1024, 16, 8, ("plain", "relu_res")),
    (512, 16, 8, ("relu",)),
    (512, 8, 4, ("relu",)),
    (2048, 8, 4, ("plain", "relu_res")),
    (2048, None, None, ("plain",)),            # feat_bn: BatchNorm1d on [B, 2048]
]
PASSES = {"plain": 8, "relu": 10, "relu_res": 12}


def main():
    import torch
    import torch.nn.functional as F
    import ssg_amd
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "batchnorm_times.txt")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    lines = ["train-mode batch norm forward + backward per call at B = %d, %s; median (min-max) over %d rounds of the median of %d calls, "
             "implementations interleaved" % (B, torch.cuda.get_device_name(0), ROUNDS, CALLS),
             "(a) torch float32 op chain  (b) ssg_amd.batch_norm_train fused  (c) ssg_amd.batch_norm_train + torch add / relu;  GB/s of (b) beside %.0f (float4 copy)"
             % COPY_GBS,
             "%-22s %-9s %26s %26s %26s %7s %7s %8s" % ("shape", "variant", "(a) ms", "(b) ms", "(c) ms", "a / b", "c / b", "(b) GB/s")]
    fused_wins, fused_lines = 0, 0
    for C, H, W, variants in SHAPES:
        shape = (B, C) if H is None else (B, C, H, W)
        x = torch.randn(shape, device=dev, generator=g).requires_grad_(True)
        r = torch.randn(shape, device=dev, generator=g).requires_grad_(True)
        gy = torch.randn(shape, device=dev, generator=g)
        w = (torch.rand(C, device=dev, generator=g) + 0.5).requires_grad_(True)
        b = torch.randn(C, device=dev, generator=g).requires_grad_(True)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        for variant in variants:
            relu, res = variant != "plain", (r if variant == "relu_res" else None)
            wrt = [x, w, b] + ([r] if res is not None else [])

            def torch_chain():
                y = F.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5)
                if res is not None:
                    y = y + res
                return torch.relu(y) if relu else y

            def fused():
                return ssg_amd.batch_norm_train(x, w, b, rm, rv, None, 0.1, 1e-5, relu, res)

            def swap():
                y = ssg_amd.batch_norm_train(x, w, b, rm, rv, None, 0.1, 1e-5)
                if res is not None:
                    y = y + res
                return torch.relu(y) if relu else y

            impls = [torch_chain, fused] + ([swap] if relu else [])

            stats = rounds([lambda fn=fn: torch.autograd.grad(fn(), wrt, gy) for fn in impls], CALLS, ROUNDS, WARMUP)
            cells = [CELL % s for s in stats] + (["-"] if not relu else [])
            gbs = PASSES[variant] * x.numel() * 4 / (stats[1][0] * 1e-3) / 1e9
            c_over_b = "%7.2f" % (stats[2][0] / stats[1][0]) if relu else "      -"
            lines.append("%-22s %-9s %26s %26s %26s %7.2f %s %8.0f" % ("x".join(str(s) for s in shape), variant, cells[0], cells[1], cells[2],
                                                                         stats[0][0] / stats[1][0], c_over_b, gbs))
            print(lines[-1], flush=True)
            if relu:
                fused_lines += 1
                fused_wins += int(verdict(stats[1], stats[2], "fused", "swap") == "fused")
        del x, r, gy
        torch.cuda.empty_cache()
    lines.append("fused (b) faster than the plain swap (c) by more than the spread of the round medians on %d of %d lines with a ReLU" % (fused_wins, fused_lines))
    lines.append("=> use_device_batchnorm: fuse defaults to %s" % (fused_wins == fused_lines))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
