#!/usr/bin/env python3
"""Write profiles/head_times.txt (run on the MI355X, e.g. `timeout -k 10 600 python tools/time_head.py`): forward + backward of the
three pieces of the reference's head at B = 128, float32, implementations interleaved in one process:

  pool            an 8 x 4 x 2048 channels_last map, num_split 2      (a) the reference's S + 2 F.avg_pool2d calls   (b) stripe_pool_train
  feat            Linear(2048, 2048, bias=False)                      (a) F.linear   (b) linear_train   (c) conv2d_train on [B, K, 1, 1]
  classifier_x2   Linear(2048, 751)                                   (a) F.linear   (b) linear_train

One call = forward, then torch.autograd.grad of a fixed upstream gradient on every output towards the input and the parameters.  Every
call is timed on its own with events; a round takes the median of CALLS calls of each implementation in turn, ROUNDS rounds; the table
shows the median of the round medians and their min-max (the spread).  A side wins when its median is lower than (a)'s by more than
the larger of the two spreads, else the line says "tie"."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from _timing import CELL, rounds, verdict  # noqa: E402 (tools/ is the script's own directory)

B = 128
CALLS, ROUNDS, WARMUP = 7, 9, 3


def main():
    import torch
    import torch.nn.functional as Fn
    import ssg_amd
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "head_times.txt")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    CL = torch.channels_last
    lines = ["train-mode head forward + backward per call at B = %d, %s, float32; median (min-max) over %d rounds of the median of %d calls, "
             "implementations interleaved" % (B, torch.cuda.get_device_name(0), ROUNDS, CALLS),
             "(a) torch's op chain  (b) ssg_amd.stripe_pool_train / linear_train  (c) ssg_amd.conv2d_train on the [B, K, 1, 1] view (feat only)",
             "%-14s %-26s %-4s %28s %7s %-7s" % ("piece", "shape", "impl", "ms", "a / .", "against (a)")]

    def report(piece, shape, res):
        a = res[0]
        for tag, r in zip("abc", res):
            word = "-" if r is a else verdict(a, r, "slower", "faster")
            lines.append("%-14s %-26s %-4s %28s %7.2f %-7s" % (piece, shape, "(%s)" % tag, CELL % r, a[0] / r[0], word))
            print(lines[-1], flush=True)

    # the pools
    S, C, h, w = 2, 2048, 8, 4
    x = torch.randn((B, C, h, w), device=dev, generator=g).contiguous(memory_format=CL).requires_grad_(True)
    gs = [torch.randn((B, C), device=dev, generator=g) for _ in range(S + 2)]

    def torch_pools():
        hs = h // S
        outs = [Fn.avg_pool2d(x, (h, w)).view(B, -1)]
        outs += [Fn.avg_pool2d(x[:, :, hs * s: hs * (s + 1), :], (hs, w)).view(B, -1) for s in range(S)]
        outs.append(Fn.avg_pool2d(x, (h, w)).view(B, -1))                   # the second global pool, for x2
        torch.autograd.grad(outs, [x], gs)

    def device_pools():
        sets = ssg_amd.stripe_pool_train(x, S)
        torch.autograd.grad(list(sets), [x], [gs[0] + gs[S + 1]] + gs[1:S + 1])

    report("pool", "%dx%dx%d S=%d" % (h, w, C, S), rounds([torch_pools, device_pools], CALLS, ROUNDS, WARMUP))
    del x, gs

    # the Linears
    for piece, K, N, bias in (("feat", 2048, 2048, False), ("classifier_x2", 2048, 751, True)):
        xin = torch.randn((B, K), device=dev, generator=g).requires_grad_(True)
        wt = (torch.randn((N, K), device=dev, generator=g) * K ** -0.5).requires_grad_(True)
        bs = torch.randn((N,), device=dev, generator=g).requires_grad_(True) if bias else None
        gy = torch.randn((B, N), device=dev, generator=g)
        wrt = [xin, wt] + ([bs] if bias else [])
        fns = [lambda: torch.autograd.grad(Fn.linear(xin, wt, bs), wrt, gy), lambda: torch.autograd.grad(ssg_amd.linear_train(xin, wt, bs), wrt, gy)]
        if not bias and N % 64 == 0 and K % 64 == 0:                            # the closest path before this module: a 1x1 convolution
            x4 = xin.detach().view(B, K, 1, 1).contiguous(memory_format=CL).requires_grad_(True)
            w4 = wt.detach().view(N, K, 1, 1).requires_grad_(True)
            gy4 = gy.view(B, N, 1, 1).contiguous(memory_format=CL)
            fns.append(lambda: torch.autograd.grad(ssg_amd.conv2d_train(x4, w4), [x4, w4], gy4))
        report(piece, "B=%d K=%d N=%d%s" % (B, K, N, " +bias" if bias else ""), rounds(fns, CALLS, ROUNDS, WARMUP))
        del xin, wt, bs, gy, fns
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
