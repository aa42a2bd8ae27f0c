#!/usr/bin/env python3
"""Write profiles/loss_times.txt (run on the MI355X, e.g. `timeout -k 10 600 python tools/time_losses.py`): forward + backward of the
classification losses at B = 128, float32, implementations interleaved in one process:

  ce        C = 751     (a) F.cross_entropy                                          (b) ssg_amd.CrossEntropyLoss
  focal     C = 751     (a) the reference's chain: log_softmax, gather, exp, pow     (b) ssg_amd.FocalLoss
  weightce  C = 751     (a) w-weighted F.cross_entropy(reduction='none') / B         (b) ssg_amd.WeightCE
                        (a1) the reference's loop of B one-row cross-entropies
  oim       C = 4096, F = 2048   (a) x @ lut.T, F.cross_entropy, then the reference's per-row table update loop
                                 (a1) the same with the update vectorised (unique targets only)   (b) ssg_amd.OIMLoss

One call = forward, then backward towards the logits (OIM: towards the features, and the table update).  Every call is timed on its own
with events; a round takes the median of CALLS calls of each implementation in turn, ROUNDS rounds; the table shows the median of the
round medians and their min-max (the spread).  A side wins when its median is lower than (a)'s by more than the larger of the two
spreads, else the line says "tie".  At these sizes a call is a handful of launches of a few microseconds each, so the host's launch
path is most of what is measured."""
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
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "loss_times.txt")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    lines = ["classification losses forward + backward per call at B = %d, %s, float32; median (min-max) over %d rounds of the median of %d calls, "
             "implementations interleaved" % (B, torch.cuda.get_device_name(0), ROUNDS, CALLS),
             "(a) torch's op chain  (a1) the reference's own loop  (b) ssg_amd",
             "%-10s %-22s %-5s %28s %7s %-7s" % ("loss", "shape", "impl", "ms", "a / .", "against (a)")]

    def report(piece, shape, tags, res):
        a = res[0]
        for tag, r in zip(tags, res):
            word = "-" if r is a else verdict(a, r, "slower", "faster")
            lines.append("%-10s %-22s %-5s %28s %7.2f %-7s" % (piece, shape, "(%s)" % tag, CELL % r, a[0] / r[0], word))
            print(lines[-1], flush=True)

    C = 751
    x = (3 * torch.randn((B, C), device=dev, generator=g)).requires_grad_(True)
    t = torch.randint(0, C, (B,), device=dev, generator=g)
    w = torch.rand((B,), device=dev, generator=g)
    shape = "B=%d C=%d" % (B, C)

    ce_dev = ssg_amd.CrossEntropyLoss()
    report("ce", shape, ("a", "b"), rounds([lambda: torch.autograd.grad(Fn.cross_entropy(x, t), x), lambda: torch.autograd.grad(ce_dev(x, t), x)], CALLS, ROUNDS, WARMUP))

    def torch_focal():
        logpt = Fn.log_softmax(x, dim=1).gather(1, t.view(-1, 1)).view(-1)
        pt = logpt.detach().exp()
        torch.autograd.grad((-1 * ((1 - pt) ** 2.0) * logpt).mean(), x)

    focal_dev = ssg_amd.FocalLoss(gamma=2.0)
    report("focal", shape, ("a", "b"), rounds([torch_focal, lambda: torch.autograd.grad(focal_dev(x, t, 0), x)], CALLS, ROUNDS, WARMUP))

    def reference_wce():
        loss = 0.
        for i in range(B):
            loss += w[i] * Fn.cross_entropy(x[i].unsqueeze(0), t[i].unsqueeze(0))
        torch.autograd.grad(loss / B, x)

    wce_dev = ssg_amd.WeightCE()
    report("weightce", shape, ("a", "a1", "b"), rounds([lambda: torch.autograd.grad((w * Fn.cross_entropy(x, t, reduction="none")).sum() / B, x), reference_wce,
                                                       lambda: torch.autograd.grad(wce_dev(x, t, w), x)], CALLS, ROUNDS, WARMUP))
    del x, t, w

    C, F, m = 4096, 2048, 0.5
    feats = torch.randn((B, F), device=dev, generator=g).requires_grad_(True)
    t = torch.randperm(C, device=dev, generator=g)[:B]                      # unique targets, so that (a1) computes the same update
    lut0 = Fn.normalize(torch.randn((C, F), device=dev, generator=g), dim=1)
    luts = [lut0.clone() for _ in range(2)]
    oim_dev = ssg_amd.OIMLoss(F, C, scalar=30.0, momentum=m).to(dev)
    oim_dev.lut.copy_(lut0)

    def torch_oim(lut, loop):
        logits = feats.mm(lut.t()) * 30.0
        torch.autograd.grad(Fn.cross_entropy(logits, t), feats)
        with torch.no_grad():
            if loop:
                for xi, y in zip(feats, t):
                    lut[y] = m * lut[y] + (1. - m) * xi
                    lut[y] /= lut[y].norm()
            else:
                lut[t] = Fn.normalize(m * lut[t] + (1. - m) * feats, dim=1)

    report("oim", "B=%d C=%d F=%d" % (B, C, F), ("a", "a1", "b"),
           rounds([lambda: torch_oim(luts[0], True), lambda: torch_oim(luts[1], False), lambda: torch.autograd.grad(oim_dev(feats, t)[0], feats)], CALLS, ROUNDS, WARMUP))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
