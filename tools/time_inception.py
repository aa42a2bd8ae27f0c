#!/usr/bin/env python3
"""Throughput of the InceptionNet embedder -> profiles/inception_times.txt.

images/s through `embed_with_flip` (both orientations of every image, evaluators.py:41-43) at B = 256 images of 144 x 56
(selftraining.py:105) for precision='split' and precision='f32', each with the dense inner layers of the branches on csrc/conv.hip
(the default) and with every convolution on csrc/inception.hip (SSG_INC_DENSE_CONV=0), and next to them torch's own forward of the restatement
tests/inception_ref.py (rocm torch, fp32, the same two orientations) on the same GPU.  Each figure is the median of --rounds round
medians (each the median of --reps event-timed calls after a warm-up, the forms taken in turn), with the smallest and the
largest round median beside it.
One process; a watchdog (--timeout seconds) ends it if it hangs.

Usage: python tools/time_inception.py [--batch 256] [--reps 5] [--rounds 5] [--timeout 400] [--out profiles/inception_times.txt]
"""
import argparse
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inception_times.txt"))
    a = ap.parse_args()
    signal.alarm(a.timeout)                             # the process ends itself if anything hangs
    import torch
    lines = ["InceptionNet embedder, embed_with_flip at 144 x 56 (tools/time_inception.py)"]
    if not torch.cuda.is_available():
        lines.append("not yet timed (no GPU in this run)")
    else:
        import ssg_amd
        import inception_ref
        from _timing import CELL, rounds
        from ssg_amd import inception
        dev = torch.device("cuda", 0)
        B = a.batch
        imgs = torch.randn(B, 3, 144, 56, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
        models = {p: ssg_amd.create("inception", seed=1, precision=p).cuda().eval() for p in ("split", "f32")}
        sd = {k: v.to(dev) for k, v in inception.synthetic_state_dict(seed=1).items() if v.dtype.is_floating_point}

        def torch_fwd():
            with torch.no_grad():
                inception_ref.sum_norm(inception_ref.head(sd, inception_ref.feature_map(sd, imgs)),
                                       inception_ref.head(sd, inception_ref.feature_map(sd, imgs.flip(3))))

        def ssg_fwd(precision, dense):
            def fn():
                models[precision].dense_conv = dense
                models[precision].embed_with_flip(imgs, check_overflow=False)
            return fn

        fns = [ssg_fwd("split", True), ssg_fwd("f32", True), ssg_fwd("split", False), ssg_fwd("f32", False), torch_fwd]
        res = rounds(fns, a.reps, a.rounds, 2)
        assert not models["split"]._overflowed()
        lines.append("device: %s; B = %d; %d rounds of %d calls, the five forms in turn; ms per call as median (min-max of the round medians)"
                     % (torch.cuda.get_device_name(0), B, a.rounds, a.reps))
        for name, r in zip(("ssg_amd precision='split'                         ", "ssg_amd precision='f32'                           ",
                            "ssg_amd precision='split', SSG_INC_DENSE_CONV=0   ", "ssg_amd precision='f32', SSG_INC_DENSE_CONV=0     ",
                            "torch fp32 restatement                            "), res):
            lines.append("  %s  %s ms   %9.1f images/s (%.1f - %.1f)" % (name, CELL % r, B / r[0] * 1e3, B / r[2] * 1e3, B / r[1] * 1e3))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
