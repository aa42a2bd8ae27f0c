#!/usr/bin/env python3
"""Times of the fused layer1 BasicBlock (csrc/basicblock.hip) against the two launches it replaces -> profiles/basicblock_times.txt.

1. the layer1 identity block of ResNet-18 / ResNet-34 (64 x 32 x 64 map, split-half tensors) at B = 256 and B = 1000:
   ssg_basicblock_nhwc_x against two ssg_conv2d_nhwc_x launches, device events around each call, the two forms interleaved.
   The measurement (median of --reps launches after a warm-up) is repeated --rounds times; reported are the median of the
   round medians and their spread (largest minus smallest round median, the larger of the two forms), beside the fastest and
   slowest single launch.  The spread is taken over repeated MEDIANS because that is what the decision compares: one slow
   launch among a hundred (other work shares the host) says nothing about how well a median reproduces;
2. images/s of embed_with_flip for resnet18 and resnet34 at B = 256 with SSG_FUSED_BASICBLOCK on and off.
The decision rule for the default of SSG_FUSED_BASICBLOCK (resnet._FUSED_BASICBLOCK_DEFAULT): on if the fused median at B = 1000 is
below the two-launch median by more than that spread, else off; the last line of the file states the outcome.
One process; a watchdog (--timeout seconds) ends it if it hangs.

Usage: python tools/time_basicblock.py [--reps 20] [--rounds 5] [--timeout 240] [--out profiles/basicblock_times.txt]
"""
import argparse
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_pair(fa, fb, reps):
    """interleaved event timing of two callables: -> ([ms of fa], [ms of fb])"""
    import torch
    fa(); fb(); torch.cuda.synchronize()                # warm-up
    ta, tb = [], []
    for _ in range(reps):
        for fn, out in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            out.append(a.elapsed_time(b))
    return ta, tb


def block_times(B, reps, rounds, lines):
    import torch
    from ssg_amd import _lib, resnet
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    H, W, C = 64, 32, 64
    sd = resnet.synthetic_state_dict(seed=1, depth=18)
    c1 = resnet._fold(sd, "base.layer1.1.conv1", "base.layer1.1.bn1", 1, 1, dev, split=True)
    c2 = resnet._fold(sd, "base.layer1.1.conv2", "base.layer1.1.bn2", 1, 1, dev, split=True)
    x = torch.relu(torch.randn(B, H, W, C, generator=torch.Generator(device=dev).manual_seed(B), device=dev))
    xs = torch.empty_like(x)
    check(L.ssg_h8l8_encode(ptr(x), ptr(xs), x.numel(), 1.0, stream()), "encode")
    o, y, yf = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def fused():
        check(L.ssg_basicblock_nhwc_x(ptr(xs), ptr(c1.w), ptr(c1.bias), ptr(c1.cscale), ptr(c2.w), ptr(c2.bias), ptr(c2.cscale), ptr(yf), B, H, W, C,
                                      ptr(flag), stream()), "basicblock")

    def two():
        check(L.ssg_conv2d_nhwc_x(ptr(xs), ptr(c1.w), ptr(c1.bias), None, ptr(o), B, H, W, C, C, 3, 3, 1, 1, 1, 3, 1.0, ptr(c1.cscale), ptr(flag), stream()), "conv1")
        check(L.ssg_conv2d_nhwc_x(ptr(o), ptr(c2.w), ptr(c2.bias), ptr(xs), ptr(y), B, H, W, C, C, 3, 3, 1, 1, 1, 3, 1.0, ptr(c2.cscale), ptr(flag), stream()), "conv2")
    tf, tt, medf, medt = [], [], [], []
    for _ in range(rounds):
        a, b = timed_pair(fused, two, reps)
        tf += a; tt += b
        medf.append(statistics.median(a)); medt.append(statistics.median(b))
    same = torch.equal(yf.view(torch.int32), y.view(torch.int32))
    mf, mt = statistics.median(medf), statistics.median(medt)
    spread = max(max(medf) - min(medf), max(medt) - min(medt))
    flop = 2 * 2.0 * B * H * W * C * C * 9              # the convolutions' own operations (each product is three half MFMAs on the device)
    lines.append("layer1 identity block %dx%dx%d, B = %d (%d rounds of %d interleaved launches, each after a warm-up; outputs bit-equal: %s)"
                 % (H, W, C, B, rounds, reps, same))
    for name, m, meds, t in (("fused (ssg_basicblock_nhwc_x)       ", mf, medf, tf), ("two launches (ssg_conv2d_nhwc_x x 2)", mt, medt, tt)):
        lines.append("  %s  median %8.4f ms   round medians %8.4f .. %8.4f   single launches %8.4f .. %8.4f   %.1f TFLOP/s (convolution operations)"
                     % (name, m, min(meds), max(meds), min(t), max(t), flop / m / 1e9))
    return mf, mt, spread


def model_rates(depth, B, reps, lines):
    import torch
    import ssg_amd
    imgs = torch.randn(B, 3, 256, 128, generator=torch.Generator(device="cuda").manual_seed(depth), device="cuda")
    m = ssg_amd.create("resnet%d" % depth, num_classes=0, num_split=2, pretrained=False).cuda().eval()

    def run(flag):
        def fn():
            os.environ["SSG_FUSED_BASICBLOCK"] = flag
            m.embed_with_flip(imgs, check_overflow=False)
        return fn
    saved = os.environ.get("SSG_FUSED_BASICBLOCK")
    ton, toff = timed_pair(run("1"), run("0"), reps)
    if saved is None:
        os.environ.pop("SSG_FUSED_BASICBLOCK", None)
    else:
        os.environ["SSG_FUSED_BASICBLOCK"] = saved
    assert not m._overflowed()
    mon, moff = statistics.median(ton), statistics.median(toff)
    lines.append("resnet%d embed_with_flip, B = %d, S = 2 (%d interleaved repeats): fused block on %8.1f images/s (%.3f ms)   off %8.1f images/s (%.3f ms)"
                 % (depth, B, reps, B / mon * 1e3, mon, B / moff * 1e3, moff))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "basicblock_times.txt"))
    a = ap.parse_args()
    signal.alarm(a.timeout)                             # the process ends itself if anything hangs
    import torch
    lines = ["Fused layer1 BasicBlock against the two launches it replaces (tools/time_basicblock.py)"]
    if not torch.cuda.is_available():
        lines.append("(no GPU in this run: nothing measured)")
    else:
        lines.append("device: %s" % torch.cuda.get_device_name(0))
        lines.append("")
        res = {}
        for B in (256, 1000):
            res[B] = block_times(B, a.reps, a.rounds, lines)
        lines.append("")
        for depth in (18, 34):
            model_rates(depth, 256, max(3, a.reps // 2), lines)
        mf, mt, spread = res[1000]
        on = (mt - mf) > spread
        lines.append("")
        lines.append("decision at B = 1000: two launches %.4f ms - fused %.4f ms = %+.4f ms against a spread of the round medians of %.4f ms -> SSG_FUSED_BASICBLOCK defaults to %s"
                     % (mt, mf, mt - mf, spread, "1 (on)" if on else "0 (off)"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
