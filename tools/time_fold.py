#!/usr/bin/env python3
"""Write profiles/fold_times.txt (run on the MI355X, e.g. `timeout -k 10 600 python tools/time_fold.py`): the embedder taking the
weights of a ResNet-50 that lives on the GPU (the state of the model the fine-tune phase has just trained), precision 'split':

  (a) the host route     embedder.load_state_dict(module.state_dict()) + _prepare(): one blocking device-to-host copy per tensor, the
                         float64 fold / pack / row scales / half split of 53 convolutions on the CPU, 53 uploads
  (b) refresh            embedder.refresh(module): one device-to-device copy per tensor, one csrc/fold.hip launch per convolution
  (c) the launches alone the fold launches of (b) on tensors already in place (`_invalidate()` + `_prepare()`)
  (d) the kernels alone  (c) enqueued behind a spinning kernel, so that every launch is in the queue before the first one starts:
                         events around the launches then see the device's time without the host's gaps

One call = one whole refresh, timed on its own with events around it (the host's share is inside where the host is the slower side);
a round takes the median of CALLS calls of each route in turn, ROUNDS rounds; the table shows the median of the round medians and their
min-max (the spread).  A side wins when its median is lower by more than the larger of the two spreads, else "tie".  (d) is also
shown as bytes moved (the float32 weights read once, the folded rows written once) over its time."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from _timing import CELL, rounds, verdict  # noqa: E402 (tools/ is the script's own directory)

CALLS, ROUNDS, WARMUP = 5, 7, 2


class _Source:
    """what refresh and load_state_dict see of a trained model: `state_dict()` hands out the tensors on the device"""

    def __init__(self, sd):
        self._sd = sd

    def state_dict(self):
        return dict(self._sd)


def main():
    import warnings
    import torch
    import ssg_amd
    from ssg_amd import resnet
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fold_times.txt")
    dev = torch.device("cuda", 0)
    sd = {k: v.to(dev) for k, v in ssg_amd.synthetic_state_dict(seed=1, depth=50).items()}
    src = _Source(sd)
    warnings.simplefilter("ignore")
    host = resnet.ResNet(50, pretrained=False, precision="split").cuda().eval()
    fresh = resnet.ResNet(50, pretrained=False, precision="split").cuda().eval()
    alone = resnet.ResNet(50, pretrained=False, precision="split").cuda().eval()
    alone.refresh(src)

    def route_host():
        host.load_state_dict(src.state_dict())
        host._prepare()

    def route_refresh():
        fresh.refresh(src)

    def launches_alone():
        alone._invalidate()
        alone._prepare()

    res = rounds([route_host, route_refresh, launches_alone], CALLS, ROUNDS, WARMUP)
    import statistics
    dts = []
    for _ in range(CALLS * ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(40_000_000)                            # about 20 ms: the host enqueues every launch meanwhile
        e0.record()
        launches_alone()
        e1.record()
        e1.synchronize()
        dts.append(e0.elapsed_time(e1))
    d = (statistics.median(dts), min(dts), max(dts))
    # the two routes must have built the same bits
    a, b = host._prepare(), fresh._prepare()
    convs = [(a["stem"], b["stem"])] + [(x[k], y[k]) for x, y in zip(a["blocks"], b["blocks"]) for k in ("c1", "c2", "c3", "ds") if x.get(k) is not None]
    same = all(torch.equal(p.w.view(torch.int32), q.w.view(torch.int32)) and torch.equal(p.bias.view(torch.int32), q.bias.view(torch.int32)) for p, q in convs)
    launches = len(convs)
    moved = sum(2 * p.w.numel() * 4 for p, _ in convs)
    h, r, k = res
    lines = ["embedder refresh from a GPU-resident ResNet-50 state dict (%d tensors, %d fold launches), precision split, %s, torch %s; "
             "median (min-max) over %d rounds of the median of %d calls, routes interleaved"
             % (len(sd), launches, torch.cuda.get_device_name(0), torch.__version__, ROUNDS, CALLS),
             "%-4s %-58s %30s" % ("", "", "ms"),
             "%-4s %-58s %30s" % ("(a)", "load_state_dict(module.state_dict()) + _prepare() [host fold]", CELL % h),
             "%-4s %-58s %30s   a / b = %.1f   refresh is %s" % ("(b)", "refresh(module) [device fold]", CELL % r, h[0] / r[0],
                                                              verdict(h, r, "slower", "faster", "tied with the host route")),
             "%-4s %-58s %30s" % ("(c)", "the fold launches alone (_invalidate + _prepare)", CELL % k),
             "%-4s %-58s %30s   %.1f MB read + written: %.2f TB/s   (median, min-max of %d calls)"
             % ("(d)", "the kernels alone (the launches of (c), queued ahead)", CELL % d, moved / 1e6, moved / (d[0] * 1e-3) / 1e12, len(dts)),
             "folded weights of (a) and (b) bit-identical: %s" % ("yes" if same else "NO")]
    for ln in lines:
        print(ln, flush=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not same:
        sys.exit("the two routes disagree")


if __name__ == "__main__":
    main()
