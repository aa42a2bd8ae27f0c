"""What tools/time_batchnorm.py, time_conv_train.py, time_conv_strided.py and time_head.py share: every call is timed on its own with
events, the implementations are run in turn round by round, and a side wins when its median is lower by more than the larger of the
two spreads."""
import statistics

CELL = "%9.4f (%.4f-%.4f)"                             # median (min-max) of a `rounds` result


def timed(fn):
    """milliseconds of one call of fn on the current stream"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def rounds(fns, calls, nrounds, warmup):
    """[(median, min, max) of the round medians] per function: `warmup` calls of each, then `nrounds` rounds that take the median of
    `calls` calls of each function in turn"""
    for fn in fns:
        for _ in range(warmup):
            timed(fn)
    meds = [[] for _ in fns]
    for _ in range(nrounds):
        for i, fn in enumerate(fns):
            meds[i].append(statistics.median(timed(fn) for _ in range(calls)))
    return [(statistics.median(m), min(m), max(m)) for m in meds]


def verdict(a, b, a_wins, b_wins, tie="tie"):
    """`a_wins` / `b_wins` when that side's median is lower by more than the larger of the two min-max spreads, else `tie`"""
    spread = max(a[2] - a[1], b[2] - b[1])
    return a_wins if b[0] - a[0] > spread else b_wins if a[0] - b[0] > spread else tie
