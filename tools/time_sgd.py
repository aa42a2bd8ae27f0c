#!/usr/bin/env python3
"""Write profiles/sgd_times.txt (run on the MI355X, e.g. `timeout -k 10 900 python tools/time_sgd.py`): one optimiser step over the
parameter set of the reference's model -- the shapes of ResNet-50 without fc, then feat and feat_bn (tests/sgd_ref.py), 162 float32
tensors in the reference's two groups, momentum 0.9, weight decay 5e-4, every parameter with a gradient, buffers already there (not
the first step) -- implementations interleaved in one process, each on its own copy of the parameters:

  (a) torch.optim.SGD, default (foreach on the device)      (b) torch.optim.SGD(foreach=False)
  (c) torch.optim.SGD(fused=True), if this torch has it     (d) ssg_amd.SGD
  (e) ssg_sgd_step_f32 called with arrays prepared once: (d) without the Python layer's walk over the groups

One call = one step, timed on its own with events (so the time includes the host's share where the host is the slower side); a round
takes the median of CALLS calls of each implementation in turn, ROUNDS rounds; the table shows the median of the round medians and
their min-max (the spread).  A side wins when its median is lower than (a)'s by more than the larger of the two spreads, else "tie".
For (d) and (e) the table also shows the bytes the update has to move, 5 x 4 x elements (read p, g, buf; write p, buf), over the time,
beside the 6.29 TB/s of a float4 copy on this GPU.  The steps run back to back, so whatever part of the 330 MB working set the
256 MB last-level cache keeps is a help that a training step, with a forward and a backward pass in between, does not get.

`--sweep LIB [LIB ...]`: builds of the library with another chunk size (hipcc ... -DSSG_SGD_CHUNK=<elements> ... -o LIB), each timed
as (e) in a child process of its own (SSG_LIB_PATH=LIB) after the table, one line per build."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from _timing import CELL, rounds, verdict  # noqa: E402 (tools/ is the script's own directory)

CALLS, ROUNDS, WARMUP = 15, 9, 5
HYPER = dict(lr=0.01, momentum=0.9, weight_decay=5e-4)
COPY_RATE = 6.29e12


def parameter_set(torch, dev, seed):
    """the reference's two groups of Parameters, with gradients, from one seeded generator"""
    import sgd_ref
    base, new = sgd_ref.resnet50_shapes()
    g = torch.Generator(device=dev).manual_seed(seed)
    groups = []
    for shapes, mult in ((base, 0.1), (new, 1.0)):
        ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g) * 0.05) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, device=dev, generator=g) * 0.01
        groups.append(dict(params=ps, lr_mult=mult, lr=HYPER["lr"] * mult))
    return groups


def direct_call(torch, groups):
    """a closure that calls ssg_sgd_step_f32 on these groups with arrays built once (the buffers are made here)"""
    from ssg_amd import _lib
    L = _lib.lib()
    ps = [(gi, p) for gi, g in enumerate(groups) for p in g["params"]]
    bufs = [torch.zeros_like(p) for _, p in ps]
    n, k = len(ps), len(groups)
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])                          # noqa: E731
    dbl = lambda vs: (ctypes.c_double * k)(*vs)                                                   # noqa: E731
    args = [ptrs([p for _, p in ps]), ptrs([p.grad for _, p in ps]), ptrs(bufs), (ctypes.c_int64 * n)(*[p.numel() for _, p in ps]),
            (ctypes.c_int * n)(*[gi for gi, _ in ps]), (ctypes.c_int * n)(*[0] * n), n, dbl([g["lr"] for g in groups]), dbl([HYPER["momentum"]] * k),
            dbl([0.0] * k), dbl([HYPER["weight_decay"]] * k), (ctypes.c_int * k)(*[0] * k), (ctypes.c_int * k)(*[0] * k), k]
    keep = (ps, bufs)

    def call():
        _lib.check(L.ssg_sgd_step_f32(*args, _lib.stream()), "ssg_sgd_step_f32")
        return keep
    return call


def abi_only():
    """child of --sweep: one line for the library SSG_LIB_PATH names"""
    import torch
    from ssg_amd import _lib
    dev = torch.device("cuda", 0)
    groups = parameter_set(torch, dev, 0)
    elements = sum(p.numel() for g in groups for p in g["params"])
    (r,) = rounds([direct_call(torch, groups)], CALLS, ROUNDS, WARMUP)
    print("SWEEP chunk %6d elements   (e) %s ms   %5.2f TB/s" % (_lib.lib().ssg_sgd_chunk_elems(), CELL % r, 20.0 * elements / (r[0] * 1e-3) / 1e12), flush=True)


def main():
    import torch
    import ssg_amd
    from ssg_amd import _lib
    argv = sys.argv[1:]
    sweep = []
    if "--sweep" in argv:
        sweep = argv[argv.index("--sweep") + 1:]
        argv = argv[:argv.index("--sweep")]
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "sgd_times.txt")
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    names, fns = [], []

    def candidate(tag, what, make):
        try:
            opt = make(parameter_set(torch, dev, 0))
            opt.step()                                                   # the first step makes the buffers
        except (RuntimeError, ValueError, TypeError) as e:
            print("%s %s: not available on this torch (%s)" % (tag, what, str(e).splitlines()[0]), flush=True)
            return
        names.append((tag, what))
        fns.append(opt.step)

    candidate("(a)", "torch.optim.SGD default", lambda g: torch.optim.SGD(g, **HYPER))
    candidate("(b)", "torch.optim.SGD foreach=False", lambda g: torch.optim.SGD(g, foreach=False, **HYPER))
    candidate("(c)", "torch.optim.SGD fused=True", lambda g: torch.optim.SGD(g, fused=True, **HYPER))
    candidate("(d)", "ssg_amd.SGD", lambda g: ssg_amd.SGD(g, **HYPER))
    groups = parameter_set(torch, dev, 0)
    names.append(("(e)", "ssg_sgd_step_f32, prepared arrays"))
    fns.append(direct_call(torch, groups))
    tensors = sum(len(g["params"]) for g in groups)
    elements = sum(p.numel() for g in groups for p in g["params"])
    res = rounds(fns, CALLS, ROUNDS, WARMUP)

    lines = ["one SGD step (momentum 0.9, weight decay 5e-4, steady state) over %d float32 tensors, %d elements, in two groups, %s, torch %s; "
             "median (min-max) over %d rounds of the median of %d calls, implementations interleaved"
             % (tensors, elements, torch.cuda.get_device_name(0), torch.__version__, ROUNDS, CALLS),
             "chunk %d elements, at most %d tensors and %d chunks per launch; bytes moved = 5 x 4 x elements = %.1f MB; float4 copy rate %.2f TB/s"
             % (L.ssg_sgd_chunk_elems(), L.ssg_sgd_max_tensors_per_launch(), L.ssg_sgd_max_chunks_per_launch(), 20.0 * elements / 1e6, COPY_RATE / 1e12),
             "%-4s %-36s %28s %7s %-11s %s" % ("impl", "", "ms", "a / .", "against (a)", "bytes moved / time")]
    a = res[0]
    for (tag, what), r in zip(names, res):
        word = "-" if r is a else verdict(a, r, "slower", "faster")
        rate = "%5.2f TB/s (%.0f%% of the copy rate)" % (20.0 * elements / (r[0] * 1e-3) / 1e12, 100 * 20.0 * elements / (r[0] * 1e-3) / COPY_RATE) if tag in ("(d)", "(e)") else ""
        lines.append("%-4s %-36s %28s %7.2f %-11s %s" % (tag, what, CELL % r, a[0] / r[0], word, rate))
        print(lines[-1], flush=True)
    if sweep:
        lines.append("chunk sizes tried, each build timed as (e) in a process of its own (not interleaved with the table above):")
        for lib in [_lib.SO_PATH] + sweep:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--abi-only"], env=dict(os.environ, SSG_LIB_PATH=os.path.abspath(lib)),
                               capture_output=True, text=True, timeout=300)
            got = [ln[6:] for ln in r.stdout.splitlines() if ln.startswith("SWEEP ")]
            if r.returncode != 0 or not got:
                sys.exit("sweep child failed for %s (%d): %s" % (lib, r.returncode, r.stderr[-2000:]))
            lines.append(got[0])
            print(lines[-1], flush=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if "--abi-only" in sys.argv:
        abi_only()
    else:
        main()
