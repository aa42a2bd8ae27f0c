#!/usr/bin/env python3
"""Interleaved A/B of library builds / env knobs inside ONE process (development aid): every repetition runs one embedding forward per
variant, round-robin, with HIP events around every C-ABI launch -- run-to-run and box-to-box noise (+-3 %, DVFS) is common to the variants.

usage: ab_inproc.py [--B 1000] [--reps 6] name=lib.so[,ENV=VAL,...] ...
Each variant gets its own dlopen'ed copy of the library (its `static` knob caches are read under its own environment at the first call).
Run-time knobs are compared on ONE build (`new=lib.so line0=lib.so,SSG_CONV_LINE=0`: the pixel fetch order of conv_dma_kernel;
`tall0=lib.so,SSG_CONV_TALL_MINTILES=0`: no 256 x 256 tiles).  Two builds of csrc/ssg_hip.hip -- another commit, or a compile-time switch
such as the epilogue cache policies `-DSSG_DMA_RES_AUX=...` -- are compared as two libraries; the same library under two names measures the
noise floor of the comparison (`base=old.so base2=old.so new=lib.so`).  A variant's environment is also set around each of its forwards, so
knobs that are read per call follow it (`off=lib.so,SSG_BN_L1_NEXT=0 next=lib.so,SSG_BN_L1_NEXT=1`); variants that take different routes
get a table each.  A library from before an entry point of the header answers 0 from its `_supported` / `_enabled` predicates."""
import argparse
import contextlib
import ctypes
import os
import shutil
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


@contextlib.contextmanager
def _env(envs):
    old = {k: os.environ.get(k) for k in envs}
    os.environ.update(envs)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--json", default="")
    ap.add_argument("variants", nargs="+")
    a = ap.parse_args()
    import ssg_amd
    from ssg_amd import _lib
    import layer_table as lt
    dev = torch.device("cuda", 0)
    protos = _lib.parse_header()
    tmp = tempfile.mkdtemp(prefix="ab_")
    m = ssg_amd.create("resnet50", num_classes=0, num_split=1, cluster=False, pretrained=False).cuda().eval()
    x = torch.randn(a.B, 3, 256, 128, device=dev)
    var = []
    for i, spec in enumerate(a.variants):
        name, rest = spec.split("=", 1)
        parts = rest.split(",")
        path, envs = parts[0], dict(p.split("=", 1) for p in parts[1:])
        cp = os.path.join(tmp, "lib%d.so" % i)
        shutil.copy(os.path.join(ROOT, path) if not os.path.isabs(path) else path, cp)
        old = {k: os.environ.get(k) for k in envs}
        os.environ.update(envs)
        L = ctypes.CDLL(cp)
        for fn, (res, args) in protos.items():
            try:
                f = getattr(L, fn)
            except AttributeError:                    # a build from before this entry point: its predicates answer 0, calling anything else is an error
                def missing(*_, fn=fn, pred=fn.endswith(("_supported", "_enabled"))):
                    if not pred:
                        raise AttributeError("%s: no %s in this build" % (name, fn))
                    return 0
                setattr(L, fn, missing)
                continue
            f.restype = res; f.argtypes = args
        _lib._lib = L
        var.append(dict(name=name, L=L, env=envs, sums=None, tot=[], rows=None))
        with _env(envs):
            m._fmap(x); torch.cuda.synchronize()      # knob caches are filled under this variant's environment
    for rep in range(a.reps):
        for v in (var if rep % 2 == 0 else var[::-1]):
            rec = lt.Rec(v["L"]); _lib._lib = rec
            with _env(v["env"]):                      # (knobs that are read per call, such as SSG_BN_L1_NEXT, follow their variant)
                m._fmap(x); torch.cuda.synchronize()
            ms = [r[2].elapsed_time(r[3]) for r in rec.rows]
            v["sums"] = ms if v["sums"] is None else [p + q for p, q in zip(v["sums"], ms)]
            v["tot"].append(sum(ms))
            v["rows"] = v["rows"] or rec.rows
    labels = [[lt.work(r[0], r[1], a.B) for r in v["rows"]] for v in var]
    if all([w[2] for w in l] == [w[2] for w in labels[0]] for l in labels):
        print("%-50s" % "launch" + "".join("%10s" % v["name"] for v in var))
        for i, (fl, by, label) in enumerate(labels[0]):
            if fl == 0:
                continue
            print("%2d %-47s" % (i, label) + "".join("%10.3f" % (v["sums"][i] / a.reps) for v in var))
    else:                                             # the variants take different routes: one table each
        for v, l in zip(var, labels):
            print("-- %s" % v["name"])
            for i, (fl, by, label) in enumerate(l):
                if fl != 0:
                    print("%2d %-62s%10.3f" % (i, label, v["sums"][i] / a.reps))
    print("%-50s" % "total ms (mean)" + "".join("%10.3f" % (sum(v["tot"]) / a.reps) for v in var))
    print("%-50s" % "total ms (min)" + "".join("%10.3f" % min(v["tot"]) for v in var))
    print("%-50s" % "total ms (median)" + "".join("%10.3f" % sorted(v["tot"])[len(v["tot"]) // 2] for v in var))
    print("%-50s" % "total ms (max)" + "".join("%10.3f" % max(v["tot"]) for v in var))
    if a.json:
        import json
        json.dump({v["name"]: dict(per_launch=[s / a.reps for s in v["sums"]], totals=v["tot"]) for v in var}, open(a.json, "w"))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
