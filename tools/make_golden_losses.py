#!/usr/bin/env python3
"""Generate tests/golden/loss_cases.npz from the reference's own FocalLoss (reid/loss/triplet.py:79-106), WeightCE
(reid/loss/weight_cross_entropy.py) and accuracy (reid/evaluation_metrics/classification.py); run where the reference is.

The classes are imported under make_golden.import_reid()'s stub modules and run on CPU float32 tensors: inputs, losses, gradients
towards the logits and accuracies are stored.  FocalLoss's constructor evaluates the Python 2 name `long`, so `builtins.long = int` is
set first.  OIM (reid/loss/oim.py) is a legacy instance-style autograd.Function that a current torch refuses to run, so it has no
golden: tests/loss_ref.py's restatement is its only yardstick.

The logits are tie-free (the top gaps of every row are at least 1e-3), so accuracy does not depend on torch.topk's order among ties."""
import builtins
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
OUT = os.path.join(ROOT, "tests", "golden", "loss_cases.npz")

# (B, C, seed)
SHAPES = ((3, 2, 11), (16, 65, 12), (8, 751, 13))
# (name, gamma, alpha: None | 'binary' (a float, C == 2 only) | 'list' (C entries), size_average)
FOCAL = (("g2_mean", 2.0, None, True), ("g05_alpha_sum", 0.5, "list", False), ("g0_mean", 0, None, True), ("g2_binary", 2.0, "binary", True))
TOPK = (1,)                                          # the reference's `correct[:k].view(-1)` raises for k > 1 on a current torch


def logits(B, C, seed):
    """tie-free float32 logits: in every row any two values differ by at least 1e-3"""
    rng = np.random.default_rng(seed)
    order = np.argsort(rng.standard_normal((B, C)), axis=1)      # a random order per row over an evenly spaced grid of values
    grid = ((np.arange(C) - C / 2.0) * max(0.01, 6.0 / C)).astype(np.float32)
    x = np.empty((B, C), dtype=np.float32)
    np.put_along_axis(x, order, np.broadcast_to(grid, (B, C)), axis=1)
    assert C == 1 or float(np.diff(np.sort(x.astype(np.float64), axis=1), axis=1).min()) >= 1e-3
    return x


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, ROOT)
    builtins.long = int
    import torch
    import make_golden
    make_golden.import_reid()
    from reid.loss.triplet import FocalLoss
    from reid.loss.weight_cross_entropy import WeightCE
    from reid.evaluation_metrics.classification import accuracy
    rec = {"shapes": np.array(SHAPES, dtype=np.int64), "topk": np.array(TOPK, dtype=np.int64), "focal": np.array([f[0] for f in FOCAL])}
    for si, (B, C, seed) in enumerate(SHAPES):
        rng = np.random.default_rng(seed + 100)
        x, t = logits(B, C, seed), rng.integers(0, C, B).astype(np.int64)
        t[::2] = x.argmax(axis=1)[::2]               # every other row is a top-1 hit
        w = rng.uniform(0.0, 1.0, B).astype(np.float32)
        alpha = rng.uniform(0.25, 2.0, C).astype(np.float32)
        rec.update({"x_%d" % si: x, "t_%d" % si: t, "w_%d" % si: w, "alpha_%d" % si: alpha})
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for name, gamma, akind, size_average in FOCAL:
                if akind == "binary" and C != 2:
                    continue
                a = None if akind is None else 0.25 if akind == "binary" else [float(v) for v in alpha]
                xr = torch.from_numpy(x).requires_grad_(True)
                loss = FocalLoss(gamma=gamma, alpha=a, size_average=size_average)(xr, torch.from_numpy(t), 0)
                loss.backward()
                rec["focal_%s_loss_%d" % (name, si)] = np.float32(loss.item())
                rec["focal_%s_grad_%d" % (name, si)] = xr.grad.numpy().copy()
                print("shape %d (B=%d C=%d) FocalLoss %s: %.7f" % (si, B, C, name, loss.item()))
            xr = torch.from_numpy(x).requires_grad_(True)
            loss = WeightCE()(xr, torch.from_numpy(t), torch.from_numpy(w))
            loss.backward()
            rec["wce_loss_%d" % si] = np.float32(loss.item())
            rec["wce_grad_%d" % si] = xr.grad.numpy().copy()
            acc = accuracy(torch.from_numpy(x), torch.from_numpy(t), topk=tuple(k for k in TOPK if k <= C))
            rec["acc_%d" % si] = np.concatenate([a.numpy() for a in acc]).astype(np.float32)
            print("shape %d WeightCE %.7f accuracy %s" % (si, loss.item(), rec["acc_%d" % si]))
    np.savez_compressed(OUT, **rec)
    print("wrote %s (%.1f KB)" % (OUT, os.path.getsize(OUT) / 1e3))


if __name__ == "__main__":
    main()
