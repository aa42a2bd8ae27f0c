#!/usr/bin/env python3
"""Generate tests/golden/triplet_loss_cases.npz from the reference's own TripletLoss (reid/loss/triplet.py:11-77; run where the
reference is).

The class is imported under make_golden.import_reid()'s stub modules and run in float64 on the CPU, as make_golden.triplet_fixture
does: loss, prec and d loss / d features for both mining branches (use_semi and hardest pair) of every case.  The cases cover the
two feature widths the fine-tune step feeds (d = 2048 and 128 at n = 128), n % K != 0, K = 8, shuffled labels (positional pairs
that are not same-label), margin 0 and 0.5, and the `w is not None` branch.

Features are not stored: the tests regenerate them with case_features() (tools/synth.py, rows grouped by identity as the
RandomIdentitySampler hands them out) and check their sha256 against the one recorded here.  The gradient is kept for a seeded sample
of its rows (`rows_<case>`: 8 at d >= 1024, else 24), which holds the file to about 0.3 MB; the tests compare every kept row in full.
"""
import hashlib
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
if TOOLS not in sys.path:                             # imported by tests/test_gpu_triplet_loss.py for case_features
    sys.path.insert(0, TOOLS)
OUT = os.path.join(ROOT, "tests", "golden", "triplet_loss_cases.npz")

from synth import clustered  # noqa: E402

GRAD_ROWS_WIDE, GRAD_ROWS = 8, 24       # gradient rows kept per case at d >= 1024 / below

# (n, d, K, margin, shuffled labels, w branch, seed)
CASES = (
    (128, 2048, 4, 0.5, False, False, 101),
    (128, 128, 4, 0.0, False, False, 102),
    (130, 128, 4, 0.5, False, False, 103),
    (64, 256, 8, 0.5, False, False, 104),
    (128, 128, 4, 0.3, True, False, 105),
    (64, 256, 4, 0.5, False, True, 106),
)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def case_features(n, d, K, shuffled, seed):
    """x [n, d] float32 and targets [n] int64: identities of K consecutive rows (the last n % K rows a short identity of their own);
    shuffled: the labels permuted, so positional pairs are mostly not same-label"""
    x = clustered(n, d, seed, per_id=K, intra=6.0)
    P = max(1, n // K)
    ids = np.arange(n) % P
    order = np.argsort(ids, kind="stable")           # rows of one identity together, as the sampler hands them out
    x = np.ascontiguousarray(x[order] * 2.0)
    targets = (np.arange(n) // K).astype(np.int64)
    if shuffled:
        targets = np.random.default_rng(seed).permutation(targets)
    return x, targets


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, ROOT)
    import torch
    import make_golden
    make_golden.import_reid()
    from reid.loss import TripletLoss
    rec = {"cases": len(CASES)}
    for ci, (n, d, K, margin, shuffled, weighted, seed) in enumerate(CASES):
        x, targets = case_features(n, d, K, shuffled, seed)
        rec["case_%d" % ci] = np.array([n, d, K, int(shuffled), int(weighted), seed], dtype=np.int64)
        rec["margin_%d" % ci] = np.float64(margin)
        rec["sha_%d" % ci] = sha(x)
        rec["targets_%d" % ci] = targets
        rows = np.sort(np.random.default_rng(seed).choice(n, GRAD_ROWS_WIDE if d >= 1024 else GRAD_ROWS, replace=False))
        rec["rows_%d" % ci] = rows.astype(np.int64)
        for semi in (True, False):
            xr = torch.from_numpy(x).double().requires_grad_(True)
            w = torch.ones(n, dtype=torch.float64) if weighted else None
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                loss, prec = TripletLoss(margin=margin, num_instances=K, use_semi=semi)(xr, torch.from_numpy(targets), 0, w)
                loss.backward()
            tag = "%d_%s" % (ci, "semi" if semi else "hard")
            rec["loss_" + tag] = np.float64(loss.item())
            rec["prec_" + tag] = np.float64(float(prec))
            rec["grad_" + tag] = xr.grad.numpy()[rows].astype(np.float32)
            print("case %d n=%d d=%d K=%d margin=%.1f shuffled=%d w=%d %s: loss %.6f prec %.4f" %
                  (ci, n, d, K, margin, shuffled, weighted, "semi" if semi else "hard", loss.item(), float(prec)))
    np.savez_compressed(OUT, **rec)
    print("wrote %s (%.2f MB)" % (OUT, os.path.getsize(OUT) / 1e6))


if __name__ == "__main__":
    main()
