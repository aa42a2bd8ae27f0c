#!/usr/bin/env python3
"""Generate tests/golden/dec_cases.npz from the reference's own DEC head (run where the reference is): `ClusterAssignment`
(reid/models/dce.py:7-51) and `FinedTrainer2.target_distribution` / `_forward`, `JointTrainer2._forward` (reid/trainers.py), imported
under make_golden.import_reid()'s stub modules and run in float64 on the CPU.

Per case (B, K, D, scale, seed): q, p [B, K], the loss nn.KLDivLoss(size_average=False)(q.log(), p) / B and its gradients with respect
to the batch (gx) and to `cluster_centers` (gc), all float64.  At D >= 1024 the gradients are kept for a seeded sample of 256 columns
(`cols_<case>`), which holds the file to about 0.3 MB; the tests compare every kept column in full.  Inputs are not stored: the tests
regenerate them with tests/dec_ref.py's case_inputs() and check their sha256 against the one recorded here.

Trainer records: `_forward` of both trainers on a stub model that returns fixed outputs (x3 = the reference's assignment of a case's
batch, float64) and stub criterions that return fixed (loss, prec) pairs -- the tensor branch (weight 3 in FinedTrainer2) and the
list branch."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "dec_cases.npz")

# (B, K, D, scale, seed)
CASES = (
    (5, 3, 40, 1.0, 201),
    (6, 32, 2048, 0.05, 202),
    (1, 32, 2048, 1.0, 203),
    (16, 32, 2048, 1.0, 204),
)
KEPT_COLS = 256
# stub criterions: (loss, prec) of criterions[0] (triplet) and criterions[1] (global); the losses are powers of two of the DEC
# term's own size, so that the total does not bury it
TRI, GLOBAL = (2.0 ** -21, 0.5), (2.0 ** -22, 0.75)
TRAINER_CASES = (1, 3)      # x3 of the first / second model call: cases (6, 32, 2048) and (16, 32, 2048)


def kept_cols(D, seed):
    if D < 1024:
        return np.arange(D, dtype=np.int64)
    return np.sort(np.random.default_rng(seed).choice(D, KEPT_COLS, replace=False)).astype(np.int64)


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, ROOT)
    import torch
    import make_golden
    import dec_ref
    make_golden.import_reid()
    from reid.models.dce import ClusterAssignment
    from reid.trainers import FinedTrainer2, JointTrainer2
    warnings.simplefilter("ignore")
    rec = {"cases": np.int64(len(CASES)), "tri": np.array(TRI), "global": np.array(GLOBAL), "trainer_cases": np.array(TRAINER_CASES, dtype=np.int64)}
    qs = {}
    for ci, (B, K, D, scale, seed) in enumerate(CASES):
        x, c = dec_ref.case_inputs(B, K, D, seed, scale)
        m = ClusterAssignment(K, D, alpha=7.0, cluster_centers=c.double().clone())      # alpha is ignored by the reference
        xx = x.double().clone().requires_grad_(True)
        q = m(xx)
        p = FinedTrainer2(None, None).target_distribution(q)
        loss = torch.nn.KLDivLoss(size_average=False)(q.log(), p) / q.shape[0]
        loss.backward()
        cols = kept_cols(D, seed)
        rec["case_%d" % ci] = np.array([B, K, D, seed], dtype=np.int64)
        rec["scale_%d" % ci] = np.float64(scale)
        rec["sha_%d" % ci] = dec_ref.sha_bytes(x, c)
        rec["cols_%d" % ci] = cols
        rec["q_%d" % ci] = q.detach().numpy()
        rec["p_%d" % ci] = p.detach().numpy()
        rec["loss_%d" % ci] = np.float64(loss.item())
        rec["gx_%d" % ci] = xx.grad.numpy()[:, cols]
        rec["gc_%d" % ci] = m.cluster_centers.grad.numpy()[:, cols]
        qs[ci] = q.detach()
        print("case %d B=%d K=%d D=%d scale=%g: loss %.6e  max|q - 1/K| %.3e  |gx|max %.3e |gc|max %.3e" %
              (ci, B, K, D, scale, loss.item(), float((q - 1.0 / K).abs().max()), float(xx.grad.abs().max()), float(m.cluster_centers.grad.abs().max())))

    def crit(pair):
        return lambda out, pids, epoch, w=None: (torch.tensor(pair[0], dtype=torch.float64), pair[1])

    def stub_model(as_list):
        calls = []

        def model(imgs):
            q = qs[TRAINER_CASES[len(calls) % 2]]
            calls.append(1)
            feat = torch.zeros(q.shape[0], 4, dtype=torch.float64)
            if as_list:
                return [feat, feat, feat], feat, [q, q * 1.0]
            return feat, feat, q
        return model

    pids = [torch.zeros(1, dtype=torch.long)] * 3
    for tag, as_list in (("tensor", False), ("list", True)):
        loss, prec = FinedTrainer2(stub_model(as_list), [crit(TRI), crit(GLOBAL)])._forward([None], pids, 0)
        rec["fined_%s_loss" % tag], rec["fined_%s_prec" % tag] = np.float64(float(loss)), np.float64(float(prec))
        print("FinedTrainer2 %s: loss %.9e prec %g" % (tag, float(loss), float(prec)))
        loss, prec = JointTrainer2(stub_model(as_list), [crit(TRI), crit(GLOBAL)])._forward([None], pids, [None], pids[0], 0)
        rec["joint_%s_loss" % tag], rec["joint_%s_prec" % tag] = np.float64(float(loss)), np.float64(float(prec))
        print("JointTrainer2 %s: loss %.9e prec %g" % (tag, float(loss), float(prec)))
    np.savez_compressed(OUT, **rec)
    print("wrote %s (%.2f MB)" % (OUT, os.path.getsize(OUT) / 1e6))


if __name__ == "__main__":
    main()
