"""GPU suite of the device TripletLoss (csrc/triplet_loss.hip behind ssg_amd.triplet): against the reference's own float64 loss
(tests/golden/triplet_loss_cases.npz, written by tools/make_golden_triplet_loss.py, and triplet_ref.npz), against the reference's
mining loop run by torch on the same device dist (bit-equal pairs, exact prec, tie splitting of the gradient), against today's
pairwise_dist + torch loop, and for the absence of host syncs, determinism and the edge cases."""
import hashlib
import os

import numpy as np
import pytest
import torch

from ssg_amd import triplet
from make_golden_triplet_loss import case_features

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------ the reference's mining and hinge, reid/loss/triplet.py:32-77
def ref_pairs(dist, targets, K, semi):
    n = dist.size(0)
    P = n // K
    mask = targets.expand(n, n).eq(targets.expand(n, n).t())
    dist_ap, dist_an = [], []
    if semi:
        for i in range(P):
            for j in range(K):
                neg_examples = dist[i * K + j][mask[i * K + j] == 0]
                for pair in range(j + 1, K):
                    dist_ap.append(dist[i * K + j][i * K + pair].view(1))
                    dist_an.append(neg_examples.min().view(1))
    else:
        for i in range(n):
            dist_ap.append(dist[i][mask[i]].max().view(1))
            dist_an.append(dist[i][mask[i] == 0].min().view(1))
    return torch.cat(dist_ap), torch.cat(dist_an)


def ref_loss(dist, targets, K, margin, semi, w=None):
    ap, an = ref_pairs(dist, targets, K, semi)
    y = torch.ones_like(an)
    if w is not None:
        loss = 0.
        for i in range(an.size(0)):
            loss += torch.nn.functional.margin_ranking_loss(an[i].unsqueeze(0), ap, y, margin=margin)
        loss /= an.size(0)
    else:
        loss = torch.nn.functional.margin_ranking_loss(an, ap, y, margin=margin)
    prec = (an.data > ap.data).sum() * 1. / y.size(0)
    return loss, prec


def ref_dist(x):
    """reid/loss/triplet.py:28-31"""
    n = x.size(0)
    dist = torch.pow(x, 2).sum(dim=1, keepdim=True).expand(n, n)
    dist = dist + dist.t()
    dist = dist.addmm(x, x.t(), beta=1, alpha=-2)
    return dist.clamp(min=1e-12).sqrt()


# ------------------------------------------------------------------ 1. float64 goldens
def _check_vs_golden(tag, x, targets, K, margin, semi, w, loss_ref, prec_ref, grad_ref, rows):
    xg = torch.from_numpy(x).to(DEV).requires_grad_(True)
    loss, prec = triplet.TripletLoss(margin=margin, num_instances=K, use_semi=semi)(xg, torch.from_numpy(targets).to(DEV), 0, w)
    assert loss.dim() == 0 and prec.dim() == 0 and prec.dtype == torch.float32 and loss.is_cuda and prec.is_cuda
    loss.backward()
    dmax = float(ref_dist(torch.from_numpy(x).double()).max())
    lerr = abs(float(loss.detach()) - loss_ref)
    assert lerr < 1e-6 * max(1.0, dmax), (tag, lerr, dmax)
    assert abs(float(prec) - prec_ref) < 1e-7, (tag, float(prec), prec_ref)
    got = xg.grad.cpu().double()[rows]
    ref = torch.from_numpy(grad_ref).double()
    err = float((got - ref).abs().max())
    assert err < 3e-5 * max(float(ref.abs().max()), 1e-3), (tag, err, float(ref.abs().max()))


def test_float64_goldens_triplet_loss_cases():
    g = np.load(os.path.join(GOLDEN, "triplet_loss_cases.npz"))
    for ci in range(int(g["cases"])):
        n, d, K, shuffled, weighted, seed = (int(v) for v in g["case_%d" % ci])
        x, targets = case_features(n, d, K, bool(shuffled), seed)
        assert hashlib.sha256(x.tobytes()).hexdigest() == str(g["sha_%d" % ci]), "case_features no longer reproduces the fixture"
        assert np.array_equal(targets, g["targets_%d" % ci])
        w = torch.ones(n, device=DEV) if weighted else None
        for semi in (True, False):
            tag = "%d_%s" % (ci, "semi" if semi else "hard")
            _check_vs_golden(tag, x, targets, K, float(g["margin_%d" % ci]), semi, w, float(g["loss_" + tag]), float(g["prec_" + tag]),
                             g["grad_" + tag], torch.from_numpy(g["rows_%d" % ci]))


def test_float64_goldens_triplet_ref():
    g = np.load(os.path.join(GOLDEN, "triplet_ref.npz"))
    for ci in range(int(g["cases"])):
        x, targets = g["x_%d" % ci], g["targets_%d" % ci]
        for semi in (True, False):
            tag = "%d_%s" % (ci, "semi" if semi else "ohem")
            _check_vs_golden(tag, x, targets, 4, 0.5, semi, None, float(g["loss_" + tag]), float(g["prec_" + tag]), g["grad_" + tag],
                             torch.arange(x.shape[0]))


# ------------------------------------------------------------------ 2. the same device dist: exact
def _crafted_cases():
    g = torch.Generator().manual_seed(7)
    cases = []
    for n, K, shuffled, kind in ((128, 4, False, "rand"), (64, 2, False, "ties"), (96, 8, False, "ties"), (130, 4, False, "ties"),
                                 (61, 4, True, "ties"), (128, 4, True, "rand"), (45, 8, True, "rand"), (128, 4, False, "ties")):
        t = torch.arange(n) // K
        if shuffled:
            t = t[torch.randperm(n, generator=g)]
        if kind == "rand":
            dist = torch.rand(n, n, generator=g) * 2
        else:                   # few distinct values: exact ties among hardest negatives / positives and hinge terms exactly 0
            dist = torch.randint(1, 6, (n, n), generator=g).float() / 4
        cases.append((dist, t, K))
    return cases


def test_same_dist_pairs_loss_prec_and_grad_exact():
    gen = torch.Generator().manual_seed(3)
    for ci, (dist0, t, K) in enumerate(_crafted_cases()):
        dist0, t = dist0.to(DEV), t.to(DEV)
        for semi in (True, False):
            # mining: bit-equal pairs, and the gradient of an arbitrary objective of them
            dr = dist0.clone().requires_grad_(True)
            ap_r, an_r = ref_pairs(dr, t, K, semi)
            dg = dist0.clone().requires_grad_(True)
            ap_g, an_g = triplet.hard_pairs(dg, t, K, semi)
            assert torch.equal(ap_g, ap_r.detach()) and torch.equal(an_g, an_r.detach()), (ci, semi)
            u1, u2 = torch.randn(ap_r.shape[0], generator=gen).to(DEV), torch.randn(ap_r.shape[0], generator=gen).to(DEV)
            ((ap_r * u1).sum() + (an_r * u2).sum()).backward()
            ((ap_g * u1).sum() + (an_g * u2).sum()).backward()
            err = float((dg.grad - dr.grad).abs().max())
            assert err <= 1e-6 * float(dr.grad.abs().max()) + 1e-12, (ci, semi, "pairs", err)
            for margin in (0.0, 0.5):
                for weighted in (False, True):
                    w = torch.ones(dist0.shape[0], device=DEV) if weighted else None
                    dr = dist0.clone().requires_grad_(True)
                    lr, pr = ref_loss(dr, t, K, margin, semi, w)
                    dg = dist0.clone().requires_grad_(True)
                    lg, pg = triplet.triplet_loss_from_dist(dg, t, K, margin, semi, w)
                    tag = (ci, semi, margin, weighted)
                    assert torch.equal(pg, pr), tag
                    # the loss against the same loop in float64 on the same dist values (the same pairs and hinge decisions: a float32
                    # difference of two float32 distances keeps its sign, the margins are exact): torch's float32 sums differ from it by
                    # their summation order, the w branch's `loss +=` over M terms by up to ~M/2 ulp
                    d64 = dist0.clone().double().requires_grad_(True)
                    l64 = ref_loss(d64, t, K, margin, semi, w)[0]
                    assert abs(float(lg.detach()) - float(l64.detach())) <= 1e-6 * max(1.0, abs(float(l64.detach()))), tag
                    assert abs(float(lr.detach()) - float(l64.detach())) <= 1e-5 * max(1.0, abs(float(l64.detach()))), tag
                    if weighted:
                        # likewise the w branch adds M hinge gradients into every dist_ap entry one loss term at a time: its gradient is
                        # held to the float64 loop
                        dr, lr = d64, l64
                    lr.backward()
                    lg.backward()
                    err = float((dg.grad.double() - dr.grad.double()).abs().max())
                    assert err <= 1e-6 * float(dr.grad.abs().max()) + 1e-12, (tag, err)


# ------------------------------------------------------------------ 3. end to end against pairwise_dist + the torch loop
def test_end_to_end_vs_pairwise_dist_and_torch_loop():
    g = torch.Generator().manual_seed(17)
    for d in (128, 2048):
        n, K = 128, 4
        x0 = torch.randn(n, d, generator=g) * 0.05
        x0[5] = x0[4]; x0[9] = x0[8]; x0[70] = x0[3]           # duplicate rows: sq at or below the clamp floor
        t = (torch.arange(n) // K).to(DEV)
        for semi in (True, False):
            for margin in (0.0, 0.3):
                xb = x0.clone().to(DEV).requires_grad_(True)
                db = triplet.pairwise_dist(xb)
                lb, pb = ref_loss(db, t, K, margin, semi)
                lb.backward()
                ap_r, an_r = ref_pairs(db.detach(), t, K, semi)
                ap_g, an_g = triplet.hard_pairs(triplet.pairwise_dist(x0.to(DEV)), t, K, semi)
                assert torch.equal(ap_g, ap_r) and torch.equal(an_g, an_r), (d, semi)
                xc = x0.clone().to(DEV).requires_grad_(True)
                lc, pc = triplet.TripletLoss(margin=margin, num_instances=K, use_semi=semi)(xc, t, 0)
                lc.backward()
                tag = (d, semi, margin)
                assert torch.equal(pc, pb), tag
                assert abs(float(lc) - float(lb)) <= 2e-6 * max(1.0, abs(float(lb))), (tag, float(lc), float(lb))
                err = float((xc.grad - xb.grad).abs().max())
                assert err <= 2e-5 * max(float(xb.grad.abs().max()), 1e-6), (tag, err, float(xb.grad.abs().max()))


# ------------------------------------------------------------------ 4. no host sync
def test_no_host_sync_in_forward_and_backward():
    n, d, K = 128, 2048, 4
    g = torch.Generator().manual_seed(23)
    x = (torch.randn(n, d, generator=g) * 0.05).to(DEV).requires_grad_(True)
    t = (torch.arange(n) // K).to(DEV)
    crits = [triplet.TripletLoss(margin=0.3, num_instances=K, use_semi=s) for s in (True, False)]
    for c in crits:                                              # warm-up: library load, allocator
        c(x, t, 0)[0].backward()
    torch.cuda.synchronize()
    dist = triplet.pairwise_dist(x.detach())
    torch.cuda.synchronize()
    control_raised = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            ref_loss(dist, t, K, 0.3, True)
        except RuntimeError:
            control_raised = True
        if control_raised:
            for c in crits:
                for w in (None, torch.ones(n, device=DEV)):
                    loss, prec = c(x, t, 0, w)
                    loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    if not control_raised:
        pytest.skip("this torch build does not raise on the reference loop's boolean index under set_sync_debug_mode('error')")


# ------------------------------------------------------------------ 5. determinism
def test_bit_identical_repeats():
    n, K = 128, 4
    g = torch.Generator().manual_seed(29)
    x0 = torch.randn(n, 2048, generator=g) * 0.05
    t = (torch.arange(n) // K).to(DEV)
    for semi in (True, False):
        for w in (None, torch.ones(n)):
            outs = []
            for _ in range(2):
                x = x0.clone().to(DEV).requires_grad_(True)
                loss, prec = triplet.TripletLoss(margin=0.3, num_instances=K, use_semi=semi)(x, t, 0, w)
                loss.backward()
                outs.append((loss.detach().clone(), prec.clone(), x.grad.clone()))
            for a, b in zip(*outs):
                assert torch.equal(a, b), (semi, w is None)


# ------------------------------------------------------------------ 6. edge cases
def test_single_label_batch_gives_nan():
    x = torch.randn(16, 64).to(DEV).requires_grad_(True)
    t = torch.zeros(16, dtype=torch.int64, device=DEV)
    for semi in (True, False):
        loss, prec = triplet.TripletLoss(margin=0.3, num_instances=4, use_semi=semi)(x, t, 0)
        assert torch.isnan(loss) and torch.isnan(prec), semi
        loss.backward()
        l2, p2 = triplet.triplet_loss_from_dist(torch.rand(16, 16, device=DEV), t, 4, 0.3, semi)
        assert torch.isnan(l2) and torch.isnan(p2)


def test_two_criteria_summed_like_fined_trainer():
    """FinedTrainer2._forward: loss = criterion1(...); loss += criterion0(...); loss.backward() -- against the reference in float64"""
    n, d, K = 64, 256, 4
    g = torch.Generator().manual_seed(31)
    x0 = torch.randn(n, d, generator=g) * 0.05
    proj = torch.randn(d, 128, generator=g) / 16
    t = torch.arange(n) // K

    def run(x, p, c0, c1, tt):
        feats = x @ p
        loss, prec = c1(x, tt, 3)
        loss_tri, _ = c0(feats, tt, 3)
        loss += loss_tri
        loss.backward()
        return loss.detach(), prec

    xr = x0.clone().double().requires_grad_(True)
    lr, pr = run(xr, proj.double(), lambda f, tt, e: ref_loss(ref_dist(f), tt, K, 0.5, True),
                 lambda f, tt, e: ref_loss(ref_dist(f), tt, K, 0.3, False), t)
    xg = x0.clone().to(DEV).requires_grad_(True)
    lg, pg = run(xg, proj.to(DEV), triplet.TripletLoss(0.5, K, True), triplet.TripletLoss(0.3, K, False), t.to(DEV))
    assert abs(float(lg) - float(lr)) < 2e-6 * max(1.0, float(lr)), (float(lg), float(lr))
    assert abs(float(pg) - float(pr)) < 1e-7
    err = float((xg.grad.cpu().double() - xr.grad).abs().max())
    assert err < 3e-5 * max(float(xr.grad.abs().max()), 1e-3), err


def test_input_dtype_and_device_roundtrip():
    n, d, K = 32, 64, 4
    x64 = torch.randn(n, d, dtype=torch.float64).requires_grad_(True)          # CPU float64 in, gradient back as CPU float64
    loss, prec = triplet.TripletLoss(0.3, K)(x64, torch.arange(n) // K, 0)
    loss.backward()
    assert loss.is_cuda and x64.grad.dtype == torch.float64 and x64.grad.device.type == "cpu"
    xr = x64.detach().clone().requires_grad_(True)
    lr, _ = ref_loss(ref_dist(xr), torch.arange(n) // K, K, 0.3, True)
    lr.backward()
    assert abs(float(loss) - float(lr)) < 1e-5
    assert float((x64.grad - xr.grad).abs().max()) < 3e-5 * max(float(xr.grad.abs().max()), 1e-3)
