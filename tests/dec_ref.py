"""Restatement of the DEC head in torch on the CPU (reid/models/dce.py:47-51, reid/trainers.py:284-292 and the KLDivLoss term of
FinedTrainer2._forward), dtype a parameter, gradients by autograd: the yardstick of tests/test_gpu_dec.py.  In float64 it is checked
against the reference's own numbers (tests/golden/dec_cases.npz, tests/test_dec_host.py); in float32 it IS the reference's
arithmetic, the error of which bounds the error the kernels may have.

Also the seeded inputs of the golden cases (tools/make_golden_dec.py stores only seeds and a checksum) and the error criterion."""
import hashlib

import numpy as np
import torch

ALPHA = 1.0          # dce.py:27: whatever the constructor was given


def soft_assignment(x, c, alpha=ALPHA):
    """-> (q, ns): ns by direct differences over a [B, K, D] temporary, as the reference forms it"""
    ns = torch.sum((x.unsqueeze(1) - c) ** 2, 2)
    num = 1.0 / (1.0 + (ns / alpha))
    num = num ** (-float(alpha + 1) / 2)
    return (num.t() / torch.sum(num, 1)).t(), ns


def target_distribution(q):
    w = (q ** 2) / torch.sum(q, 0)
    return (w.t() / torch.sum(w, 1)).t()


def kl_loss(q):
    """sum p (log p - log q) / B with p = target_distribution(q) NOT detached"""
    p = target_distribution(q)
    return torch.nn.functional.kl_div(q.log(), p, reduction="sum") / q.shape[0]


def loss_grad_q(q, dtype, gloss=1.0):
    """(p, loss, d (gloss * loss) / d q) from a given q"""
    qq = q.detach().to(dtype).clone().requires_grad_(True)
    loss = kl_loss(qq)
    (loss * gloss).backward()
    return target_distribution(qq.detach()), loss.detach(), qq.grad


def assign_grad(x, c, gq, dtype, alpha=ALPHA):
    """(gx, gc) = gradient of sum(gq * q) with respect to the batch and the centres"""
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    cc = c.detach().to(dtype).clone().requires_grad_(True)
    q, _ = soft_assignment(xx, cc, alpha)
    (q * gq.to(dtype)).sum().backward()
    return xx.grad, cc.grad


def chain(x, c, dtype, alpha=ALPHA):
    """the whole head: dict(q, ns, p, loss, gx, gc) with gx, gc the gradients of the unit-weight loss"""
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    cc = c.detach().to(dtype).clone().requires_grad_(True)
    q, ns = soft_assignment(xx, cc, alpha)
    loss = kl_loss(q)
    loss.backward()
    return dict(q=q.detach(), ns=ns.detach(), p=target_distribution(q.detach()), loss=loss.detach(), gx=xx.grad, gc=cc.grad)


def case_inputs(B, K, D, seed, scale):
    """x [B, D] float32: non-negative and skewed like pooled post-ReLU features (2 * scale * u^3, u uniform); c [K, D] float32:
    Xavier-uniform centres.  Products and sums only, so every machine gets the same bits from the same seed."""
    g = torch.Generator().manual_seed(int(seed))
    u = torch.rand(B, D, generator=g)
    x = u * u * u * (2.0 * scale)
    bound = float(np.sqrt(6.0 / (K + D)))
    c = (torch.rand(K, D, generator=g) * 2.0 - 1.0) * bound
    return x, c


def sha_bytes(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def rel_err(got, ref):
    """max |got - ref| / max |ref| (float64); ref == 0 everywhere: the absolute error"""
    got = torch.as_tensor(got).detach().cpu().double()
    ref = torch.as_tensor(ref).detach().cpu().double()
    m = float(ref.abs().max())
    return float((got - ref).abs().max()) / (m if m > 0 else 1.0)


def trainer_totals(kl_a, kl_b, tri, glob):
    """what reid/trainers.py's _forward methods return for a stub model whose first call gives x3 = a and whose second call gives
    x3 = b, and stub criterions with the fixed losses `tri` (criterions[0]) and `glob` (criterions[1]); kl_* are the DEC terms, all in
    one dtype.  Tensor branch: one triplet term, weight 3 on the DEC term in FinedTrainer2 only; list branch (3 feature sets, x3 a list
    of two equal assignments): three triplet terms, every DEC term with weight 1.  Sums in the reference's order."""
    return {
        "fined_tensor": glob + tri + 3 * kl_a,
        "joint_tensor": (glob + tri + kl_b) + (glob + tri + kl_a),              # loss_os + loss_uns
        "fined_list": glob + tri + tri + tri + kl_a + kl_a,
        "joint_list": (glob + tri + tri + tri + kl_b + kl_b) + (glob + tri + tri + tri + kl_a + kl_a),
    }
