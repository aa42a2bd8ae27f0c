"""Pairwise block of the fine-tune phase's TripletLoss on the GPU -- reid/loss/triplet.py:28-31:

    dist = torch.pow(inputs, 2).sum(dim=1, keepdim=True).expand(n, n)
    dist = dist + dist.t()
    dist.addmm_(1, -2, inputs, inputs.t())
    dist = dist.clamp(min=1e-12).sqrt()

Forward: the fp32-MFMA Gram kernel with its distance epilogue (`ssg_pairwise_sqdist_f32`, shared with the evaluator's
`pairwise_distance`) + an in-place clamp/sqrt.  Backward (round 4): `pairwise_dist` is a `torch.autograd.Function`, so the block can
stand where the reference's four lines stand inside `TripletLoss.forward` -- the loss back-propagates through `dist` into the
features: grad_x = diag(rowsum(S)) x - S x with S = W + W^T, W = grad_dist / dist where the clamp passes the gradient; S x runs on
the same fp32-MFMA GEMM (`ssg_conv2d_nhwc_f32` as a 1 x 1 convolution), the two elementwise halves are HIP kernels
(`ssg_triplet_grad_weights`, `ssg_triplet_grad_combine`).

The whole loss (reid/loss/triplet.py:19-77) is `TripletLoss`: the same Gram kernel for the squared distances, then one HIP mining
kernel (csrc/triplet_loss.hip) that square-roots them on the fly, finds every anchor's hardest negative (and hardest positive) with
its tie count and writes the pairs in the reference's append order, and one fixed-order reduction into loss and prec -- no host
sync, where the reference's loops block on a boolean index per anchor.  The backward rebuilds S = W + W^T straight from that
mining record and runs the S x GEMM above.  `hard_pairs` / `triplet_loss_from_dist` run the same kernels on a given [n, n] dist.

One difference from the reference: a batch in which some anchor has no negative (a single-label batch) makes the reference raise
(min() of an empty tensor); detecting that needs a host read, so here loss and prec come back NaN instead."""
import torch
from torch import nn

from . import _lib
from ._lib import SSGError, check, ptr, stream
from .evaluators import _sqdist

CLAMP_MIN = 1e-12           # triplet.py:31 dist.clamp(min=1e-12)
MAX_N = 4096                # batch rows the mining kernels take


class _PairwiseDist(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, clamp_min):
        L = _lib.lib()
        xc = x.detach().to(torch.device("cuda", torch.cuda.current_device()), torch.float32).contiguous()
        sq = _sqdist(xc, xc).contiguous()
        dist = sq.clone()
        check(L.ssg_clamp_sqrt_f32(ptr(dist), dist.numel(), float(clamp_min), stream()), "ssg_clamp_sqrt_f32")
        ctx.save_for_backward(xc, sq, dist)
        ctx.clamp_min, ctx.in_device, ctx.in_dtype = float(clamp_min), x.device, x.dtype
        return dist

    @staticmethod
    def backward(ctx, grad_dist):
        L = _lib.lib()
        x, sq, dist = ctx.saved_tensors
        n, d = x.shape
        dev, st = x.device, stream()
        g = grad_dist.to(dev, torch.float32).contiguous()
        ld = (n + 31) // 32 * 32                       # K granule of the GEMM
        dp = (d + 63) // 64 * 64                       # its output-channel granule
        S = torch.empty((n, ld), dtype=torch.float32, device=dev)
        rowsum = torch.empty(n, dtype=torch.float32, device=dev)
        check(L.ssg_triplet_grad_weights(ptr(g), ptr(sq), ptr(dist), n, ld, ctx.clamp_min, ptr(S), ptr(rowsum), st), "ssg_triplet_grad_weights")
        xt = torch.zeros((dp, ld), dtype=torch.float32, device=dev)
        xt[:d, :n] = x.t()                             # the GEMM's "weights": x^T, one row per feature channel
        zeros = torch.zeros(dp, dtype=torch.float32, device=dev)
        Sx = torch.empty((n, dp), dtype=torch.float32, device=dev)
        check(L.ssg_conv2d_nhwc_f32(ptr(S), ptr(xt), ptr(zeros), None, ptr(Sx), n, 1, 1, ld, dp, 1, 1, 1, 0, 0, st), "ssg_conv2d_nhwc_f32 (S x)")
        gx = torch.empty((n, d), dtype=torch.float32, device=dev)
        check(L.ssg_triplet_grad_combine(ptr(x), ptr(rowsum), ptr(Sx), n, d, dp, ptr(gx), st), "ssg_triplet_grad_combine")
        return gx.to(device=ctx.in_device, dtype=ctx.in_dtype), None


def pairwise_dist(inputs, clamp_min=1e-12):
    """inputs [n, d] float32 (any device; may require grad) -> [n, n] float32 CUDA, float32 accuracy (GEMM accumulation order differs
    from torch's).  Differentiable: the gradient flows back to `inputs` like through the reference's four lines."""
    x = torch.as_tensor(inputs)
    if x.dim() != 2:
        raise ValueError("inputs must be [n, d]")
    return _PairwiseDist.apply(x, clamp_min)


# ------------------------------------------------------------------ mining + hinge (reid/loss/triplet.py:32-77)
def _num_pairs(n, K, use_semi):
    """M, with the reference's errors: P = n // K first (ZeroDivisionError for K == 0 in both branches); the semi branch with no
    positional pair ends in torch.cat([]) (RuntimeError)"""
    P = n // K
    if n < 1 or n > MAX_N:
        raise ValueError("TripletLoss: batch of %d rows; the mining kernels take 1 <= n <= %d" % (n, MAX_N))
    if use_semi:
        M = P * K * (K - 1) // 2
        if M == 0:
            raise RuntimeError("torch.cat(): expected a non-empty list of Tensors (no positional pair: n=%d, num_instances=%d)" % (n, K))
        return M
    return n


def _device():
    if not torch.cuda.is_available():
        raise SSGError("ssg_amd.triplet.TripletLoss needs a GPU (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _record(n, M, dev):
    rec_f = torch.empty(2 * n + 4 * M, dtype=torch.float32, device=dev)
    rec_i = torch.empty(2 * n + 2 * M, dtype=torch.int32, device=dev)
    return rec_f, rec_i


def _targets(targets, n, dev):
    t = torch.as_tensor(targets).detach().to(dev, torch.int64).reshape(-1).contiguous()
    if t.numel() != n:
        raise ValueError("targets has %d entries for %d rows" % (t.numel(), n))
    return t


def _mine(L, mat, ld, is_sq, tg, n, K, semi, M, margin, weighted, dev):
    rec_f, rec_i = _record(n, M, dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    prec = torch.empty((), dtype=torch.float32, device=dev)
    check(L.ssg_triplet_mine_f32(ptr(mat), ld, is_sq, CLAMP_MIN, ptr(tg), n, K, semi, M, float(margin), weighted, ptr(rec_f), ptr(rec_i),
                                 ptr(loss), ptr(prec), stream()), "ssg_triplet_mine_f32")
    return rec_f, rec_i, loss, prec


class _TripletLossFn(torch.autograd.Function):
    """inputs [n, d] -> (loss, prec); the whole loss on the GPU, the gradient back to inputs"""

    @staticmethod
    def forward(ctx, x, targets, K, M, semi, margin, weighted):
        L = _lib.lib()
        dev = _device()
        xc = x.detach().to(dev, torch.float32).contiguous()
        n = xc.shape[0]
        tg = _targets(targets, n, dev)
        sq = _sqdist(xc, xc)                           # [n, n] view of the padded Gram output: the kernel reads it at its pitch
        rec_f, rec_i, loss, prec = _mine(L, sq, sq.stride(0), 1, tg, n, K, semi, M, margin, weighted, dev)
        ctx.save_for_backward(xc, sq, tg, rec_f, rec_i)
        ctx.args = (K, M, semi, weighted)
        ctx.in_device, ctx.in_dtype = x.device, x.dtype
        ctx.mark_non_differentiable(prec)
        return loss, prec

    @staticmethod
    def backward(ctx, gloss, gprec):
        L = _lib.lib()
        xc, sq, tg, rec_f, rec_i = ctx.saved_tensors
        K, M, semi, weighted = ctx.args
        n, d = xc.shape
        dev, st = xc.device, stream()
        g = gloss.to(dev, torch.float32).contiguous()  # read by the kernel through its device pointer
        ldS = (n + 31) // 32 * 32                      # K granule of the GEMM
        dp = (d + 63) // 64 * 64                       # its output-channel granule
        S = torch.empty((n, ldS), dtype=torch.float32, device=dev)
        rowsum = torch.empty(n, dtype=torch.float32, device=dev)
        xt = torch.empty((dp, ldS), dtype=torch.float32, device=dev)
        zeros = torch.empty(dp, dtype=torch.float32, device=dev)
        check(L.ssg_triplet_grad_weights_rec(ptr(sq), sq.stride(0), CLAMP_MIN, ptr(tg), n, K, semi, M, weighted, ptr(rec_f), ptr(rec_i), ptr(g),
                                             ptr(xc), d, ldS, dp, ptr(S), ptr(rowsum), ptr(xt), ptr(zeros), st), "ssg_triplet_grad_weights_rec")
        Sx = torch.empty((n, dp), dtype=torch.float32, device=dev)
        check(L.ssg_conv2d_nhwc_f32(ptr(S), ptr(xt), ptr(zeros), None, ptr(Sx), n, 1, 1, ldS, dp, 1, 1, 1, 0, 0, st), "ssg_conv2d_nhwc_f32 (S x)")
        gx = torch.empty((n, d), dtype=torch.float32, device=dev)
        check(L.ssg_triplet_grad_combine(ptr(xc), ptr(rowsum), ptr(Sx), n, d, dp, ptr(gx), st), "ssg_triplet_grad_combine")
        return gx.to(device=ctx.in_device, dtype=ctx.in_dtype), None, None, None, None, None, None


class _FromDistFn(torch.autograd.Function):
    """dist [n, n] -> (dist_ap, dist_an) (pairs=True) or (loss, prec); the gradient back to dist, written densely"""

    @staticmethod
    def forward(ctx, dist, targets, K, M, semi, margin, weighted, pairs):
        L = _lib.lib()
        dev = _device()
        dc = dist.detach().to(dev, torch.float32).contiguous()
        n = dc.shape[0]
        tg = _targets(targets, n, dev)
        rec_f, rec_i, loss, prec = _mine(L, dc, n, 0, tg, n, K, semi, M, margin, weighted, dev)
        ctx.save_for_backward(dc, tg, rec_f, rec_i)
        ctx.args = (K, M, semi, weighted, pairs)
        ctx.in_device, ctx.in_dtype = dist.device, dist.dtype
        if pairs:
            return rec_f[2 * n:2 * n + M].clone(), rec_f[2 * n + M:2 * n + 2 * M].clone()
        ctx.mark_non_differentiable(prec)
        return loss, prec

    @staticmethod
    def backward(ctx, g0, g1):
        L = _lib.lib()
        dc, tg, rec_f, rec_i = ctx.saved_tensors
        K, M, semi, weighted, pairs = ctx.args
        n, dev = dc.shape[0], dc.device

        def dev32(t):
            return None if t is None else t.to(dev, torch.float32).contiguous()
        gloss, gap, gan = (None, dev32(g0), dev32(g1)) if pairs else (dev32(g0), None, None)
        gdist = torch.empty((n, n), dtype=torch.float32, device=dev)
        check(L.ssg_triplet_grad_dist_f32(ptr(dc), n, 0, CLAMP_MIN, ptr(tg), n, K, semi, M, weighted, ptr(rec_f), ptr(rec_i), ptr(gloss), ptr(gap),
                                          ptr(gan), ptr(gdist), stream()), "ssg_triplet_grad_dist_f32")
        return gdist.to(device=ctx.in_device, dtype=ctx.in_dtype), None, None, None, None, None, None, None


def _square(dist):
    d = torch.as_tensor(dist)
    if d.dim() != 2 or d.shape[0] != d.shape[1]:
        raise ValueError("dist must be [n, n]")
    return d


def hard_pairs(dist, targets, num_instances, use_semi=True):
    """The mining of reid/loss/triplet.py:32-61 on a given [n, n] dist: (dist_ap, dist_an) [M] float32 on the GPU, in the order the
    reference appends them (bit-equal values), differentiable with respect to dist"""
    d = _square(dist)
    n = d.shape[0]
    M = _num_pairs(n, num_instances, use_semi)
    return _FromDistFn.apply(d, targets, int(num_instances), M, 1 if use_semi else 0, 0.0, 0, True)


def triplet_loss_from_dist(dist, targets, num_instances, margin=0, use_semi=True, w=None):
    """reid/loss/triplet.py:32-77 on a given [n, n] dist -> (loss, prec), 0-dim float32 on the GPU; loss differentiable w.r.t. dist.
    Only `w is None` matters (the values of w are never read, as in the reference)."""
    d = _square(dist)
    n = d.shape[0]
    M = _num_pairs(n, num_instances, use_semi)
    return _FromDistFn.apply(d, targets, int(num_instances), M, 1 if use_semi else 0, float(margin), 0 if w is None else 1, False)


class TripletLoss(nn.Module):
    """Drop-in for reid/loss/triplet.py:11-77 (`from ssg_amd.triplet import TripletLoss` after the reference's own import):
    forward(inputs, targets, epoch, w=None) -> (loss, prec).  `epoch` is ignored (the curriculum branch is `if False`), only
    `w is None` matters.  inputs of any dtype / device are taken as float32 on the current GPU; the gradient comes back in
    theirs.  n <= 4096.  An anchor without negatives gives NaN loss and prec (the reference raises)."""

    def __init__(self, margin=0, num_instances=0, use_semi=True):
        super(TripletLoss, self).__init__()
        self.margin = margin
        self.use_semi = use_semi
        self.ranking_loss = nn.MarginRankingLoss(margin=self.margin)
        self.K = num_instances

    def forward(self, inputs, targets, epoch, w=None):
        x = torch.as_tensor(inputs)
        n = x.size(0)
        M = _num_pairs(n, self.K, self.use_semi)
        if x.dim() != 2:
            raise ValueError("inputs must be [n, d]")
        return _TripletLossFn.apply(x, targets, int(self.K), M, 1 if self.use_semi else 0, float(self.margin), 0 if w is None else 1)
