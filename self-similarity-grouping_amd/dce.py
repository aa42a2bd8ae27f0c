"""DEC cluster head of the fine-tune phase (--dce-loss) on the GPU -- reid/models/dce.py:7-51 (`ClusterAssignment`),
reid/trainers.py:284-292 (`target_distribution`) and the KLDivLoss term of FinedTrainer2 / JointTrainer2._forward (:268-279):

    norm_squared = torch.sum((batch.unsqueeze(1) - self.cluster_centers)**2, 2)          # [B, K, D] temporary
    numerator = (1.0 / (1.0 + norm_squared / alpha)) ** (-(alpha + 1) / 2)
    q = (numerator.t() / torch.sum(numerator, 1)).t()
    weight = q ** 2 / torch.sum(q, 0);  p = (weight.t() / torch.sum(weight, 1)).t()
    loss = nn.KLDivLoss(size_average=False)(q.log(), p) / B                               # p is not detached

Four entry points of csrc/dec.hip stand for that chain (`ssg_dec_assign_f32`, `ssg_dec_kl_loss_f32`, `ssg_dec_kl_loss_grad_f32`,
`ssg_dec_assign_grad_f32`): float32 tensors in and out, every sum in float64 in a fixed order, no host read, no [B, K, D] temporary.
`ClusterAssignment` and `kl_loss` are differentiable (torch.autograd.Function around the kernels), so the reference's optimiser
trains `cluster_centers` through them.

The reference's quirks are kept: the module sets alpha = 1.0 whatever the constructor was given, and with
alpha = 1 the exponent is -1, so q is proportional to 1 + |x - c|^2 -- the farthest centre gets the largest weight.

There is no CPU fallback: without a GPU every compute entry point raises SSGError."""
import torch
from torch import nn
from torch.nn import Parameter

from . import _lib
from ._lib import SSGError, check, ptr, stream

MAX_B = 4096                # batch rows the kernels take
MAX_K = 64                  # cluster centres


def _device():
    if not torch.cuda.is_available():
        raise SSGError("ssg_amd.dce needs a GPU (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _rows(t, dev):
    """[B, D] float32 on `dev` with unit column stride (a row pitch larger than D is passed on to the kernel as it is)"""
    t = t.detach().to(dev, torch.float32)
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def _check_q(q, what):
    q = torch.as_tensor(q)
    if q.dim() != 2:
        raise ValueError("%s: q must be [B, K]" % what)
    return q


def soft_assignment(batch, centers, alpha=1.0, want_ns=False):
    """dce.py:47-51 on given tensors, no autograd: batch [B, D], centers [K, D] -> q [B, K] float32 on the GPU (and ns, the squared
    distances, with want_ns)"""
    dev = _device()
    x, c = _rows(torch.as_tensor(batch), dev), torch.as_tensor(centers).detach().to(dev, torch.float32).contiguous()
    if x.dim() != 2 or c.dim() != 2 or x.shape[1] != c.shape[1]:
        raise ValueError("batch must be [B, D] and centers [K, D] (got %r and %r)" % (tuple(x.shape), tuple(c.shape)))
    B, D = x.shape
    K = c.shape[0]
    q = torch.empty((B, K), dtype=torch.float32, device=dev)
    ns = torch.empty((B, K), dtype=torch.float32, device=dev) if want_ns else None
    check(_lib.lib().ssg_dec_assign_f32(ptr(x), x.stride(0), ptr(c), B, K, D, float(alpha), ptr(q), ptr(ns), stream()), "ssg_dec_assign_f32")
    return (q, ns) if want_ns else q


class _AssignFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, batch, centers, alpha):
        dev = _device()
        x, c = _rows(batch, dev), centers.detach().to(dev, torch.float32).contiguous()
        B, D = x.shape
        K = c.shape[0]
        q = torch.empty((B, K), dtype=torch.float32, device=dev)
        ns = torch.empty((B, K), dtype=torch.float32, device=dev)
        check(_lib.lib().ssg_dec_assign_f32(ptr(x), x.stride(0), ptr(c), B, K, D, alpha, ptr(q), ptr(ns), stream()), "ssg_dec_assign_f32")
        ctx.save_for_backward(x, c, ns)
        ctx.alpha = alpha
        ctx.src = ((batch.device, batch.dtype), (centers.device, centers.dtype))
        return q

    @staticmethod
    def backward(ctx, gq):
        x, c, ns = ctx.saved_tensors
        dev = x.device
        (B, D), K = x.shape, c.shape[0]
        g = gq.to(dev, torch.float32).contiguous()
        gns = torch.empty((B, K), dtype=torch.float64, device=dev)
        gx = torch.empty((B, D), dtype=torch.float32, device=dev)
        gc = torch.empty((K, D), dtype=torch.float32, device=dev)
        check(_lib.lib().ssg_dec_assign_grad_f32(ptr(x), x.stride(0), ptr(c), ptr(ns), ptr(g), B, K, D, ctx.alpha, ptr(gns), ptr(gx), ptr(gc), stream()),
              "ssg_dec_assign_grad_f32")
        (xd, xt), (cd, ct) = ctx.src
        return gx.to(device=xd, dtype=xt), gc.to(device=cd, dtype=ct), None


class ClusterAssignment(nn.Module):
    """Drop-in for reid/models/dce.py:7-51: the same attributes, the same Parameter name (`cluster_centers`), the same Xavier-uniform
    initialisation through torch's global generator (the same seed gives the reference's centres bit for bit).  `alpha` is ignored like
    there: the module always works with alpha = 1.0.  forward(batch [B, D]) -> q [B, K] float32 on the current GPU, differentiable
    with respect to `batch` and `cluster_centers` (gradients come back in their dtype / on their device).
    B <= 4096, cluster_number <= 64."""

    def __init__(self, cluster_number, embedding_dimension, alpha=1.0, cluster_centers=None):
        super(ClusterAssignment, self).__init__()
        self.embedding_dimension = embedding_dimension
        self.cluster_number = cluster_number
        self.alpha = 1.0
        if cluster_centers is None:
            initial_cluster_centers = torch.zeros(self.cluster_number, self.embedding_dimension, dtype=torch.float)
            nn.init.xavier_uniform_(initial_cluster_centers)
        else:
            initial_cluster_centers = cluster_centers
        self.cluster_centers = initial_cluster_centers if isinstance(initial_cluster_centers, Parameter) else Parameter(initial_cluster_centers)

    def forward(self, batch):
        x = torch.as_tensor(batch)
        if x.dim() != 2 or x.shape[1] != self.cluster_centers.shape[1]:
            raise ValueError("batch must be [B, %d] (got %r)" % (self.cluster_centers.shape[1], tuple(x.shape)))
        return _AssignFn.apply(x, self.cluster_centers, float(self.alpha))


def target_distribution(q):
    """reid/trainers.py:284-292 on the GPU: q [B, K] -> p [B, K] float32.  The value only: the gradient through p is part of
    `kl_loss`, which is what the trainers differentiate."""
    q = _check_q(q, "target_distribution")
    dev = _device()
    qc = q.detach().to(dev, torch.float32).contiguous()
    B, K = qc.shape
    p = torch.empty((B, K), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    check(_lib.lib().ssg_dec_kl_loss_f32(ptr(qc), B, K, ptr(p), ptr(loss), stream()), "ssg_dec_kl_loss_f32")
    return p


class _KLFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q):
        dev = _device()
        qc = q.detach().to(dev, torch.float32).contiguous()
        B, K = qc.shape
        loss = torch.empty((), dtype=torch.float32, device=dev)
        check(_lib.lib().ssg_dec_kl_loss_f32(ptr(qc), B, K, None, ptr(loss), stream()), "ssg_dec_kl_loss_f32")
        ctx.save_for_backward(qc)
        ctx.src = (q.device, q.dtype)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        qc, = ctx.saved_tensors
        B, K = qc.shape
        g = gloss.to(qc.device, torch.float32).contiguous()          # read by the kernel through its device pointer
        gq = torch.empty_like(qc)
        check(_lib.lib().ssg_dec_kl_loss_grad_f32(ptr(qc), B, K, ptr(g), ptr(gq), stream()), "ssg_dec_kl_loss_grad_f32")
        return gq.to(device=ctx.src[0], dtype=ctx.src[1])


def kl_loss(q):
    """nn.KLDivLoss(size_average=False)(q.log(), target_distribution(q)) / q.shape[0] with p not detached, as FinedTrainer2 /
    JointTrainer2._forward form it: q [B, K] -> 0-dim float32 on the GPU, differentiable with respect to q through both paths.
    q > 0 is taken for granted (the soft assignment never gives 0); an entry of 0 contributes 0."""
    return _KLFn.apply(_check_q(q, "kl_loss"))


def use_device_assignment(model):
    """Replace `model.assignment` (or `model.module.assignment` under nn.DataParallel) of the reference's torch model by the device
    module.  The Parameter object is kept, so optimiser groups built before the call and the state-dict key
    `assignment.cluster_centers` stay valid.  Returns the model."""
    host = model if hasattr(model, "assignment") else getattr(model, "module", None)
    if host is None or not hasattr(host, "assignment"):
        raise ValueError("the model has no `assignment` module (create it with cluster=True)")
    old = host.assignment
    centers = old.cluster_centers
    if centers.dim() != 2 or centers.shape[0] > MAX_K:
        raise ValueError("cluster_centers must be [K <= %d, D] (got %r)" % (MAX_K, tuple(centers.shape)))
    host.assignment = ClusterAssignment(centers.shape[0], centers.shape[1], cluster_centers=centers)
    return model
