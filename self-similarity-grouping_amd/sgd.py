"""The optimiser step of the fine-tune phase on the GPU: torch.optim.SGD in one multi-tensor kernel (csrc/sgd.hip).

The reference builds `torch.optim.SGD(param_groups, lr, momentum=0.9, weight_decay)` over about 160 parameter tensors in two groups that
carry an extra `lr_mult` key, rewrites `g['lr']` between epochs (`adjust_lr`) and freezes the classifier (selftraining.py:152-172,
semitraining.py:162).  torch runs that step as a chain of `_foreach_*` passes.  Here one `ssg_sgd_step_f32` call updates every
parameter that has a gradient, in one pass over p, g and buf and a launch per 64 tensors, with torch's own float32 arithmetic:

    g = maximize ? -g : g;   g = weight_decay != 0 ? fma(weight_decay, p, g) : g
    momentum != 0:   buf = first ? g : fma(1 - dampening, g, momentum * buf);   g = nesterov ? fma(momentum, buf, g) : buf
    p = fma(-lr, g, p)

    opt = SGD(param_groups, lr, momentum=0.9, weight_decay=5e-4)     torch.optim.SGD with that step; everything else is inherited
    use_device_sgd(optimizer)                                        a built torch.optim.SGD becomes one in place

The parameters and buffers after a step are bit for bit those of torch.optim.SGD on the CPU.  There is no CPU fallback: a step that
has a gradient to apply needs the parameters on one GPU; a step without any gradient launches nothing."""
import functools
import inspect
from array import array

import torch

from . import _lib, _train
from ._lib import check, stream

__all__ = ["SGD", "use_device_sgd"]

_STEP = "ssg_amd.SGD.step"


def _group_rule(group, i=None):
    """None when a parameter group (or the constructor's arguments) can be stepped on the device, else the rule it breaks (one line)"""
    why = None
    if group.get("differentiable"):
        why = "differentiable=True is not supported (the step runs outside autograd)"
    for key in ("lr", "weight_decay"):
        if why is None and isinstance(group[key], torch.Tensor):
            why = "a tensor %s is not supported (it would be read on the host every step); pass a float" % key
    return why if why is None or i is None else "param_groups[%d]: %s" % (i, why)


def _dense(t):
    """t covers one block of memory exactly once (any permutation of a contiguous tensor)"""
    expect = 1
    for n, s in sorted(((n, s) for n, s in zip(t.shape, t.stride()) if n > 1), key=lambda ns: ns[1]):
        if s != expect:
            return False
        expect *= n
    return True


def _same_layout(a, b):
    return all(sa == sb for sa, sb, n in zip(a.stride(), b.stride(), a.shape) if n > 1)


class _Known(object):
    """what `step` has checked of a parameter (held, so that its id stays its own), and the momentum buffer it made or took over"""
    __slots__ = ("p", "ptr", "shape", "stride", "numel", "device", "buf", "buf_ptr")

    def __init__(self, p):
        self.p, self.ptr, self.shape, self.stride, self.numel, self.device = p, p.data_ptr(), p.shape, p.stride(), p.numel(), p.device
        self.buf = self.buf_ptr = None


class SGD(torch.optim.SGD):
    """torch.optim.SGD (same constructor, `param_groups` with any extra keys, `state[p]['momentum_buffer']`, state dicts, `zero_grad`,
    `add_param_group`, hooks and lr schedulers) whose `step` is one `ssg_sgd_step_f32` call.  A state dict moves between the two classes
    in both directions.  `foreach` and `fused` are accepted and ignored; `differentiable=True`, a tensor `lr` and a tensor
    `weight_decay` raise ValueError."""

    @functools.wraps(torch.optim.SGD.__init__)
    def __init__(self, params, *args, **kwargs):
        given = inspect.signature(torch.optim.SGD.__init__).bind(self, params, *args, **kwargs)
        given.apply_defaults()
        _train.refuse("ssg_amd.SGD", _group_rule(given.arguments))
        kwargs.pop("foreach", None)
        kwargs.pop("fused", None)
        super(SGD, self).__init__(params, *args, **kwargs)

    def _learn(self, known, p, gi, pi):
        """check a parameter met for the first time, or whose storage changed, and remember what the later steps rely on"""
        why = None
        if not p.is_cuda:
            why = "the parameter must be on a GPU (got %s; there is no CPU fallback)" % (p.device,)
        elif p.dtype != torch.float32:
            why = "the parameter must be float32 (got %s)" % (p.dtype,)
        elif p.numel() and not _dense(p):
            why = "the parameter must be dense in memory (shape %r, strides %r)" % (tuple(p.shape), tuple(p.stride()))
        _train.refuse(_STEP, None if why is None else "param_groups[%d]['params'][%d]: %s" % (gi, pi, why))
        rec = known[id(p)] = _Known(p)
        return rec

    def step(self, closure=None):
        """One SGD step of every parameter that has a gradient, on the current stream of the parameters' GPU; returns the closure's
        loss.  The hyper-parameters of every group are read now.  New momentum buffers are `torch.empty_like(p)`, in p's layout; a
        gradient in another layout is copied once into p's layout (`.grad` itself is neither replaced nor written), a loaded buffer in
        another layout is converted once and its state entry replaced.  Parameters must be float32, dense and on one GPU, gradients
        dense tensors: anything else raises ValueError naming the group and the position, before anything is changed.  What a step
        has checked of a parameter is checked again only when its storage changes; gradients and state entries are looked at afresh
        every step.  No host read, no synchronisation."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        known = self.__dict__.setdefault("_ssg_known", {})
        state, groups, f32 = self.state, self.param_groups, torch.float32
        p_ptr, g_ptr, b_ptr, numel, group, touched = [], [], [], [], [], []
        later = []                                   # (position, parameter, gradient or None, buffer or None): what needs a new tensor
        dev = None
        for gi, grp in enumerate(groups):
            _train.refuse(_STEP, _group_rule(grp, gi))
            momentum = grp["momentum"] != 0
            for pi, p in enumerate(grp["params"]):
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    _train.refuse(_STEP, "param_groups[%d]['params'][%d]: a sparse gradient is not supported" % (gi, pi))
                rec = known.get(id(p))
                if rec is None or rec.p is not p or p.data_ptr() != rec.ptr:
                    rec = self._learn(known, p, gi, pi)
                # the gradient: torch keeps a dense .grad at its parameter's dtype, device and shape; the checks guard a parameter
                # whose data was replaced under a gradient that stayed
                why = relaid = None
                if g.dtype != f32 or g.device != rec.device or g.shape != rec.shape:
                    why = "the gradient must be float32, on the parameter's GPU and of its shape (got %s, %s, %r)" % (g.dtype, g.device, tuple(g.shape))
                elif dev is not None and rec.device != dev:
                    why = "every parameter must be on the same GPU (got %s after %s)" % (rec.device, dev)
                elif g.stride() != rec.stride and not _same_layout(g, p):
                    relaid = g
                buf = fresh = None
                if why is None and momentum:
                    entry = state.get(p)
                    buf = None if entry is None else entry.get("momentum_buffer")
                    if buf is None or buf is not rec.buf or buf.data_ptr() != rec.buf_ptr:      # not the one this class made or took over
                        if buf is not None and (buf.device != rec.device or buf.dtype != f32 or buf.shape != rec.shape):
                            why = "its momentum buffer must be float32, on the parameter's GPU and of its shape (got %s, %s, %r)" % (
                                buf.dtype, buf.device, tuple(buf.shape))
                        fresh = True
                if why is not None:
                    _train.refuse(_STEP, "param_groups[%d]['params'][%d]: %s" % (gi, pi, why))
                dev = rec.device
                if not rec.numel:
                    continue
                if relaid is not None or fresh:
                    later.append((len(p_ptr), p, relaid, buf, rec))
                p_ptr.append(rec.ptr); g_ptr.append(g.data_ptr()); b_ptr.append((rec.buf_ptr or 0) if momentum else 0)
                numel.append(rec.numel); group.append(gi); touched.append(p)
                if momentum:
                    touched.append(buf)
        n, k = len(p_ptr), len(groups)
        if not n:
            return loss
        first = [0] * n
        scratch = []                                 # gradients laid out like their parameters live until the launch is queued
        with torch.no_grad():
            for at, p, relaid, buf, rec in later:
                if relaid is not None:
                    scratch.append(torch.empty_like(p).copy_(relaid))
                    g_ptr[at] = scratch[-1].data_ptr()
                if groups[group[at]]["momentum"] != 0:
                    if buf is None:
                        first[at] = 1
                        buf = state[p]["momentum_buffer"] = torch.empty_like(p)
                    elif not _same_layout(buf, p):
                        buf = state[p]["momentum_buffer"] = torch.empty_like(p).copy_(buf)
                    rec.buf, rec.buf_ptr = buf, buf.data_ptr()
                    b_ptr[at] = rec.buf_ptr
        if later:
            touched = [t for t in touched if t is not None] + [rec.buf for _, _, _, _, rec in later if rec.buf is not None]
        # the host arrays of the call, as array.array: built from a list several times faster than a ctypes array
        arrays = [array("Q", p_ptr), array("Q", g_ptr), array("Q", b_ptr), array("q", numel), array("i", group), array("i", first),
                  array("d", [g["lr"] for g in groups]), array("d", [g["momentum"] for g in groups]), array("d", [g["dampening"] for g in groups]),
                  array("d", [g["weight_decay"] for g in groups]), array("i", [bool(g["nesterov"]) for g in groups]),
                  array("i", [bool(g["maximize"]) for g in groups])]
        a = [x.buffer_info()[0] for x in arrays]
        with torch.cuda.device(dev):
            check(_lib.lib().ssg_sgd_step_f32(a[0], a[1], a[2], a[3], a[4], a[5], n, a[6], a[7], a[8], a[9], a[10], a[11], k, stream()), "ssg_sgd_step_f32")
        torch.autograd.graph.increment_version(touched)           # the kernel wrote them behind autograd's back
        return loss


def use_device_sgd(optimizer):
    """Turn a built `torch.optim.SGD` into an `ssg_amd.SGD` in place: its class is swapped and `step` gets the hook wrapper the
    constructor would have given it, so pre- and post-step hooks run once per step; the parameter groups (with extra keys such as
    `lr_mult`), the state and the registered hooks are kept.  Call it before an lr scheduler is built on the optimiser: a scheduler
    binds the optimiser's `step` of that moment.  An `ssg_amd.SGD` is returned as it is.  Any other type (subclasses of
    torch.optim.SGD included), `differentiable=True`, a tensor `lr` or `weight_decay`, or an lr scheduler already attached raise
    ValueError and change nothing.  Returns the optimiser."""
    fn = "use_device_sgd"
    if isinstance(optimizer, SGD):
        return optimizer
    if type(optimizer) is not torch.optim.SGD:
        raise ValueError("%s: the optimiser must be a torch.optim.SGD itself, not a subclass or another optimiser (got %s)"
                         % (fn, type(optimizer).__name__))
    for gi, group in enumerate(optimizer.param_groups):
        _train.refuse(fn, _group_rule(group, gi))
    if "step" in vars(optimizer):
        raise ValueError("%s: an lr scheduler has already bound this optimiser's step; call %s before building the scheduler" % (fn, fn))
    optimizer.__class__ = SGD
    optimizer._patch_step_function()
    return optimizer
