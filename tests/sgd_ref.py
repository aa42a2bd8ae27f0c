"""Yardstick of the SGD tests (tests/test_sgd_host.py, tests/test_gpu_sgd.py): torch's own CPU optimiser, bit for bit.

    run(optimiser class, groups, gradients per step, ...)   builds the parameters from float32 CPU tensors, takes the steps and returns
                                                            the parameters and momentum buffers after every step, as CPU tensors
    reference(...)                                          that with torch.optim.SGD(foreach=False) on the CPU
    restated(...)                                           the same steps by a float64 restatement of the fused arithmetic

The update is element-wise and its rounding is fixed (include/ssg_hip.h: every add(., alpha=.) one fused multiply-add, momentum * buf
rounded on its own, every hyper-parameter rounded from double to float32 once), so no tolerance is involved: a comparison is of
the bits.  The restatement forms a * b + c in float64: the product of two float32 values is exact there and the sum is rounded
twice, to float64 and then to float32.  The second rounding can differ from a single one only when the float64 sum falls exactly
half-way between two float32 values, which random data meets about once in 2^29 elements; the host suite keeps its cases below 2^12
elements so that this stays out of reach."""
import torch

# the reference's optimiser (selftraining.py:152-161): two groups told apart by lr_mult, momentum 0.9, weight decay 5e-4
REFERENCE_DEFAULTS = dict(lr=0.1, momentum=0.9, weight_decay=5e-4)

# the hyper-parameter variants both suites cross, each on its own
VARIANTS = {
    "plain": dict(lr=0.1, momentum=0.9, weight_decay=5e-4),
    "nesterov": dict(lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True),
    "dampening": dict(lr=0.1, momentum=0.9, dampening=0.1, weight_decay=5e-4),
    "maximize": dict(lr=0.1, momentum=0.9, weight_decay=5e-4, maximize=True),
    "no_decay": dict(lr=0.1, momentum=0.9, weight_decay=0),
    "lr_zero": dict(lr=0.0, momentum=0.9, weight_decay=5e-4),
    "no_momentum": dict(lr=0.05, momentum=0, weight_decay=1e-3),
}
SMALL_SIZES = (1, 3, 4, 5, 255, 256, 257)


def randn(seed, *shapes):
    """float32 CPU tensors of these shapes from one seeded generator"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*((s,) if isinstance(s, int) else tuple(s)), generator=g, dtype=torch.float32) for s in shapes]


def step_grads(seed, shapes, steps):
    """[step][tensor] gradients"""
    return [randn(seed + 1000 * (k + 1), *shapes) for k in range(steps)]


def snapshot(opt):
    """([parameter], [momentum buffer or None]) as CPU clones, in group order"""
    ps = [p for g in opt.param_groups for p in g["params"]]
    bufs = [opt.state[p].get("momentum_buffer") if p in opt.state else None for p in ps]
    return [p.detach().cpu().clone() for p in ps], [None if b is None else b.detach().cpu().clone() for b in bufs]


def run(make, groups, grads, place=lambda t, i: t.clone(), place_grad=None, between=None, **defaults):
    """`groups`: a list of dicts with 'params' (float32 CPU tensors; never modified) and any per-group options, or a plain list of
    tensors for one group.  `grads[k][i]` is the gradient of parameter i (numbered through the groups) at step k, or None.
    `place(t, i)` makes the parameter's data from the CPU tensor (a copy: on a device, at a storage offset, in a layout), `place_grad`
    likewise for gradients (default: like `place`).  `make(param_groups, **defaults)` builds the optimiser; `between(opt, k)` runs
    before step k.  Returns (optimiser, [snapshot after each step])."""
    if not isinstance(groups[0], dict):
        groups = [dict(params=list(groups))]
    place_grad = place_grad or place
    params, pgs, i = [], [], 0
    for g in groups:
        mine = []
        for t in g["params"]:
            mine.append(torch.nn.Parameter(place(t, i)))
            i += 1
        params += mine
        pgs.append(dict(g, params=mine))
    opt = make(pgs, **defaults)
    shots = []
    for k, gk in enumerate(grads):
        for i, p in enumerate(params):
            p.grad = None if gk[i] is None else place_grad(gk[i], i)
        if between is not None:
            between(opt, k)
        opt.step()
        shots.append(snapshot(opt))
    return opt, shots


def torch_sgd(pgs, **kw):
    return torch.optim.SGD(pgs, foreach=False, **kw)


def reference(groups, grads, between=None, **defaults):
    """the snapshots of torch.optim.SGD(foreach=False) on the CPU"""
    return run(torch_sgd, groups, grads, between=between, **defaults)[1]


def bit_equal(a, b, nan_ok=False):
    """the same shape and the same bits element by element (whatever the strides); with `nan_ok` the NaNs must sit at the same
    positions and their payloads are not compared"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if nan_ok:
        if not torch.equal(a.isnan(), b.isnan()):
            return False
        a, b = a.masked_fill(a.isnan(), 0.0), b.masked_fill(b.isnan(), 0.0)
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def same(got, ref, what="", nan_ok=False):
    """every parameter and buffer of every step is bit-equal"""
    assert len(got) == len(ref)
    for k, ((gp, gb), (rp, rb)) in enumerate(zip(got, ref)):
        assert len(gp) == len(rp) and len(gb) == len(rb)
        for i, (a, b) in enumerate(zip(gp, rp)):
            assert bit_equal(a, b, nan_ok), "%s step %d parameter %d (%s)" % (what, k, i, tuple(b.shape))
        for i, (a, b) in enumerate(zip(gb, rb)):
            assert (a is None) == (b is None), "%s step %d buffer %d: present in one run only" % (what, k, i)
            assert a is None or bit_equal(a, b, nan_ok), "%s step %d buffer %d (%s)" % (what, k, i, tuple(b.shape))


# ---- the float64 restatement -----------------------------------------------------------------------------------------------------------

def _f32(x):
    return torch.tensor(x, dtype=torch.float64).float().double()         # a hyper-parameter: double -> float32 once


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def restated_step(p, g, buf, lr=0.0, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False):
    """(p, buf) after one step, float32 tensors; buf None when there is no buffer yet (and None back without momentum)"""
    if maximize:
        g = -g
    if weight_decay != 0:
        g = _fma(_f32(weight_decay), p, g)
    if momentum != 0:
        buf = g.clone() if buf is None else _fma(_f32(1.0 - dampening), g, (_f32(momentum) * buf.double()).float())
        g = _fma(_f32(momentum), buf, g) if nesterov else buf
    return _fma(-_f32(lr), g, p), buf


def restated(tensors, grads, **hyper):
    """the snapshots of one group stepped by `restated_step`"""
    ps, bufs, shots = [t.clone() for t in tensors], [None] * len(tensors), []
    for gk in grads:
        for i, g in enumerate(gk):
            if g is not None:
                ps[i], bufs[i] = restated_step(ps[i], g, bufs[i], **hyper)
        shots.append(([p.clone() for p in ps], [None if b is None else b.clone() for b in bufs]))
    return shots


# ---- the real shape list -----------------------------------------------------------------------------------------------------------------

def resnet50_shapes(num_features=2048):
    """the parameter shapes of the reference's model in module order: torchvision's ResNet-50 without fc, then feat and feat_bn"""
    shapes = [(64, 3, 7, 7), (64,), (64,)]
    inplanes = 64
    for planes, blocks in ((64, 3), (128, 4), (256, 6), (512, 3)):
        for b in range(blocks):
            shapes += [(planes, inplanes, 1, 1), (planes,), (planes,), (planes, planes, 3, 3), (planes,), (planes,),
                       (planes * 4, planes, 1, 1), (planes * 4,), (planes * 4,)]
            if b == 0:
                shapes += [(planes * 4, inplanes, 1, 1), (planes * 4,), (planes * 4,)]
            inplanes = planes * 4
    return shapes, [(num_features, inplanes), (num_features,), (num_features,)]
