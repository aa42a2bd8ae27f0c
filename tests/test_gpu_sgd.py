"""GPU half of the SGD tests: ssg_amd.SGD / ssg_sgd_step_f32 against torch.optim.SGD(foreach=False) on float32 CPU copies of the same
parameters and gradients (tests/sgd_ref.py), bit for bit, parameters and momentum buffers after every one of three steps (the first
step writes the buffers, the later ones read them).  CHUNK, T and CAP are read from the library, so the cases stay on both sides of
every launch limit whatever values the library is built with."""
import copy
import ctypes
import os
import sys
from functools import lru_cache

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgd_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
CL = torch.channels_last
STEPS = 3


@lru_cache(maxsize=None)
def limits():
    """(CHUNK, T, CAP): elements per chunk, descriptors per launch, chunks per launch"""
    from ssg_amd import _lib
    L = _lib.lib()
    return L.ssg_sgd_chunk_elems(), L.ssg_sgd_max_tensors_per_launch(), L.ssg_sgd_max_chunks_per_launch()


def cuda(t, i=0):
    return t.cuda()


def shifted(t, i=0):
    """a device copy of t one element into its storage: 4-byte aligned and no more"""
    v = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def device_sgd(pgs, **kw):
    import ssg_amd
    return ssg_amd.SGD(pgs, **kw)


def check(groups, grads, place=cuda, place_grad=None, between=None, nan_ok=False, make=device_sgd, **defaults):
    """the device run equals the CPU run after every step; returns the device optimiser"""
    opt, got = ref.run(make, groups, grads, place=place, place_grad=place_grad, between=between, **defaults)
    ref.same(got, ref.reference(groups, grads, between=between, **defaults), nan_ok=nan_ok)
    return opt


def case(seed, sizes, steps=STEPS):
    return ref.randn(seed, *sizes), ref.step_grads(seed, sizes, steps)


# ---- sizes, alignment, launch cuts ----------------------------------------------------------------------------------------------------

def test_sizes_in_one_optimiser():
    CHUNK, _, _ = limits()
    sizes = ref.SMALL_SIZES + (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
    tensors, grads = case(31, sizes)
    kept = []
    opt = check(tensors, grads, place_grad=lambda t, i: kept.append(t.cuda()) or kept[-1], **ref.VARIANTS["plain"])
    params = opt.param_groups[0]["params"]
    for p, g, src in zip(params, kept[-len(params):], grads[-1]):
        assert p.grad is g and ref.bit_equal(g.cpu(), src)               # the gradient is not written
        assert p._version >= STEPS                                       # autograd is told that the parameter changed


@pytest.mark.parametrize("which", ["p", "g", "p_and_g", "buf", "all"])
def test_scalar_and_vector_path_give_the_same_bits(which):
    """p, g and buf one element off 16-byte alignment, independently; the buffer arrives that way through a loaded state"""
    CHUNK, _, _ = limits()
    tensors, grads = case(32, (7, CHUNK + 5))

    def load_shifted_buffers(opt, k):
        if k != 1 or which not in ("buf", "all"):
            return
        sd = opt.state_dict()
        for s in sd["state"].values():
            s["momentum_buffer"] = shifted(s["momentum_buffer"])
        opt.load_state_dict(sd)
        assert all(opt.state[p]["momentum_buffer"].data_ptr() % 16 == 4 for p in opt.param_groups[0]["params"])

    def between(opt, k):
        if opt.param_groups[0]["params"][0].is_cuda:                     # the CPU run keeps its buffers
            load_shifted_buffers(opt, k)

    check(tensors, grads, place=shifted if which in ("p", "p_and_g", "all") else cuda,
          place_grad=shifted if which in ("g", "p_and_g", "all") else cuda, between=between, **ref.VARIANTS["plain"])


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("small", ["T-1", "T", "T+1", "2T+1"])
def test_launch_cut_by_tensor_count(small, where):
    """T - 1, T, T + 1 and 2 T + 1 tensors of 1 to 9 elements and one of CHUNK + 1: the cut falls before, on and after every position"""
    CHUNK, T, _ = limits()
    n = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}[small]
    sizes = [1 + i % 9 for i in range(n)]
    sizes.insert({"first": 0, "middle": n // 2, "last": n}[where], CHUNK + 1)
    tensors, grads = case(33, sizes)
    check(tensors, grads, **ref.VARIANTS["plain"])


@pytest.fixture(scope="module")
def cap_case():
    """tensors of 5, CAP * CHUNK and 5 elements, their gradients and the CPU run; made once for both cases below, dropped after them"""
    CHUNK, _, CAP = limits()
    tensors, grads = case(34, (5, CAP * CHUNK, 5))
    return tensors, grads, ref.reference(tensors, grads, **ref.VARIANTS["plain"])


@pytest.mark.parametrize("side", ["at_the_cap", "over_the_cap"])
def test_launch_cut_by_chunk_count(side, cap_case):
    """CAP chunks in one launch; and one chunk before them, so that the large tensor is cut inside: CAP - 1 chunks close the first
    launch and its last chunk opens the second"""
    tensors, grads, full = cap_case
    if side == "over_the_cap":
        got = ref.run(device_sgd, tensors, grads, place=cuda, **ref.VARIANTS["plain"])[1]
        ref.same(got, full)
    else:
        got = ref.run(device_sgd, tensors[1:2], [g[1:2] for g in grads], place=cuda, **ref.VARIANTS["plain"])[1]
        ref.same(got, [([p[1]], [b[1]]) for p, b in full])               # element-wise: the tensor's own run is the same alone


# ---- hyper-parameters and control flow -----------------------------------------------------------------------------------------------

def test_two_groups_one_without_momentum():
    CHUNK, _, _ = limits()
    sizes = (5, 257, CHUNK + 1, 3, 256, CHUNK + 7)
    tensors, grads = case(35, sizes)
    groups = [dict(params=tensors[:3], lr=0.1, weight_decay=5e-4, momentum=0.9), dict(params=tensors[3:], lr=0.03, weight_decay=1e-2, momentum=0)]
    opt = check(groups, grads, lr=1.0)
    assert all("momentum_buffer" in opt.state[p] for p in opt.param_groups[0]["params"])
    assert not any(p in opt.state and "momentum_buffer" in opt.state[p] for p in opt.param_groups[1]["params"])      # no buffer is made there


@pytest.mark.parametrize("variant", sorted(ref.VARIANTS))
def test_each_hyper_parameter_on_its_own(variant):
    CHUNK, _, _ = limits()
    tensors, grads = case(36, ref.SMALL_SIZES + (CHUNK + 1,))
    check(tensors, grads, **ref.VARIANTS[variant])


def test_a_parameter_without_a_gradient_and_a_late_first_gradient():
    """parameter 1 never has a gradient; parameter 3 gets its first one at step 2, so `first` is per tensor and per step"""
    CHUNK, _, _ = limits()
    tensors, grads = case(37, (6, 300, CHUNK + 1, 9, 5))
    for k in range(STEPS):
        grads[k][1] = None
    grads[0][3] = None
    opt = check(tensors, grads, **ref.VARIANTS["plain"])
    assert opt.param_groups[0]["params"][1] not in opt.state


def test_lr_rewritten_between_steps_through_lr_mult():
    """the reference's adjust_lr (selftraining.py:164-172): g['lr'] = lr * g.get('lr_mult', 1)"""
    tensors, grads = case(38, (40, 257, 5, 1000))
    groups = [dict(params=tensors[:2], lr_mult=0.1), dict(params=tensors[2:], lr_mult=1.0)]

    def adjust_lr(opt, k):
        lr = 0.1 * (0.1 ** k)
        for g in opt.param_groups:
            g["lr"] = lr * g.get("lr_mult", 1)

    opt = check(groups, grads, between=adjust_lr, **ref.REFERENCE_DEFAULTS)
    assert [g["lr_mult"] for g in opt.param_groups] == [0.1, 1.0]


def test_use_device_sgd_continues_from_torchs_buffers():
    """one step of torch.optim.SGD on the GPU, then use_device_sgd: the later steps equal those of a CPU optimiser that starts from the
    device's parameters and buffers after that first step"""
    import ssg_amd
    CHUNK, _, _ = limits()
    tensors, grads = case(39, (5, 257, CHUNK + 1))
    calls = []

    def swap(opt, k):
        if k == 1:
            assert type(opt) is torch.optim.SGD and ssg_amd.use_device_sgd(opt) is opt
            opt.register_step_post_hook(lambda *a: calls.append(k))
        assert type(opt) is (torch.optim.SGD if k == 0 else ssg_amd.SGD)

    opt, got = ref.run(lambda pgs, **kw: torch.optim.SGD(pgs, **kw), tensors, grads, place=cuda, between=swap, **ref.VARIANTS["plain"])
    assert calls == [1, 1]                                               # steps 2 and 3 ran the hook once each
    after_first = got[0]
    cpu = [torch.nn.Parameter(p.clone()) for p in after_first[0]]
    cpu_opt = ref.torch_sgd(cpu, **ref.VARIANTS["plain"])
    for p, b in zip(cpu, after_first[1]):
        cpu_opt.state[p]["momentum_buffer"] = b.clone()
    want = []
    for gk in grads[1:]:
        for p, g in zip(cpu, gk):
            p.grad = g.clone()
        cpu_opt.step()
        want.append(ref.snapshot(cpu_opt))
    ref.same(got[1:], want)


# ---- layout ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["cl_gradient", "contiguous_gradient", "loaded_contiguous_buffer"])
def test_channels_last_parameter(what):
    """the buffer is made in the parameter's layout; a gradient or a loaded buffer in another layout is laid out like the parameter
    once, and `.grad` itself stays as it was"""
    shapes = ((2, 3, 2, 2), (5, 8, 3, 3))
    tensors, grads = case(40, shapes)
    kept = []

    def place_grad(t, i):
        g = t.cuda().contiguous(memory_format=CL) if what == "cl_gradient" else t.cuda()
        kept.append((g, g.clone(), g.stride()))
        return g

    def between(opt, k):
        ps = opt.param_groups[0]["params"]
        if k != 1 or what != "loaded_contiguous_buffer" or not ps[0].is_cuda:
            return
        sd = opt.state_dict()
        for s in sd["state"].values():
            s["momentum_buffer"] = s["momentum_buffer"].contiguous()
        opt.load_state_dict(sd)
        assert all(opt.state[p]["momentum_buffer"].is_contiguous() and not opt.state[p]["momentum_buffer"].is_contiguous(memory_format=CL) for p in ps)

    opt, got = ref.run(device_sgd, tensors, grads, place=lambda t, i: t.cuda().contiguous(memory_format=CL), place_grad=place_grad, between=between,
                       **ref.VARIANTS["plain"])
    ref.same(got, ref.reference(tensors, grads, **ref.VARIANTS["plain"]))
    ps = opt.param_groups[0]["params"]
    assert ps[0].stride() == (12, 1, 6, 3)
    for p in ps:
        assert p.is_contiguous(memory_format=CL) and opt.state[p]["momentum_buffer"].stride() == p.stride()
    for (g, before, stride), p in zip(kept[-len(ps):], ps):
        assert p.grad is g and g.stride() == stride and ref.bit_equal(g, before)


# ---- non-finite values, the ABI called directly ------------------------------------------------------------------------------------

def test_non_finite_gradients():
    CHUNK, _, _ = limits()
    tensors, grads = case(41, (9, CHUNK + 5))
    spots = {0: float("inf"), 3: float("-inf"), 5: float("nan")}
    for i, g in enumerate(grads[0]):
        for at, v in spots.items():
            g[at + (0 if i == 0 else CHUNK - 2)] = v                     # in the float4 part, and across the end of the first chunk
    opt, got = ref.run(device_sgd, tensors, grads, place=cuda, **ref.VARIANTS["plain"])
    want = ref.reference(tensors, grads, **ref.VARIANTS["plain"])
    ref.same(got, want, nan_ok=True)                                     # the NaNs coincide; everything else, infinities included, is bit-equal
    p_first = got[0][0][1]
    base = CHUNK - 2
    assert p_first[base + 0] == float("-inf") and p_first[base + 3] == float("inf") and p_first[base + 5].isnan()
    assert int(got[0][0][1].isnan().sum()) == 1 and int(got[0][0][0].isnan().sum()) == 1


def test_abi_first_flag_is_per_tensor():
    """two tensors whose buffers hold NaN, `first` set on the first only: it is overwritten without being read, the other turns NaN"""
    from ssg_amd import _lib
    L = _lib.lib()
    n = 300
    p = [t.cuda() for t in ref.randn(42, n, n)]
    g = [t.cuda() for t in ref.randn(43, n, n)]
    buf = [torch.full((n,), float("nan"), device="cuda") for _ in range(2)]
    p0 = [t.clone() for t in p]
    ptrs = lambda ts: (ctypes.c_void_p * 2)(*[t.data_ptr() for t in ts])                          # noqa: E731
    one = lambda v: (ctypes.c_double * 1)(v)                                                      # noqa: E731
    rc = L.ssg_sgd_step_f32(ptrs(p), ptrs(g), ptrs(buf), (ctypes.c_int64 * 2)(n, n), (ctypes.c_int * 2)(0, 0), (ctypes.c_int * 2)(1, 0), 2,
                            one(0.1), one(0.9), one(0.0), one(0.0), (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(0), 1, _lib.stream())
    assert rc == 0, L.ssg_last_error()
    torch.cuda.synchronize()
    assert ref.bit_equal(buf[0], g[0]) and bool(torch.isfinite(p[0]).all()) and not torch.equal(p[0], p0[0])
    assert bool(buf[1].isnan().all()) and bool(p[1].isnan().all())
    assert L.ssg_sgd_step_f32(None, None, None, None, None, None, 0, None, None, None, None, None, None, 0, _lib.stream()) == 0


# ---- the real shape list --------------------------------------------------------------------------------------------------------------

def test_resnet50_shape_list():
    """the ~160 tensors of the reference's model (the largest 2048 x 2048) in the reference's two groups, two steps: multi-million-element
    tensors inside a call of several launches"""
    base, new = ref.resnet50_shapes()
    assert len(base) + len(new) == 162 and max(torch.Size(s).numel() for s in base + new) == 2048 * 2048
    tensors, grads = case(44, base + new, steps=2)
    groups = [dict(params=tensors[:len(base)], lr_mult=0.1, lr=0.01), dict(params=tensors[len(base):], lr_mult=1.0)]
    check(groups, grads, **ref.REFERENCE_DEFAULTS)


# ---- composition ------------------------------------------------------------------------------------------------------------------------

def _train_three_steps(mirror):
    """three steps of ssg_amd.SGD on the look-alike model of tests/head_ref.py with every device layer swapped in; with `mirror` the
    device gradients of each step also go to a CPU clone stepped by torch.optim.SGD, which must agree after each step.  Returns the
    parameters, the momentum buffers and the BatchNorm statistics."""
    import ssg_amd
    import test_gpu_head as head_suite
    model, x, coef = head_suite._comp_data()
    m = copy.deepcopy(model).cuda()
    ssg_amd.use_device_conv(m, strided=True)
    ssg_amd.use_device_maxpool(m)
    ssg_amd.use_device_batchnorm(m)
    ssg_amd.use_device_head(m)
    m = m.to(memory_format=CL).train()
    xd, coefd = x.cuda().contiguous(memory_format=CL), [c.cuda() for c in coef]
    split = lambda named: ([p for n, p in named if n.startswith("base.")], [p for n, p in named if not n.startswith("base.")])      # noqa: E731
    hyper = dict(lr=0.01, momentum=0.9, weight_decay=5e-4)
    groups = lambda ps: [dict(params=ps[0], lr_mult=0.1, lr=0.001), dict(params=ps[1], lr_mult=1.0)]                                  # noqa: E731
    named = list(m.named_parameters())
    opt = ssg_amd.SGD(groups(split(named)), **hyper)
    if mirror:
        twins = [(n, torch.nn.Parameter(p.detach().cpu().clone())) for n, p in named]
        cpu_opt = ref.torch_sgd(groups(split(twins)), **hyper)
    for k in range(STEPS):
        opt.zero_grad()
        head_suite._comp_backward(m, xd, coefd)
        assert sum(p.grad is not None for _, p in named) > 10 and any(p.grad is None for _, p in named)       # base.fc is outside the forward
        if mirror:
            for (_, p), (_, q) in zip(named, twins):
                q.grad = None if p.grad is None else p.grad.detach().cpu().clone()
        opt.step()
        if mirror:
            cpu_opt.step()
            for (n, p), (_, q) in zip(named, twins):
                assert bool(torch.isfinite(q).all()) and ref.bit_equal(p.detach().cpu(), q.detach()), "step %d %s" % (k, n)
    out = {"p." + n: p.detach().clone() for n, p in named}
    out.update({"buf." + n: opt.state[p]["momentum_buffer"].clone() for n, p in named if p in opt.state})
    out.update({"bn." + n: b.clone() for n, b in m.named_buffers()})
    return out


def test_whole_training_step_is_reproducible_and_equals_torchs_update():
    a, b = _train_three_steps(mirror=True), _train_three_steps(mirror=False)
    assert sorted(a) == sorted(b) and any(k.startswith("buf.") for k in a) and any(k.startswith("bn.") for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), k
