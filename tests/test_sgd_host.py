"""Host half of the SGD tests (no GPU): the names and the constructor's signature, the pin of the yardstick (torch's CPU SGD equals the
float64 restatement of the fused arithmetic, tests/sgd_ref.py), the argument checks of ssg_sgd_step_f32 that come before any launch,
the refusals of the Python layer, and what both construction routes (ssg_amd.SGD and use_device_sgd) owe the rest of torch: hooks,
closures, lr schedulers and state dicts."""
import ctypes
import inspect
import os
import sys
import warnings

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgd_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def L():
    from ssg_amd import _lib
    return _lib.lib()


def test_names_and_signature():
    import ssg_amd
    assert callable(ssg_amd.SGD) and callable(ssg_amd.use_device_sgd)
    assert issubclass(ssg_amd.SGD, torch.optim.SGD) and ssg_amd.SGD is not torch.optim.SGD
    assert inspect.signature(ssg_amd.SGD.__init__) == inspect.signature(torch.optim.SGD.__init__)
    assert inspect.signature(ssg_amd.SGD) == inspect.signature(torch.optim.SGD)
    # step is the only method of torch's class that is overridden (the constructor checks and forwards)
    assert sorted(n for n in vars(ssg_amd.SGD) if callable(vars(ssg_amd.SGD)[n]) and not n.startswith("_")) == ["step"]


@pytest.mark.parametrize("variant", sorted(ref.VARIANTS))
@pytest.mark.parametrize("foreach", [False, None])
def test_torch_cpu_sgd_is_the_fused_restatement(variant, foreach):
    """the yardstick pin: should a torch release change how its CPU SGD rounds, this says so here and not on the GPU"""
    sizes = ref.SMALL_SIZES + (1031,)
    tensors = ref.randn(11, *sizes)
    grads = ref.step_grads(12, sizes, 3)
    hyper = ref.VARIANTS[variant]
    got = ref.run(lambda pgs, **kw: torch.optim.SGD(pgs, foreach=foreach, **kw), tensors, grads, **hyper)[1]
    ref.same(got, ref.restated(tensors, grads, **hyper), "%s foreach=%s" % (variant, foreach))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------

def _abi_args(n=1, groups=1, **over):
    """well-formed arguments of ssg_sgd_step_f32 with made-up (never dereferenced) pointers; `over` replaces whole arguments"""
    ptrs = lambda base: (ctypes.c_void_p * n)(*[base + 64 * i for i in range(n)])      # noqa: E731
    a = dict(params=ptrs(0x1000), grads=ptrs(0x2000), bufs=ptrs(0x3000), numel=(ctypes.c_int64 * n)(*[8] * n),
             group=(ctypes.c_int * n)(*[0] * n), first=(ctypes.c_int * n)(*[0] * n), count=n,
             lr=(ctypes.c_double * groups)(*[0.1] * groups), momentum=(ctypes.c_double * groups)(*[0.9] * groups),
             dampening=(ctypes.c_double * groups)(*[0.0] * groups), weight_decay=(ctypes.c_double * groups)(*[5e-4] * groups),
             nesterov=(ctypes.c_int * groups)(*[0] * groups), maximize=(ctypes.c_int * groups)(*[0] * groups), num_groups=groups, stream=None)
    a.update(over)
    return list(a.values())


def _refused(L, word, **over):
    assert L.ssg_sgd_step_f32(*_abi_args(**over)) == -1, over
    msg = L.ssg_last_error().decode()
    assert "ssg_sgd_step_f32" in msg and word in msg, msg


def test_abi_limits(L):
    T, chunk, cap = L.ssg_sgd_max_tensors_per_launch(), L.ssg_sgd_chunk_elems(), L.ssg_sgd_max_chunks_per_launch()
    assert T > 0 and chunk > 0 and cap > 0
    assert chunk & (chunk - 1) == 0


def test_abi_refusals_come_before_any_launch(L):
    assert L.ssg_sgd_step_f32(*_abi_args(n=0)) == 0                                           # nothing to do, nothing launched
    assert L.ssg_sgd_step_f32(None, None, None, None, None, None, 0, None, None, None, None, None, None, 0, None) == 0
    for name in ("params", "grads", "bufs", "numel", "group", "first", "lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize"):
        _refused(L, "NULL array", **{name: None})
    _refused(L, "count", count=-1)
    _refused(L, "num_groups", num_groups=0)
    two = lambda a, b: (ctypes.c_void_p * 2)(a, b)                                                # noqa: E731
    _refused(L, "NULL parameter or gradient", n=2, params=two(0x1000, None))
    _refused(L, "NULL parameter or gradient", n=2, grads=two(None, 0x2000))
    _refused(L, "NULL momentum buffer", n=2, bufs=two(0x3000, None))
    for n in (0, -5):
        _refused(L, "n must be at least 1", numel=(ctypes.c_int64 * 1)(n))
    for g in (-1, 1, 7):
        _refused(L, "group index out of range", group=(ctypes.c_int * 1)(g))
    one = lambda v: (ctypes.c_double * 1)(v)                                                      # noqa: E731
    _refused(L, "nesterov requires", nesterov=(ctypes.c_int * 1)(1), momentum=one(0.0))
    _refused(L, "nesterov requires", nesterov=(ctypes.c_int * 1)(1), dampening=one(0.1))
    for name in ("lr", "momentum", "weight_decay"):
        for bad in (-0.1, float("inf"), float("-inf"), float("nan")):
            _refused(L, "finite and not negative", **{name: one(bad)})
    # the second group is checked like the first, and a buffer may be NULL where the group has no momentum
    _refused(L, "finite and not negative", groups=2, lr=(ctypes.c_double * 2)(0.1, -1.0))
    with pytest.raises(ValueError, match="ssg_sgd_step_f32"):
        from ssg_amd import _lib
        _lib.check(L.ssg_sgd_step_f32(*_abi_args(numel=(ctypes.c_int64 * 1)(0))), "ssg_sgd_step_f32")


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------

def _params(n=3):
    return [torch.nn.Parameter(t) for t in ref.randn(21, *[(4, 3)] * n)]


def _direct(params, **kw):
    import ssg_amd
    return ssg_amd.SGD(params, **kw)


def _swapped(params, **kw):
    import ssg_amd
    return ssg_amd.use_device_sgd(torch.optim.SGD(params, **kw))


ROUTES = {"constructed": _direct, "swapped": _swapped}


def test_constructor_refusals():
    import ssg_amd
    for kw, word in ((dict(lr=0.1, differentiable=True), "differentiable"), (dict(lr=torch.tensor(0.1)), "tensor lr"),
                     (dict(lr=0.1, weight_decay=torch.tensor(0.1)), "tensor weight_decay")):
        with pytest.raises(ValueError, match=word):
            ssg_amd.SGD(_params(), **kw)
    with pytest.raises(ValueError):                                                               # torch's own rules still hold
        ssg_amd.SGD(_params(), lr=-1.0)
    with pytest.raises(ValueError):
        ssg_amd.SGD(_params(), lr=0.1, nesterov=True)
    for kw in (dict(foreach=True), dict(foreach=False), dict(fused=True), dict(fused=False), dict(foreach=True, fused=True)):
        assert type(ssg_amd.SGD(_params(), lr=0.1, **kw)) is ssg_amd.SGD                          # accepted and ignored


def _state_of(opt):
    return type(opt), {k: {n: v.clone() for n, v in s.items()} for k, s in opt.state.items()}, [p.detach().clone() for g in opt.param_groups for p in g["params"]]


def _unchanged(opt, before):
    cls, state, params = before
    assert type(opt) is cls and set(opt.state) == set(state)
    for k, s in state.items():
        assert set(opt.state[k]) == set(s) and all(torch.equal(opt.state[k][n], v) for n, v in s.items())
    assert all(torch.equal(p, q) for p, q in zip((p for g in opt.param_groups for p in g["params"]), params))


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_step_refusals_change_nothing(route):
    """a CPU parameter with a gradient, a float64 parameter, a sparse gradient: ValueError naming the group and the position"""
    def cpu(p):
        p.grad = torch.ones_like(p)

    def double(p):
        p.data = p.data.double()
        p.grad = torch.ones_like(p)

    def sparse(p):
        p.grad = torch.ones_like(p).to_sparse()

    for spoil, word in ((cpu, "GPU"), (double, "GPU|float32"), (sparse, "sparse")):
        ps = _params()
        opt = ROUTES[route]([dict(params=ps[:1]), dict(params=ps[1:], lr=0.01)], lr=0.1, momentum=0.9)
        spoil(ps[2])                                                                              # params[1] of group 1
        before = _state_of(opt)
        with pytest.raises(ValueError, match=word) as e:
            opt.step()
        assert "param_groups[1]['params'][1]" in str(e.value) and "ssg_amd.SGD.step" in str(e.value)
        _unchanged(opt, before)
    # hyper-parameters written into a group after construction are read at call time
    ps = _params()
    opt = ROUTES[route](ps, lr=0.1)
    opt.param_groups[0]["lr"] = torch.tensor(0.1)
    with pytest.raises(ValueError, match="tensor lr"):
        opt.step()


def test_use_device_sgd_refusals_change_nothing():
    import ssg_amd

    class MySGD(torch.optim.SGD):
        pass

    for opt, word in ((torch.optim.Adam(_params(), lr=0.1), "Adam"), (MySGD(_params(), lr=0.1, momentum=0.9), "MySGD"),
                      (torch.optim.SGD(_params(), lr=0.1, differentiable=True), "differentiable"),
                      (torch.optim.SGD(_params(), lr=torch.tensor(0.1)), "tensor lr")):
        before = _state_of(opt)
        with pytest.raises(ValueError, match=word):
            ssg_amd.use_device_sgd(opt)
        _unchanged(opt, before)
    opt = torch.optim.SGD(_params(), lr=0.1)
    sched = torch.optim.lr_scheduler.StepLR(opt, 1)                                               # it has bound torch's step
    with pytest.raises(ValueError, match="scheduler"):
        ssg_amd.use_device_sgd(opt)
    assert type(opt) is torch.optim.SGD and sched.optimizer is opt


def test_use_device_sgd_keeps_state_and_groups_and_is_idempotent():
    import ssg_amd
    ps = _params()
    opt = torch.optim.SGD([dict(params=ps[:1], lr_mult=0.1), dict(params=ps[1:], lr_mult=1.0)], lr=0.1, momentum=0.9, weight_decay=5e-4)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()                                                                                    # torch's step on the CPU: buffers exist
    groups, state, bufs = opt.param_groups, opt.state, [opt.state[p]["momentum_buffer"] for p in ps]
    calls = []
    opt.register_step_post_hook(lambda *a: calls.append(1))
    assert ssg_amd.use_device_sgd(opt) is opt and type(opt) is ssg_amd.SGD
    assert opt.param_groups is groups and opt.state is state and all(opt.state[p]["momentum_buffer"] is b for p, b in zip(ps, bufs))
    assert [g["lr_mult"] for g in opt.param_groups] == [0.1, 1.0]
    step = type(opt).step
    assert ssg_amd.use_device_sgd(opt) is opt and type(opt) is ssg_amd.SGD and type(opt).step is step      # a second call changes nothing
    for p in ps:
        p.grad = None
    opt.step()
    assert calls == [1]                                                                           # a hook registered before the swap runs once


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_a_step_without_gradients_needs_no_gpu(route):
    ps = _params()
    opt = ROUTES[route]([dict(params=ps[:1], lr_mult=0.1), dict(params=ps[1:], lr_mult=1.0)], lr=0.1, momentum=0.9)
    before = [p.detach().clone() for p in ps]
    pre, post = [], []
    opt.register_step_pre_hook(lambda *a: pre.append(1))
    opt.register_step_post_hook(lambda *a: post.append(1))
    assert opt.step() is None
    assert (pre, post) == ([1], [1])                                                              # exactly once per step
    loss = opt.step(lambda: torch.tensor(3.5))
    assert float(loss) == 3.5 and (pre, post) == ([1, 1], [1, 1])
    assert all(torch.equal(p, q) for p, q in zip(ps, before)) and len(opt.state) == 0
    # the closure runs with gradients enabled even under no_grad, as torch's does
    with torch.no_grad():
        assert opt.step(lambda: torch.is_grad_enabled()) is True
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                                            # "lr_scheduler.step() before optimizer.step()"
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
        opt.step()
        sched.step()
    assert [g["lr"] for g in opt.param_groups] == [0.05, 0.05] and len(post) == 4


def test_state_dict_round_trip_both_ways():
    import ssg_amd
    ps = _params()
    groups = lambda q: [dict(params=q[:1], lr_mult=0.1), dict(params=q[1:], lr_mult=1.0, lr=0.01)]            # noqa: E731
    src = torch.optim.SGD(groups(ps), lr=0.1, momentum=0.9, weight_decay=5e-4)
    for p in ps:
        p.grad = torch.full_like(p, 0.5)
    src.step()
    sd = src.state_dict()
    ours = ssg_amd.SGD(groups(_params()), lr=0.3)
    ours.load_state_dict(sd)                                                                      # torch -> ssg_amd
    assert type(ours) is ssg_amd.SGD
    assert [g["lr_mult"] for g in ours.param_groups] == [0.1, 1.0] and [g["lr"] for g in ours.param_groups] == [0.1, 0.01]
    assert all(torch.equal(ours.state[q]["momentum_buffer"], src.state[p]["momentum_buffer"])
               for p, q in zip(ps, (q for g in ours.param_groups for q in g["params"])))
    back = torch.optim.SGD(groups(_params()), lr=0.7)
    back.load_state_dict(ours.state_dict())                                                       # ssg_amd -> torch
    a, b = back.state_dict(), sd
    assert [{k: v for k, v in g.items() if k not in ("foreach", "fused")} for g in a["param_groups"]] == \
           [{k: v for k, v in g.items() if k not in ("foreach", "fused")} for g in b["param_groups"]]
    assert a["state"].keys() == b["state"].keys()
    assert all(torch.equal(a["state"][k]["momentum_buffer"], b["state"][k]["momentum_buffer"]) for k in a["state"])
    for p in (q for g in back.param_groups for q in g["params"]):
        p.grad = torch.full_like(p, 0.5)
    back.step()                                                                                   # and torch steps on from it
