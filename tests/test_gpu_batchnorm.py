"""GPU suite of the train-mode batch norm (csrc/batchnorm.hip, ssg_amd/batchnorm.py): the entry points through the C ABI, the autograd
function end to end and one use_device_batchnorm(fuse=True) pass, against tests/batchnorm_ref.py.

Accuracy criterion (every output, every case, every variant): with err(v) = max |v - ref64| / max |ref64| and ref64 = the yardstick in
float64,

    err(device) <= F * err(yardstick in float32 on the CPU) + 2^-24

-- the float32 run is the torch arithmetic a user gets without the kernels, not the code under test; 2^-24 is the rounding of the
float32 output itself.  F = 1 (by the issue F may not exceed 4): the kernels work in float64 and round once, so every output measured
on the MI355X stays within 2^-24 of the reference by itself (no ratio counts), and the worst ratio err_dev / err_f32 among all outputs
whose float32 error is not 0 is 1.0, reached where both runs give the same bits (profiles/batchnorm_errors.txt, written by
tools/batchnorm_errors.py from `measure()` below).

The test data keep every pre-activation at least 2^-8 away from 0 in float64 (batchnorm_ref.nudge; asserted before anything touches
the device), so the ReLU mask does not depend on the precision."""
import copy
import os
import sys
from functools import lru_cache

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batchnorm_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F = 1.0
FLOOR = 2.0 ** -24
MOMENTUM = 0.1

# name -> (shape, channels_last, kind, seed)
CASES = {
    "tiny": ((2, 3, 1, 1), False, None, 102),                # two values per channel
    "odd": ((3, 5, 7, 5), False, None, 103),                 # HW = 35: unaligned planes, the scalar path
    "odd_cl": ((3, 5, 7, 5), True, None, 103),
    "aligned": ((4, 64, 8, 4), False, None, 104),            # the float4 path
    "aligned_cl": ((4, 64, 8, 4), True, None, 104),
    "wide_c": ((5, 70, 3, 3), False, None, 105),             # C > 64 and no multiple of 64
    "wide_c_cl": ((2, 260, 3, 2), True, None, 109),          # channel contiguous, four channels per lane, two column tiles
    "real_c1024_cl": ((3, 1024, 4, 8), True, None, 111),     # layer3's width: four column tiles of 256 channels
    "real_c2048_cl": ((5, 2048, 2, 4), True, None, 112),     # layer4's width: eight column tiles
    "multi_partial": ((33, 8, 16, 8), False, None, 106),     # the smallest N at which a channel is split over two workgroups
    "large_mean": ((4, 6, 8, 4), False, "large_mean", 107),  # x = 1000 + N(0, 1): cancellation in the variance
    "const_channel": ((3, 5, 7, 5), False, "const", 108),    # var = 0, invstd = eps^-1/2
    "bn1d": ((7, 130), False, None, 110),                    # the [B, C] layout
}
VARIANTS = ("plain", "relu", "relu_res")


def _geom(name):
    shape, cl = CASES[name][:2]
    N, C = shape[:2]
    HW = 1
    for s in shape[2:]:
        HW *= s
    return N, C, HW, int(cl)


@lru_cache(maxsize=None)
def _data(name):
    shape, _, kind, seed = CASES[name]
    d = ref.make_case(shape, seed, kind)
    # the margin, in float64, before anything touches the device
    assert ref.min_margin(d["x"], d["weight"], d["bias"], d["eps"]) >= ref.MARGIN
    assert ref.min_margin(d["x"], d["weight"], d["bias"], d["eps"], d["residual"]) >= ref.MARGIN
    return d


@lru_cache(maxsize=None)
def _refs(name, variant):
    """{output: (ref64, ref32)} of one case and variant, computed once"""
    d = _data(name)
    relu, res = variant != "plain", (d["residual"] if variant == "relu_res" else None)
    out = {}
    per = []
    for dt in (torch.float64, torch.float32):
        f = ref.forward(d["x"], d["weight"], d["bias"], d["eps"], relu, res, dt)
        b = ref.backward(d["x"], d["weight"], f, d["gy"], relu, dt)
        rm, rv = ref.running_update(d["running_mean"], d["running_var"], f["mean"], f["var"], ref.count(d["x"]), MOMENTUM, dt)
        per.append(dict(mean=f["mean"], var=f["var"], invstd=f["invstd"], y=f["y"], running_mean=rm, running_var=rv, dx=b["dx"],
                        dweight=b["dweight"], dbias=b["dbias"], dresidual=b["dresidual"]))
    for k in per[0]:
        out[k] = (per[0][k], per[1][k])
    return out


def _dev(t, cl):
    t = t.cuda()
    return t.contiguous(memory_format=torch.channels_last) if cl else t


def _abi(name, variant):
    """every entry point once through the C ABI -> {output: device value on the CPU}"""
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    d = _data(name)
    N, C, HW, cl = _geom(name)
    relu, with_res = variant != "plain", variant == "relu_res"
    x, gy = _dev(d["x"], cl), _dev(d["gy"], cl)
    r = _dev(d["residual"], cl) if with_res else None
    w, b = d["weight"].cuda(), d["bias"].cuda()
    rm, rv = d["running_mean"].cuda(), d["running_var"].cuda()
    P = L.ssg_bn_num_partials(N, C, HW, cl)
    nws = L.ssg_bn_workspace_bytes(N, C, HW, cl)
    assert P >= 1 and nws == 16 * C * P

    def nan(*shape, dtype=torch.float32):
        return torch.full(shape, float("nan"), dtype=dtype, device="cuda")
    ws, stat, coef = nan(nws // 8, dtype=torch.float64), nan(3, C, dtype=torch.float64), nan(2, C, dtype=torch.float64)
    y, dx, dres = torch.full_like(x, float("nan")), torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    dw, db = nan(C), nan(C)
    check(L.ssg_bn_stats_f32(ptr(x), N, C, HW, cl, d["eps"], MOMENTUM, None, ptr(rm), ptr(rv), ptr(stat), ptr(ws), nws, stream()), "ssg_bn_stats_f32")
    check(L.ssg_bn_apply_f32(ptr(x), ptr(stat), ptr(w), ptr(b), ptr(r), int(relu), N, C, HW, cl, ptr(y), stream()), "ssg_bn_apply_f32")
    ws.fill_(float("nan"))
    check(L.ssg_bn_backward_reduce_f32(ptr(gy), ptr(x), ptr(y) if relu else None, ptr(stat), N, C, HW, cl, ptr(coef), ptr(dw), ptr(db), ptr(ws), nws,
                                       stream()), "ssg_bn_backward_reduce_f32")
    check(L.ssg_bn_backward_apply_f32(ptr(gy), ptr(x), ptr(y) if relu else None, ptr(stat), ptr(w), ptr(coef), N, C, HW, cl, ptr(dx),
                                      ptr(dres) if with_res else None, stream()), "ssg_bn_backward_apply_f32")
    torch.cuda.synchronize()
    assert y.stride() == x.stride() and dx.stride() == x.stride()
    out = dict(mean=stat[0], var=stat[1], invstd=stat[2], y=y, running_mean=rm, running_var=rv, dx=dx, dweight=dw, dbias=db)
    if with_res:
        out["dresidual"] = dres
    return {k: v.cpu() for k, v in out.items()}


def _function(name, variant):
    """batch_norm_train end to end: forward, backward of sum(y * gy), the running statistics -> {output: value on the CPU}"""
    from ssg_amd import batchnorm as bn
    d = _data(name)
    cl = CASES[name][1]
    relu, with_res = variant != "plain", variant == "relu_res"
    x = _dev(d["x"], cl).requires_grad_(True)
    r = _dev(d["residual"], cl).requires_grad_(True) if with_res else None
    w, b = d["weight"].cuda().requires_grad_(True), d["bias"].cuda().requires_grad_(True)
    rm, rv = d["running_mean"].cuda(), d["running_var"].cuda()
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    y = bn.batch_norm_train(x, w, b, rm, rv, nbt, MOMENTUM, d["eps"], relu, r)
    assert y.is_cuda and y.dtype == torch.float32 and y.shape == x.shape and y.stride() == x.stride()
    (y * _dev(d["gy"], cl)).sum().backward()
    torch.cuda.synchronize()
    assert int(nbt) == 1
    out = dict(y=y.detach(), running_mean=rm, running_var=rv, dx=x.grad, dweight=w.grad, dbias=b.grad)
    if with_res:
        out["dresidual"] = r.grad
    return {k: v.cpu() for k, v in out.items()}


def measure(name, variant, run=None):
    """[(output, err_dev, err_f32)] of one case and variant through the C ABI (or through `run`)"""
    refs = _refs(name, variant)
    rows = []
    for k, v in (run or _abi)(name, variant).items():
        r64, r32 = refs[k]
        assert bool(torch.isfinite(v).all()), (name, variant, k)
        rows.append((k, ref.rel_err(v, r64), ref.rel_err(r32, r64)))
    return rows


def _within(err_dev, err_f32):
    return err_dev <= F * err_f32 + FLOOR


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_points_vs_float64_reference(name, variant):
    for k, err_dev, err_f32 in measure(name, variant):
        print("%-14s %-9s %-13s err_dev %.3e err_f32 %.3e" % (name, variant, k, err_dev, err_f32))
        assert _within(err_dev, err_f32), (name, variant, k, err_dev, err_f32)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_autograd_function_vs_float64_reference(name, variant):
    for k, err_dev, err_f32 in measure(name, variant, _function):
        print("%-14s %-9s %-13s err_dev %.3e err_f32 %.3e" % (name, variant, k, err_dev, err_f32))
        assert _within(err_dev, err_f32), (name, variant, k, err_dev, err_f32)


def test_constant_channel_has_zero_variance():
    out = _abi("const_channel", "plain")
    assert float(out["var"][1]) == 0.0 and abs(float(out["invstd"][1]) * 1e-5 ** 0.5 - 1.0) < 1e-15
    d = _data("const_channel")
    assert torch.equal(out["y"][:, 1], torch.full_like(out["y"][:, 1], float(d["bias"][1])))


def test_multi_partial_case_crosses_the_split():
    from ssg_amd import _lib
    L = _lib.lib()
    N, C, HW, cl = _geom("multi_partial")
    assert L.ssg_bn_num_partials(N, C, HW, cl) > 1
    assert L.ssg_bn_num_partials(N - 1, C, HW, cl) == 1            # the smallest: one image fewer is a single workgroup per channel
    N, C, HW, cl = _geom("odd_cl")
    assert L.ssg_bn_num_partials(N, C, HW, cl) > 1                 # the channel-contiguous kernels are split as well


@pytest.mark.parametrize("name", ["multi_partial", "aligned_cl", "odd", "bn1d", "wide_c_cl"])
def test_two_runs_give_the_same_bits(name):
    for run in (_abi, _function):
        a, b = run(name, "relu_res"), run(name, "relu_res")
        for k in a:
            assert torch.equal(a[k].view(torch.int32 if a[k].dtype == torch.float32 else torch.int64),
                               b[k].view(torch.int32 if b[k].dtype == torch.float32 else torch.int64)), (name, k)


def test_cumulative_average_over_two_batches():
    """momentum=None: f = 1 / num_batches_tracked, read on the device; two consecutive calls of the module"""
    from ssg_amd import batchnorm as bn
    d1, d2 = _data("large_mean"), _data("aligned")
    x1, x2 = d1["x"], d2["x"][:, :6].contiguous()
    m = bn.BatchNorm2d(6, momentum=None).cuda().train()
    m.running_mean.copy_(d1["running_mean"]); m.running_var.copy_(d1["running_var"])
    yard = {}
    for dt in (torch.float64, torch.float32):
        rm, rv = d1["running_mean"], d1["running_var"]
        for k, x in enumerate((x1, x2)):
            f = ref.forward(x, m.weight.detach().cpu(), m.bias.detach().cpu(), m.eps, dtype=dt)
            rm, rv = ref.running_update(rm, rv, f["mean"], f["var"], ref.count(x), 1.0 / (k + 1), dt)
        yard[dt] = (rm, rv)
    m(x1.cuda()); m(x2.cuda())
    assert int(m.num_batches_tracked) == 2
    for k, got in enumerate((m.running_mean, m.running_var)):
        e_dev, e_f32 = ref.rel_err(got, yard[torch.float64][k]), ref.rel_err(yard[torch.float32][k], yard[torch.float64][k])
        print("cumulative %s err_dev %.3e err_f32 %.3e" % (("running_mean", "running_var")[k], e_dev, e_f32))
        assert _within(e_dev, e_f32)


def test_one_value_per_channel_raises_before_any_launch():
    from ssg_amd import batchnorm as bn
    from ssg_amd import _lib
    x = torch.zeros(1, 3, 1, 1, device="cuda")
    rm, rv = torch.zeros(3, device="cuda"), torch.ones(3, device="cuda")
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        bn.batch_norm_train(x, torch.ones(3, device="cuda"), torch.zeros(3, device="cuda"), rm, rv)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        bn.BatchNorm1d(3).cuda().train()(x.view(1, 3))
    assert float(rm.abs().sum()) == 0.0 and float(rv.sum()) == 3.0                                 # nothing ran
    assert _lib.lib().ssg_bn_stats_f32(_lib.ptr(x), 1, 3, 1, 0, 1e-5, 0.1, None, None, None, _lib.ptr(rm), _lib.ptr(rv), 1 << 20, None) == -1


def test_inputs_the_kernels_do_not_take_and_double_backward():
    """a float64 CPU input is computed on the GPU in float32 and gets its gradient back as float64 on the CPU (as
    ssg_amd.dce.ClusterAssignment does it); a non-contiguous input is made contiguous; a double backward raises"""
    from ssg_amd import batchnorm as bn
    d = _data("odd")
    refs = _refs("odd", "relu")
    x = d["x"].double().requires_grad_(True)
    w, b = d["weight"].clone().requires_grad_(True), d["bias"].cuda().requires_grad_(True)
    rm, rv = d["running_mean"].clone(), d["running_var"].clone()                                  # CPU buffers: updated in place too
    y = bn.batch_norm_train(x, w, b, rm, rv, None, MOMENTUM, d["eps"], relu=True)
    (y * d["gy"].cuda()).sum().backward()
    assert y.is_cuda and y.dtype == torch.float32
    assert x.grad.dtype == torch.float64 and x.grad.device.type == "cpu" and w.grad.device.type == "cpu" and b.grad.is_cuda
    for k, v in (("y", y.detach()), ("dx", x.grad), ("dweight", w.grad), ("running_mean", rm), ("running_var", rv)):
        assert _within(ref.rel_err(v, refs[k][0]), ref.rel_err(refs[k][1], refs[k][0])), k
    xt = d["x"].cuda().permute(0, 1, 3, 2)                                                        # [3, 5, 5, 7], neither layout
    assert not xt.is_contiguous()
    yt = bn.batch_norm_train(xt, d["weight"].cuda(), d["bias"].cuda(), None, None, relu=True)
    assert _within(ref.rel_err(yt.permute(0, 1, 3, 2), refs["y"][0]), ref.rel_err(refs["y"][1], refs["y"][0]))
    x2 = d["x"].cuda().requires_grad_(True)
    y2 = bn.batch_norm_train(x2, d["weight"].cuda(), d["bias"].cuda(), None, None)
    g, = torch.autograd.grad((y2 * y2).sum(), x2, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_use_device_batchnorm_fused_pass_over_the_test_local_blocks():
    """train-mode forward and backward of the look-alike network of tests/test_batchnorm_host.py after use_device_batchnorm(fuse=True)
    (fused Bottleneck with a downsample branch, fused BasicBlock, fused stem, a block of another shape, BatchNorm1d) against the
    untouched network in float64 on the CPU: the output, the gradients of the input and of every parameter, every running statistic.
    The bound here is structural: the network chains 10 normalisations and the float32 element-wise layers between them (torch's, not
    under test); a float32 forward + backward of that depth stays within 2^-24 * (a few hundred operations per value) < 2^-14 of the
    largest magnitude, a wrong wiring (a missing ReLU, residual or gradient path) is off by O(1).  Seeded inputs."""
    import test_batchnorm_host as host
    from ssg_amd import batchnorm as bn
    tol = 2.0 ** -14
    net64 = host.randomise(host.Net()).double().train()
    net = copy.deepcopy(net64).float()
    bn.use_device_batchnorm(net, fuse=True)
    net = net.cuda().train()
    x = torch.randn(6, 6, 5, 4, generator=torch.Generator().manual_seed(21))
    gy = torch.randn(6, 6, generator=torch.Generator().manual_seed(22))
    x64 = x.double().requires_grad_(True)
    out64 = net64(x64)
    (out64 * gy.double()).sum().backward()
    xd = x.cuda().requires_grad_(True)
    out = net(xd)
    (out * gy.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert out.shape == out64.shape and ref.rel_err(out.detach(), out64.detach()) <= tol, ref.rel_err(out.detach(), out64.detach())
    p64 = dict(net64.named_parameters())
    assert ref.rel_err(xd.grad, x64.grad) <= tol, ref.rel_err(xd.grad, x64.grad)
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        assert ref.rel_err(p.grad, p64[k].grad) <= tol, (k, ref.rel_err(p.grad, p64[k].grad))
    b64 = dict(net64.named_buffers())
    for k, v in net.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(b64[k]) == 1, k
        else:
            assert ref.rel_err(v, b64[k]) <= tol, (k, ref.rel_err(v, b64[k]))
