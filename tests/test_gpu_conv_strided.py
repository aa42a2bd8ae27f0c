"""GPU suite of the strided train-mode Conv2d and the 7x7 stem (csrc/conv_strided.hip, ssg_amd/conv_strided.py): every case once
through `conv2d_train_strided` and once through the raw entry points, against torch's `F.conv2d` and its autograd in float64 on the
CPU (tests/conv_strided_ref.py).

Accuracy criterion, derived and not measured (the one of test_gpu_conv_train.py): every element of every output satisfies

    |dev - ref64| <= (L + 2) * 2^-24 * A

with L the length of that output's reduction (KH KW Cin for y, KH KW Cout for dX -- an upper bound for every parity class -- and
B OH OW for dW) and A the same operator applied to |x|, |w|, |dY| in float64.

The cases: the smallest shapes at which each thing can go wrong (CASES, MULTI) and the six stride-2 convolutions of ResNet-50 at their
real channel pairs and input row widths, with just enough pixels for three weight-gradient slices and two 64-pixel tiles per parity
class of dX (REAL: up to 1024 -> 2048, K up to 4608; tests/test_conv_strided_host.py shows what the bound sees there).

Composition (use_device_conv(strided=True) + use_device_batchnorm on a stride-2 bottleneck): test_gpu_conv_train.py's criterion on the
parameter gradients,

    err(device) <= F_COMP * err(float32 CPU run of the same block) + 2^-24,   err(v) = max |v - ref64| / max |ref64|

with F_COMP the next power of two above the largest ratio measured on the MI355X (profiles/conv_strided_errors.txt, written by
tools/conv_strided_errors.py from `measure()` / `measure_composition()` below) and never more than 4: measured 1.67 (bn2.weight),
so F_COMP = 2.  The block's data keep every ReLU input at least 2^-15 away from 0 in float64 (asserted before anything touches the
device)."""
import copy
import os
import sys
from functools import lru_cache

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_strided_ref as ref  # noqa: E402
import train_common as tc  # noqa: E402
from train_common import FLOOR, _lib, _nan  # noqa: E402,F401

pytestmark = pytest.mark.gpu

F_COMP = 2.0
CL = torch.channels_last
OUTS = ("y", "dx", "dw")


def _case(name):
    """the (B, H, W, Cin, Cout, k, seed) of a named case; the multi-slice ones take the smallest B that gives three ragged slices"""
    if name in ref.CASES:
        return ref.CASES[name]
    if name in ref.REAL:
        return ref.REAL[name]
    H, W, cin, cout, k, seed = ref.MULTI[name]
    B = ref.multi_slice_batch(_lib(), H, W, cin, cout, k)
    # a slice rule with a floor that hides stage 2 from this suite must be changed, not tested around
    assert B is not None, "no B <= 64 gives ssg_conv_wgrad_strided_num_slices >= 3 with a ragged slice at %r" % (ref.MULTI[name],)
    return (B, H, W, cin, cout, k, seed)


ALL = tuple(ref.CASES) + tuple(ref.MULTI) + tuple(ref.REAL)


def _outs(case):
    return ("y", "dw") if case[5] == 7 else OUTS            # the stem has no data gradient


def _api(case, x_cl=True, w_cl=False, x_grad=True, w_grad=True):
    """one forward + backward through ssg_amd.conv2d_train_strided -> {y, dx, dw} as the device returned them"""
    import ssg_amd
    d = ref.reference(*case)[0]
    x_grad = x_grad and d["k"] != 7
    x = d["x"].cuda()
    x = (x.contiguous(memory_format=CL) if x_cl else x).requires_grad_(x_grad)
    w = d["w"].cuda()
    w = (w.contiguous(memory_format=CL) if w_cl else w).requires_grad_(w_grad)
    y = ssg_amd.conv2d_train_strided(x, w, 2, d["pad"])
    # autograd.grad, not .backward(): AccumulateGrad re-lays a gradient out in its leaf's strides, which would hide what the function returns
    wrt = [t for t, need in ((x, x_grad), (w, w_grad)) if need]
    grads = dict(zip([n for n, need in (("dx", x_grad), ("dw", w_grad)) if need], torch.autograd.grad(y, wrt, d["gy"].cuda())))
    return dict(y=y.detach(), dx=grads.get("dx"), dw=grads.get("dw"))


def _abi(case):
    """the raw entry points -> {y, dx, dw} as NCHW-shaped CPU tensors; every output and the workspace start as NaN"""
    from ssg_amd._lib import check, ptr, stream
    L = _lib()
    B, H, W, cin, cout, k, _ = case
    stem = k == 7
    OH, OW = ref.out_hw(H, W, k)
    d = ref.reference(*case)[0]
    gy = d["gy"].cuda().permute(0, 2, 3, 1).contiguous()
    w = d["w"].cuda()
    s = w.stride()
    zeros = torch.zeros(max(cin, cout), dtype=torch.float32, device="cuda")
    if stem:
        x = _nan(B, H, W, 4)
        check(L.ssg_nchw_to_nhwc4(ptr(d["x"].cuda().contiguous()), ptr(x), B, H, W, 0, stream()), "nhwc4")
        wf, wd = _nan(cout, 224), None
        # the stem has no data-gradient packing and no data gradient
        assert L.ssg_conv_pack_strided_f32(ptr(w), s[0], s[1], s[2], s[3], cout, cin, k, k, ptr(wf), ptr(wf), stream()) == -1
        assert L.ssg_conv_dgrad_strided_f32(ptr(gy), ptr(wf), ptr(x), B, H, W, cin, cout, k, k, 2, stream()) == -1
    else:
        x = d["x"].cuda().permute(0, 2, 3, 1).contiguous()
        wf, wd = _nan(cout, k * k * cin), _nan(k * k, cout, cin)
    check(L.ssg_conv_pack_strided_f32(ptr(w), s[0], s[1], s[2], s[3], cout, cin, k, k, ptr(wf), ptr(wd), stream()), "pack")
    y, dw = _nan(B, OH, OW, cout), _nan(cout, cin, k, k)
    check(L.ssg_conv2d_nhwc_f32(ptr(x), ptr(wf), ptr(zeros), None, ptr(y), B, H, W, 4 if stem else cin, cout, k, k, 2, k // 2, 0, stream()), "forward")
    out = {}
    if not stem:
        dx = _nan(B, H, W, cin)
        check(L.ssg_conv_dgrad_strided_f32(ptr(gy), ptr(wd), ptr(dx), B, H, W, cin, cout, k, k, 2, stream()), "dgrad")
        out["dx"] = dx.permute(0, 3, 1, 2).cpu()
    M = B * OH * OW
    n = L.ssg_conv_wgrad_strided_num_slices(M, cout, k, k, cin, 2)
    nws = L.ssg_conv_wgrad_strided_workspace_bytes(M, cout, k, k, cin, 2)
    assert n >= 1 and nws == 4 * n * cout * (13 * 64 if stem else k * k * cin)
    ws = _nan(nws // 4 + 64)                               # 64 floats of guard behind the workspace
    s = dw.stride()
    check(L.ssg_conv_wgrad_strided_f32(ptr(gy), ptr(x), B, H, W, cin, cout, k, k, 2, ptr(dw), s[0], s[1], s[2], s[3], ptr(ws), nws, 3, stream()), "wgrad")
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[nws // 4:]).all()) and not bool(torch.isnan(ws[:nws // 4]).any())     # all of the workspace, nothing past it
    out.update(y=y.permute(0, 3, 1, 2).cpu(), dw=dw.cpu(), w_fwd=wf.cpu(), w_dgrad=None if stem else wd.cpu())
    return out


def _check(case, got, which=None):
    tc.check_bound(ref.reference, case, got, which or _outs(case))


@pytest.mark.parametrize("name", ALL)
def test_conv2d_train_strided_against_float64(name):
    case = _case(name)
    got = _api(case)
    _check(case, got)
    assert got["y"].is_contiguous(memory_format=CL) and (case[5] == 7 or got["dx"].is_contiguous(memory_format=CL))


@pytest.mark.parametrize("name", ALL)
def test_entry_points_against_float64(name):
    case = _case(name)
    got = _abi(case)
    _check(case, got)
    B, H, W, cin, cout, k, _ = case
    w = ref.reference(*case)[0]["w"]
    if k == 7:                                              # the packings move bits: k = (r*7 + s)*4 + c, zero padding
        want = torch.zeros(cout, 56, 4)
        want[:, :49, :3] = w.permute(0, 2, 3, 1).reshape(cout, 49, 3)
        assert torch.equal(got["w_fwd"], want.reshape(cout, 224))
    else:
        from conv_train_ref import pack_fwd
        assert torch.equal(got["w_fwd"], pack_fwd(w))
        assert torch.equal(got["w_dgrad"], ref.pack_dgrad_s2(w))
    api = _api(case)
    for o in _outs(case):                                   # the autograd function adds nothing of its own
        assert torch.equal(api[o].cpu(), got[o]), o


def test_1x1_even_sides_are_exact_zeros():
    """what no tap of a stride-2 1x1 reaches -- the three empty parity classes, the last row and column of an even-sized input -- is
    written, and as exactly 0.0, by both routes"""
    _exact_zeros(ref.CASES["1x1_even"])


def _exact_zeros(case):
    for dx in (_api(case)["dx"].cpu(), _abi(case)["dx"]):
        live = torch.zeros(dx.shape[2:], dtype=torch.bool)
        live[0::2, 0::2] = True
        assert not bool(live[-1].any()) and not bool(live[:, -1].any())            # even sides: the last row and column are unreached
        dead = dx[:, :, ~live]
        assert bool((dead == 0).all()) and not bool(torch.signbit(dead).any())
        assert bool((dx[:, :, live] != 0).any())


@pytest.mark.parametrize("name", ref.DOWNSAMPLE)
def test_downsample_empty_classes_are_exact_zeros(name):
    """the same property on ResNet-50's three downsample shapes: 4 to 16 column tiles of dX, three of four classes without a tap"""
    _exact_zeros(ref.REAL[name])


def test_real_cases_have_three_slices_and_ragged_tiles():
    """every real-width case: exactly three weight-gradient slices of which the last is shorter (from the library's own count, so a
    later change of the plan cannot quietly turn these into one-slice cases), a ragged last 128-row tile in the forward, and, the
    sides being even, four parity classes of M pixels each: at least two 64-pixel tiles, the last one ragged"""
    L = _lib()
    for name, (B, H, W, cin, cout, k, _) in ref.REAL.items():
        assert H % 2 == 0 and W % 2 == 0, name
        OH, OW = ref.out_hw(H, W, k)
        M = B * OH * OW
        assert (OH, OW) == (H // 2, W // 2) and 512 < M < 768 and M % 256 != 0 and M % 128 != 0, name
        assert M == B * ((H + 1) // 2) * ((W + 1) // 2) and M > 64 and M % 64 != 0, name       # the largest class of dX
        n = L.ssg_conv_wgrad_strided_num_slices(M, cout, k, k, cin, 2)
        assert n == 3 and M % n != 0, (name, n)             # equal slices cannot cover M: the last one is shorter
        assert L.ssg_conv_wgrad_strided_workspace_bytes(M, cout, k, k, cin, 2) == 4 * 3 * cout * k * k * cin
    assert sorted(c[3:6] for c in ref.REAL.values()) == [(128, 128, 3), (256, 256, 3), (256, 512, 1), (512, 512, 3), (512, 1024, 1), (1024, 2048, 1)]


def test_multi_slice_cases_have_a_real_slice_sum():
    L = _lib()
    for name in ref.MULTI:
        B, H, W, cin, cout, k, _ = _case(name)
        OH, OW = ref.out_hw(H, W, k)
        assert B <= 64
        n = L.ssg_conv_wgrad_strided_num_slices(B * OH * OW, cout, k, k, cin, 2)
        assert n >= 3 and (B * OH * OW) % n != 0           # equal slices cannot cover M: the last one is shorter


def test_layouts_give_the_same_bits():
    for name, cl_stride, std_stride in (("3x3_cout192", (64 * 9, 1, 3 * 64, 64), (64 * 9, 9, 3, 1)), ("stem_odd", (147, 1, 21, 3), (147, 49, 7, 1))):
        case = ref.CASES[name]
        base = _api(case, x_cl=True, w_cl=False)
        assert base["dw"].is_contiguous()
        _check(case, base)
        for x_cl, w_cl in [(False, False), (True, True), (False, True)]:
            got = _api(case, x_cl=x_cl, w_cl=w_cl)
            for o in _outs(case):
                assert torch.equal(got[o], base[o]), (name, o, x_cl, w_cl)
            assert got["dw"].stride() == (cl_stride if w_cl else std_stride)     # the stem's dW also with a channels_last weight


def test_frozen_input_and_frozen_weight():
    case = ref.CASES["3x3_odd"]
    base = _api(case)
    got = _api(case, x_grad=False)
    assert got["dx"] is None and torch.equal(got["dw"], base["dw"]) and torch.equal(got["y"], base["y"])
    got = _api(case, w_grad=False)
    assert got["dw"] is None and torch.equal(got["dx"], base["dx"])


def test_two_passes_are_bit_identical():
    for name in tuple(ref.MULTI) + ("3x3_even", "1x1_odd"):
        case = _case(name)
        a, b = _api(case), _api(case)
        for o in _outs(case):
            assert torch.equal(a[o], b[o]), (name, o)
    case = _case("multi_3x3")
    a, b = _abi(case), _abi(case)
    for o in OUTS:
        assert torch.equal(a[o], b[o]), o


def test_stem_refuses_a_data_gradient_and_modules_run():
    import ssg_amd
    d = ref.reference(*ref.CASES["stem_even"])[0]
    with pytest.raises(ValueError, match="data gradient"):
        ssg_amd.conv2d_train_strided(d["x"].cuda().requires_grad_(True), d["w"].cuda(), 2, 3)
    m = ssg_amd.StridedConv2d(3, 64, 7, 2, 3).cuda()
    with torch.no_grad():
        m.weight.copy_(d["w"])
    y = m(d["x"].cuda())
    assert torch.equal(y, _api(ref.CASES["stem_even"])["y"])
    with torch.no_grad():
        assert torch.equal(m.eval()(d["x"].cuda()), y)
    with pytest.raises(RuntimeError):                       # a double backward raises
        d3 = ref.reference(*ref.CASES["3x3_odd"])[0]
        x, w = d3["x"].cuda().requires_grad_(True), d3["w"].cuda().requires_grad_(True)
        (gx,) = torch.autograd.grad(ssg_amd.conv2d_train_strided(x, w, 2, 1), x, d3["gy"].cuda(), create_graph=True)
        gx.sum().backward()


# ---- composition -----------------------------------------------------------------------------------------------------------------------

COMP_SHAPE = (4, 256, 8, 4)
COMP_MARGIN = 2.0 ** -15


def _comp_inputs(g):
    return torch.randn(*COMP_SHAPE, generator=g), torch.randn(COMP_SHAPE[0], 512, COMP_SHAPE[2] // 2, COMP_SHAPE[3] // 2, generator=g)


@lru_cache(maxsize=None)
def _comp_data():
    """(block in float32 on the CPU, x, gy): the first seed whose ReLU inputs all stay COMP_MARGIN away from 0 in float64"""
    return tc.quiet_data(range(500, 600), lambda: ref.Bottleneck(256, 128, 2, ref.downsample(256, 512, 2)), _comp_inputs, 3, COMP_MARGIN)


def _comp_backward(b, x, gy):
    b(x).backward(gy)


@lru_cache(maxsize=None)
def _comp_refs():
    return tc.reference_grads(_comp_data(), 3, COMP_MARGIN, _comp_backward)


def _comp_device():
    import ssg_amd
    block, x, gy = _comp_data()
    b = copy.deepcopy(block).cuda()
    ssg_amd.use_device_conv(b, strided=True)
    ssg_amd.use_device_batchnorm(b)
    assert b._ssg_conv_skipped == [] and b._ssg_bn_skipped == []
    assert isinstance(b.conv1, ssg_amd.Conv2d) and isinstance(b.conv3, ssg_amd.Conv2d)
    assert isinstance(b.conv2, ssg_amd.StridedConv2d) and isinstance(b.downsample[0], ssg_amd.StridedConv2d)
    b = b.to(memory_format=CL)
    return tc.grads(b, lambda m: _comp_backward(m, x.cuda().contiguous(memory_format=CL), gy.cuda().contiguous(memory_format=CL)))


def measure_composition():
    """[(parameter, err_dev, err_f32)] of the composed block's parameter gradients"""
    g64, g32 = _comp_refs()
    return tc.composition_rows(g64, g32, _comp_device())


def test_composition_with_device_batchnorm():
    tc.check_composition(measure_composition(), F_COMP)


def measure():
    """[(case, path, output, max |dev - ref64|, max |f32 CPU - ref64|, worst err_dev / bound)] for tools/conv_strided_errors.py"""
    rows = []
    for name in ALL:
        case = _case(name)
        rows += tc.bound_rows(ref.reference, ref.outputs, name, case, (("conv2d_train_strided", _api(case)), ("entry points", _abi(case))), _outs(case))
    return rows
