"""GPU suite of the train-mode Conv2d (csrc/conv_train.hip, ssg_amd/conv.py): every case once through `conv2d_train` and once through
the raw entry points, against torch's `F.conv2d` and its autograd in float64 on the CPU (tests/conv_train_ref.py).

Accuracy criterion, derived and not measured: every element of every output satisfies

    |dev - ref64| <= (L + 2) * 2^-24 * A

with L the length of that output's reduction (KH KW Cin for y, KH KW Cout for dX, B OH OW for dW) and A the same convolution or gradient
applied to |x|, |w|, |dY| in float64: the standard bound of a length-L float32 sum in any order, plus one rounding.

The cases: the smallest shapes at which each thing can go wrong (CASES, MULTI: 64 ... 192 channels, sides up to 8), every distinct
(Cin, Cout, k) of ResNet-50 on its real row width with just enough pixels for three weight-gradient slices (REAL: up to 2048 channels,
K up to 4608), and layer1's two 1x1 shapes at the trainer's own M = 131072 against float64 matmuls, dW under the tighter slice-aware
bound derived in test_trainer_batch_1x1_against_float64_matmul (TRAINER).  tests/test_conv_train_host.py shows that both bounds see
a missing 32-wide chunk, stage or pixel group at these shapes.

Composition (use_device_conv + use_device_batchnorm on a bottleneck block): each BatchNorm divides by a batch standard deviation, so
the per-element bound does not carry through; the criterion is test_gpu_batchnorm.py's form, on the parameter gradients,

    err(device) <= F_COMP * err(float32 CPU run of the same block) + 2^-24,   err(v) = max |v - ref64| / max |ref64|

with F_COMP the next power of two above the largest ratio measured on the MI355X (profiles/conv_train_errors.txt, written by
tools/conv_train_errors.py from `measure()` / `measure_composition()` below) and never more than 4: measured 3.28 (downsample.0.weight,
where the float32 CPU run happens to err by only 1.7e-7; the device's 5.4e-7 is that of the other convolutions), so F_COMP = 4.  The block's data keep every ReLU
input at least 2^-15 away from 0 in float64 (asserted before anything touches the device), so no mask depends on the precision."""
import copy
import os
import sys
from functools import lru_cache

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_train_ref as ref  # noqa: E402
import train_common as tc  # noqa: E402
from train_common import FLOOR, _lib, _nan  # noqa: E402,F401

pytestmark = pytest.mark.gpu

F_COMP = 4.0
CL = torch.channels_last
OUTS = ("y", "dx", "dw")


def _case(name):
    """the (B, H, W, Cin, Cout, k, seed) of a named case; the multi-slice ones take the smallest B that gives three slices"""
    if name in ref.CASES:
        return ref.CASES[name]
    if name in ref.REAL:
        return ref.REAL[name]
    H, W, cin, cout, k, seed = ref.MULTI[name]
    B = ref.multi_slice_batch(_lib(), H, W, cin, cout, k)
    # a slice rule with a floor that hides stage 2 from this suite must be changed, not tested around
    assert B is not None, "no B <= 64 gives ssg_conv_wgrad_num_slices >= 3 at %r" % (ref.MULTI[name],)
    return (B, H, W, cin, cout, k, seed)


ALL = tuple(ref.CASES) + tuple(ref.MULTI) + tuple(ref.REAL)


def _api(case, x_cl=True, w_cl=False, x_grad=True, w_grad=True):
    """one forward + backward through ssg_amd.conv2d_train -> {y, dx, dw} as the device returned them"""
    import ssg_amd
    d = ref.reference(*case)[0]
    x = d["x"].cuda()
    x = (x.contiguous(memory_format=CL) if x_cl else x).requires_grad_(x_grad)
    w = d["w"].cuda()
    w = (w.contiguous(memory_format=CL) if w_cl else w).requires_grad_(w_grad)
    y = ssg_amd.conv2d_train(x, w, 1, d["pad"])
    # autograd.grad, not .backward(): AccumulateGrad re-lays a gradient out in its leaf's strides, which would hide what the function returns
    wrt = [t for t, need in ((x, x_grad), (w, w_grad)) if need]
    grads = dict(zip([n for n, need in (("dx", x_grad), ("dw", w_grad)) if need], torch.autograd.grad(y, wrt, d["gy"].cuda())))
    return dict(y=y.detach(), dx=grads.get("dx"), dw=grads.get("dw"))


def _abi(case):
    """the raw entry points -> {y, dx, dw} as NCHW-shaped CPU tensors, plus the two packings"""
    from ssg_amd._lib import check, ptr, stream
    L = _lib()
    B, H, W, cin, cout, k, _ = case
    d = ref.reference(*case)[0]
    x = d["x"].cuda().permute(0, 2, 3, 1).contiguous()
    gy = d["gy"].cuda().permute(0, 2, 3, 1).contiguous()
    w = d["w"].cuda()
    wf, wd = _nan(cout, k * k * cin), _nan(cin, k * k * cout)
    s = w.stride()
    check(L.ssg_conv_pack_train_f32(ptr(w), s[0], s[1], s[2], s[3], cout, cin, k, k, ptr(wf), ptr(wd), stream()), "pack")
    zeros = torch.zeros(max(cin, cout), dtype=torch.float32, device="cuda")
    y, dx, dw = _nan(B, H, W, cout), _nan(B, H, W, cin), _nan(cout, cin, k, k)
    check(L.ssg_conv2d_nhwc_f32(ptr(x), ptr(wf), ptr(zeros), None, ptr(y), B, H, W, cin, cout, k, k, 1, k // 2, 0, stream()), "forward")
    check(L.ssg_conv2d_nhwc_f32(ptr(gy), ptr(wd), ptr(zeros), None, ptr(dx), B, H, W, cout, cin, k, k, 1, k // 2, 0, stream()), "dgrad")
    n = L.ssg_conv_wgrad_num_slices(B * H * W, cout, k, k, cin)
    nws = L.ssg_conv_wgrad_workspace_bytes(B * H * W, cout, k, k, cin)
    assert n >= 1 and nws == 4 * n * cout * k * k * cin
    ws = _nan(nws // 4 + 64)                               # 64 floats of guard behind the workspace
    s = dw.stride()
    check(L.ssg_conv_wgrad_f32(ptr(gy), ptr(x), B, H, W, cin, cout, k, k, ptr(dw), s[0], s[1], s[2], s[3], ptr(ws), nws, 3, stream()), "wgrad")
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[nws // 4:]).all()) and not bool(torch.isnan(ws[:nws // 4]).any())     # all of the workspace, nothing past it
    return dict(y=y.permute(0, 3, 1, 2).cpu(), dx=dx.permute(0, 3, 1, 2).cpu(), dw=dw.cpu(), w_fwd=wf.cpu(), w_dgrad=wd.cpu())


def _check(case, got, which=OUTS):
    tc.check_bound(ref.reference, case, got, which)


@pytest.mark.parametrize("name", ALL)
def test_conv2d_train_against_float64(name):
    case = _case(name)
    got = _api(case)
    _check(case, got)
    assert got["y"].is_contiguous(memory_format=CL) and got["dx"].is_contiguous(memory_format=CL)


@pytest.mark.parametrize("name", ALL)
def test_entry_points_against_float64(name):
    case = _case(name)
    got = _abi(case)
    _check(case, got)
    w = ref.reference(*case)[0]["w"]
    assert torch.equal(got["w_fwd"], ref.pack_fwd(w)) and torch.equal(got["w_dgrad"], ref.pack_dgrad(w))   # the packings move bits
    api = _api(case)
    for o in OUTS:                                          # the autograd function adds nothing of its own
        assert torch.equal(api[o].cpu(), got[o]), o


def test_multi_slice_cases_have_a_real_slice_sum():
    L = _lib()
    for name in ref.MULTI:
        B, H, W, cin, cout, k, _ = _case(name)
        assert B <= 64
        n = L.ssg_conv_wgrad_num_slices(B * H * W, cout, k, k, cin)
        assert n >= 3 and (B * H * W) % n != 0             # equal slices cannot cover M: the last one is shorter
        assert L.ssg_conv_wgrad_num_slices((B - 1) * H * W, cout, k, k, cin) < 3


def test_real_cases_have_three_slices_and_ragged_tiles():
    """every real-width case: exactly three weight-gradient slices of which the last is shorter (from the library's own count, so a
    later change of the plan cannot quietly turn these into one-slice cases), and a ragged last 128-row tile in the forward and in
    the data gradient"""
    L = _lib()
    pairs = set()
    for name, (B, H, W, cin, cout, k, _) in ref.REAL.items():
        M = B * H * W
        assert 512 < M < 768 and M % 256 != 0 and M % 128 != 0, name
        n = L.ssg_conv_wgrad_num_slices(M, cout, k, k, cin)
        assert n == 3 and M % n != 0, (name, n)             # equal slices cannot cover M: the last one is shorter
        assert L.ssg_conv_wgrad_workspace_bytes(M, cout, k, k, cin) == 4 * 3 * cout * k * k * cin
        pairs.add((cin, cout, k))
    assert len(pairs) == len(ref.REAL) == 16 and max(p[0] for p in pairs) == 2048 and max(p[1] for p in pairs) == 2048


def _abi_gemm(name):
    """a TRAINER case through the raw entry points -> ({y, dx, dw} on the device in NHWC / [Cout, Cin], slice count n); the workspace
    is checked against its NaN guard"""
    from ssg_amd._lib import check, ptr, stream
    L = _lib()
    B, H, W, cin, cout, _ = ref.TRAINER[name]
    M = B * H * W
    d = ref.gemm_reference(name)[0]
    x, gy, w = d["x"].cuda(), d["gy"].cuda(), d["w"].cuda().view(cout, cin, 1, 1)
    wf, wd = _nan(cout, cin), _nan(cin, cout)
    s = w.stride()
    check(L.ssg_conv_pack_train_f32(ptr(w), s[0], s[1], s[2], s[3], cout, cin, 1, 1, ptr(wf), ptr(wd), stream()), "pack")
    zeros = torch.zeros(max(cin, cout), dtype=torch.float32, device="cuda")
    y, dx, dw = _nan(M, cout), _nan(M, cin), _nan(cout, cin, 1, 1)
    check(L.ssg_conv2d_nhwc_f32(ptr(x), ptr(wf), ptr(zeros), None, ptr(y), B, H, W, cin, cout, 1, 1, 1, 0, 0, stream()), "forward")
    check(L.ssg_conv2d_nhwc_f32(ptr(gy), ptr(wd), ptr(zeros), None, ptr(dx), B, H, W, cout, cin, 1, 1, 1, 0, 0, stream()), "dgrad")
    n = L.ssg_conv_wgrad_num_slices(M, cout, 1, 1, cin)
    nws = L.ssg_conv_wgrad_workspace_bytes(M, cout, 1, 1, cin)
    assert n >= 1 and nws == 4 * n * cout * cin
    ws = _nan(nws // 4 + 64)                               # 64 floats of guard behind the workspace
    s = dw.stride()
    check(L.ssg_conv_wgrad_f32(ptr(gy), ptr(x), B, H, W, cin, cout, 1, 1, ptr(dw), s[0], s[1], s[2], s[3], ptr(ws), nws, 3, stream()), "wgrad")
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[nws // 4:]).all()) and not bool(torch.isnan(ws[:nws // 4]).any())     # all of the workspace, nothing past it
    return dict(y=y, dx=dx, dw=dw.view(cout, cin)), n


def _gemm_rows(name, got, n):
    """[(output, L, max |dev - ref64|, worst err / bound)] of a TRAINER case: L = Cin for y, Cout for dx, the slice length bound for dw"""
    B, H, W, cin, cout, _ = ref.TRAINER[name]
    _, r64, A = ref.gemm_reference(name)
    rows = []
    for o, L in (("y", cin), ("dx", cout), ("dw", ref.slice_length_bound(B * H * W, n))):
        g = got[o].cpu().double()
        assert g.shape == r64[o].shape and bool(torch.isfinite(g).all()), o
        err = (g - r64[o]).abs()
        rows.append((o, L, float(err.max()), float((err / ref.bound(L, A[o]).clamp_min(1e-300)).max())))
    return rows


@pytest.mark.parametrize("name", sorted(ref.TRAINER))
def test_trainer_batch_1x1_against_float64_matmul(name):
    """layer1's two 1x1 shapes at the trainer's own B = 64, 64 x 32 pixels: M = 131072, hundreds of slices and a grid.z to match.  A
    1x1 convolution is a GEMM, so the reference is float64 matmuls (conv_train_ref.gemm_reference).

    y and dX: the usual (L + 2) 2^-24 A.  dW: (M + 2) 2^-24 A would be about 500 times looser than what the kernel's documented
    structure gives -- float32 partial sums over one slice each, the slices added in float64, one rounding.  A slice's partial sum
    errs by at most len 2^-24 A_slice, the A_slice add up to A, the float64 sum adds nothing visible and the rounding 2^-24 A, so

        |dW - ref64| <= (L_s + 2) 2^-24 A,   L_s = ceil(M / (n - 1)) >= len

    because n - 1 full slices of len pixels leave at least one pixel to the last: (n - 1) len < M.  n is the public slice count
    (ssg_conv_wgrad_num_slices); no constant of the kernel enters.  Also: the workspace is 4 n Cout K bytes, all of it and nothing
    behind it is written, and a second run gives the same bits."""
    B, H, W, cin, cout, _ = ref.TRAINER[name]
    got, n = _abi_gemm(name)
    assert n >= 256 and n == _lib().ssg_conv_wgrad_workspace_bytes(B * H * W, cout, 1, 1, cin) // (4 * cout * cin)
    for o, L, err, worst in _gemm_rows(name, got, n):
        print("%s %s: n = %d slices, L = %d, max |dev - ref64| = %.3g, worst err / bound = %.3g" % (name, o, n, L, err, worst))
        assert worst <= 1.0, "%s: %s misses (L + 2) 2^-24 A with L = %d by a factor of %.3g" % (name, o, L, worst)
    again, n2 = _abi_gemm(name)
    assert n2 == n
    for o in OUTS:
        assert torch.equal(again[o], got[o]), (name, o)


def test_layouts_give_the_same_bits():
    case = ref.CASES["3x3_cout192"]
    base = _api(case, x_cl=True, w_cl=False)
    assert base["dw"].is_contiguous() and base["dw"].shape == (192, 64, 3, 3)
    for x_cl, w_cl in [(False, False), (True, True), (False, True)]:
        got = _api(case, x_cl=x_cl, w_cl=w_cl)
        for o in OUTS:
            assert torch.equal(got[o], base[o]), (o, x_cl, w_cl)
        assert got["y"].is_contiguous(memory_format=CL) and got["dx"].is_contiguous(memory_format=CL)
        assert got["dw"].is_contiguous(memory_format=CL) if w_cl else got["dw"].is_contiguous()
        assert got["dw"].stride() == ((64 * 9, 1, 3 * 64, 64) if w_cl else (64 * 9, 9, 3, 1))


def test_frozen_input_and_frozen_weight():
    case = ref.CASES["3x3_border"]
    base = _api(case)
    got = _api(case, x_grad=False)
    assert got["dx"] is None and torch.equal(got["dw"], base["dw"]) and torch.equal(got["y"], base["y"])
    _check(case, got, ("y", "dw"))
    got = _api(case, w_grad=False)
    assert got["dw"] is None and torch.equal(got["dx"], base["dx"])
    _check(case, got, ("y", "dx"))


def test_two_passes_are_bit_identical():
    for name in ref.MULTI:
        case = _case(name)
        a, b = _api(case), _api(case)
        for o in OUTS:
            assert torch.equal(a[o], b[o]), (name, o)


def test_double_backward_raises():
    import ssg_amd
    d = ref.reference(*ref.CASES["1x1_ragged"])[0]
    x, w = d["x"].cuda().requires_grad_(True), d["w"].cuda().requires_grad_(True)
    y = ssg_amd.conv2d_train(x, w)
    (gx,) = torch.autograd.grad(y, x, d["gy"].cuda(), create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def test_shapes_outside_the_class():
    import ssg_amd
    nn = torch.nn
    x = torch.zeros(1, 64, 4, 4, device="cuda")
    w1 = torch.zeros(64, 64, 1, 1, device="cuda")
    with pytest.raises(ValueError, match="stride"):
        ssg_amd.conv2d_train(x, torch.zeros(64, 64, 3, 3, device="cuda"), 2, 1)
    with pytest.raises(ValueError, match="Cin"):
        ssg_amd.conv2d_train(torch.zeros(1, 3, 4, 4, device="cuda"), torch.zeros(64, 3, 1, 1, device="cuda"))
    with pytest.raises(ValueError, match="Cin"):
        ssg_amd.conv2d_train(torch.zeros(1, 96, 4, 4, device="cuda"), torch.zeros(64, 96, 1, 1, device="cuda"))
    with pytest.raises(ValueError, match="groups"):
        ssg_amd.conv2d_train(x, torch.zeros(64, 32, 1, 1, device="cuda"), groups=2)
    with pytest.raises(ValueError, match="bias"):
        ssg_amd.conv2d_train(x, w1, bias=torch.zeros(64, device="cuda"))
    m = nn.Sequential(nn.Conv2d(64, 64, 3, 2, 1, bias=False), nn.Conv2d(3, 64, 1, bias=False), nn.Conv2d(96, 64, 1, bias=False),
                      nn.Conv2d(64, 64, 1, groups=2, bias=False), nn.Conv2d(64, 64, 1, bias=True), nn.Conv2d(64, 128, 1, bias=False)).cuda()
    ssg_amd.use_device_conv(m)
    assert m._ssg_conv_skipped == ["0", "1", "2", "3", "4"]
    assert [isinstance(c, ssg_amd.Conv2d) for c in m] == [False] * 5 + [True]
    y = m[5](x)                                             # the swapped module runs on the device, also in eval mode and without grad
    with torch.no_grad():
        assert torch.equal(m[5].eval()(x), y)


# ---- composition -----------------------------------------------------------------------------------------------------------------------

COMP_SHAPE = (4, 64, 8, 4)
COMP_MARGIN = 2.0 ** -15


def _comp_inputs(g):
    return torch.randn(*COMP_SHAPE, generator=g), torch.randn(COMP_SHAPE[0], 256, *COMP_SHAPE[2:], generator=g)


@lru_cache(maxsize=None)
def _comp_data():
    """(block in float32 on the CPU, x, gy): the first seed whose ReLU inputs all stay COMP_MARGIN away from 0 in float64"""
    return tc.quiet_data(range(300, 400), lambda: ref.Bottleneck(64, 64, 1, ref.downsample(64, 256, 1)), _comp_inputs, 3, COMP_MARGIN)


def _comp_backward(b, x, gy):
    b(x).backward(gy)


@lru_cache(maxsize=None)
def _comp_refs():
    return tc.reference_grads(_comp_data(), 3, COMP_MARGIN, _comp_backward)


def _comp_device():
    import ssg_amd
    block, x, gy = _comp_data()
    b = copy.deepcopy(block).cuda()
    ssg_amd.use_device_conv(b)
    ssg_amd.use_device_batchnorm(b)
    assert b._ssg_conv_skipped == [] and b._ssg_bn_skipped == []
    assert all(isinstance(getattr(b, n), ssg_amd.Conv2d) for n in ("conv1", "conv2", "conv3")) and isinstance(b.downsample[0], ssg_amd.Conv2d)
    b = b.to(memory_format=CL)
    return tc.grads(b, lambda m: _comp_backward(m, x.cuda().contiguous(memory_format=CL), gy.cuda().contiguous(memory_format=CL)))


def measure_composition():
    """[(parameter, err_dev, err_f32)] of the composed block's parameter gradients"""
    g64, g32 = _comp_refs()
    return tc.composition_rows(g64, g32, _comp_device())


def test_composition_with_device_batchnorm():
    tc.check_composition(measure_composition(), F_COMP)


def measure():
    """[(case, path, output, max |dev - ref64|, max |f32 CPU - ref64|, worst err_dev / bound)] for tools/conv_train_errors.py"""
    rows = []
    for name in ALL:
        case = _case(name)
        rows += tc.bound_rows(ref.reference, ref.outputs, name, case, (("conv2d_train", _api(case)), ("entry points", _abi(case))), OUTS)
    for name in sorted(ref.TRAINER):                        # the float32 CPU column: the same three matmuls in float32; dw against the slice-aware bound
        B, H, W, cin, cout, _ = ref.TRAINER[name]
        d, r64, _ = ref.gemm_reference(name)
        f32 = dict(y=d["x"] @ d["w"].t(), dx=d["gy"] @ d["w"], dw=d["gy"].t() @ d["x"])
        got, n = _abi_gemm(name)
        for o, _, err, worst in _gemm_rows(name, got, n):
            rows.append((name, (B, H, W, cin, cout, 1), "entry points", o, err, float((f32[o].double() - r64[o]).abs().max()), worst))
    return rows
