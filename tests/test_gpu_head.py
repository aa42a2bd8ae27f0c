"""GPU suite of the train-mode head (csrc/head_train.hip, ssg_amd/head.py): every case once through `stripe_pool_train` /
`linear_train` and once through the raw entry points, against torch's `F.avg_pool2d` / `F.linear` and their autograd in float64 on the
CPU (tests/head_ref.py).  Outputs handed to the raw entry points start as NaN, so an element that is not written shows.

Accuracy criterion, derived and not measured (the one of test_gpu_conv_train.py): every element of every output satisfies

    |dev - ref64| <= (L + 2) * 2^-24 * A

with L the length of that output's reduction (K for y, plus one term for the bias; N for dX; B for dW and db; the window size for the
pooled sets) and A the same operator applied to absolute values in float64.  The pool's backward is a reciprocal, a product and one
add per element: |dX - ref64| <= 4 * 2^-24 * A with A = |g0| / (h w) + |g_s| / ((h // S) w).

Composition (use_device_conv(strided=True) + use_device_maxpool + use_device_batchnorm + use_device_head on the look-alike model of
tests/head_ref.py, num_split = 2, num_classes = 0, loss = a fixed linear functional of all outputs): two forward + backward passes from
the same state give bit-equal parameter gradients, and against the float64 CPU run of the unswapped model

    err(device) <= F_COMP * err(float32 CPU run) + 2^-24,   err(v) = max |v - ref64| / max |ref64|

with F_COMP the next power of two above the largest ratio measured on the MI355X (profiles/head_errors.txt, written by
tools/head_errors.py from `measure()` / `measure_composition()` below) and never more than 4: measured 1.58
(base.layer4.0.conv1.weight), so F_COMP = 2.  The data keep every ReLU input at least 2^-15 away from 0 in float64 (asserted before anything touches the device)."""
import copy
import os
import sys
from functools import lru_cache

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_ref as ref  # noqa: E402
import train_common as tc  # noqa: E402
from train_common import FLOOR, _lib, _nan  # noqa: E402,F401

pytestmark = pytest.mark.gpu

F_COMP = 2.0
CL = torch.channels_last


# ---- stripe pooling ------------------------------------------------------------------------------------------------------------------------

def _pool_api(case, mask="all", x_cl=True):
    """one forward + backward through ssg_amd.stripe_pool_train -> (sets [nsets][B,C], dx [B,C,h,w]) as the device returned them"""
    import ssg_amd
    d = ref.pool_reference(*case)
    S = case[4]
    x = d["x"].cuda()
    x = (x.contiguous(memory_format=CL) if x_cl else x).requires_grad_(True)
    sets = ssg_amd.stripe_pool_train(x, S)
    assert isinstance(sets, tuple) and len(sets) == ref.nsets(S)
    idx = ref.present(S, mask)
    (dx,) = torch.autograd.grad([sets[i] for i in idx], x, [d["gs"][i].cuda() for i in idx])
    return [s.detach() for s in sets], dx


def _pool_abi(case, mask="all"):
    """the raw entry points; out and dX start as NaN, and so do the absent sets of g"""
    from ssg_amd._lib import check, ptr, stream
    L = _lib()
    B, h, w, C, S, _ = case
    d = ref.pool_reference(*case)
    n = ref.nsets(S)
    x = d["x"].cuda().permute(0, 2, 3, 1).contiguous()
    out, dx, g = _nan(n, B, C), _nan(B, h, w, C), _nan(n, B, C)
    check(L.ssg_gap_stripes(ptr(x), ptr(out), B, h, w, C, S, stream()), "ssg_gap_stripes")
    bits = 0
    for i in ref.present(S, mask):
        g[i].copy_(d["gs"][i])
        bits |= 1 << i
    check(L.ssg_gap_stripes_bwd(ptr(g), bits, ptr(dx), B, h, w, C, S, stream()), "ssg_gap_stripes_bwd")
    return [out[i] for i in range(n)], dx.permute(0, 3, 1, 2)


def _pool_fracs(case, got, mask):
    """[(output, max |dev - ref64|, worst err / bound)]; asserts nothing"""
    d = ref.pool_reference(*case)
    sets, dx = got
    rows = []
    for i, s in enumerate(sets):
        err, lim = (s.cpu().double() - d["sets"][i]).abs(), ref.bound(d["L"][i], d["A_sets"][i])
        assert s.shape == d["sets"][i].shape
        rows.append(("set%d" % i, float(err.max()), float((err / lim.clamp_min(1e-300)).max())))
    err, lim = (dx.cpu().double() - d["dx"][mask]).abs(), 4 * ref.U * d["A_dx"][mask]
    assert dx.shape == d["dx"][mask].shape
    # where A is 0 (a row in no stripe with set 0 absent) the reference is 0 and so must the device be
    rows.append(("dx", float(err.max()), float(torch.where(lim > 0, err / lim.clamp_min(1e-300), (err > 0).double() * 2).max())))
    return rows


def _pool_check(case, got, mask):
    sets, dx = got
    assert all(bool(torch.isfinite(s).all()) for s in sets) and bool(torch.isfinite(dx).all()), "an element was not written"
    for o, e, frac in _pool_fracs(case, got, mask):
        print("%s %s %s: max |dev - ref64| = %.3g, worst err / bound = %.3g" % (case[:5], mask, o, e, frac))
        assert frac <= 1.0, "%s %s: %s misses its bound by a factor of %.3g" % (case[:5], mask, o, frac)


@pytest.mark.parametrize("mask", ref.POOL_MASKS)
@pytest.mark.parametrize("name", tuple(ref.POOL_CASES))
def test_stripe_pool_against_float64(name, mask):
    case = ref.POOL_CASES[name]
    api, abi = _pool_api(case, mask), _pool_abi(case, mask)
    _pool_check(case, api, mask)
    _pool_check(case, abi, mask)
    for a, b in zip(api[0] + [api[1]], abi[0] + [abi[1]]):       # the autograd function adds nothing of its own
        assert torch.equal(a, b)
    assert api[1].is_contiguous(memory_format=CL)
    again = _pool_api(case, mask)                                # the same inputs give the same bits
    assert all(torch.equal(a, b) for a, b in zip(api[0] + [api[1]], again[0] + [again[1]]))


def test_stripe_pool_rows_in_no_stripe_and_layouts():
    case = ref.POOL_CASES["ragged_h"]                            # h = 7, S = 2: row 6 is in no stripe
    d = ref.pool_reference(*case)
    _, dx = _pool_api(case, "last")
    assert bool((dx[:, :, :3] == 0).all()) and bool((dx[:, :, 6] == 0).all()) and bool((dx[:, :, 3:6] != 0).all())
    _, dx = _pool_api(case, "set0")
    assert torch.equal(dx[:, :, 6], dx[:, :, 0]) and torch.equal(dx[:, :, 6].cpu(), (d["gs"][0] / torch.full_like(d["gs"][0], 21.0))[:, :, None].expand(-1, -1, 3))
    for name in ("ragged_h", "single", "real_c"):                # an x that is not channels_last gives the same values
        case = ref.POOL_CASES[name]
        a, b = _pool_api(case, "all", x_cl=True), _pool_api(case, "all", x_cl=False)
        assert all(torch.equal(p, q) for p, q in zip(a[0] + [a[1]], b[0] + [b[1]]))


def test_stripe_pool_sets_share_one_buffer_and_double_backward_raises():
    import ssg_amd
    x = ref.pool_reference(*ref.POOL_CASES["even"])["x"].cuda().contiguous(memory_format=CL).requires_grad_(True)
    sets = ssg_amd.stripe_pool_train(x, 2)
    B, C = sets[0].shape
    assert [s.data_ptr() - sets[0].data_ptr() for s in sets] == [0, 4 * B * C, 8 * B * C]     # slices of one [nsets, B, C] buffer
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(sets, ssg_amd.stripe_pool_train(x, 2)))
    with pytest.raises(RuntimeError):
        (gx,) = torch.autograd.grad(sets[1].sum(), x, create_graph=True)
        gx.sum().backward()


# ---- Linear ----------------------------------------------------------------------------------------------------------------------------------

def _lin_api(case, x_grad=True, w_grad=True):
    """one forward + backward through ssg_amd.linear_train -> {y, dx, dw, db} as the device returned them"""
    import ssg_amd
    d = ref.linear_reference(*case)[0]
    x = d["x"].cuda().requires_grad_(x_grad)
    w = d["w"].cuda().requires_grad_(w_grad)
    b = None if d["b"] is None else d["b"].cuda().requires_grad_(True)
    y = ssg_amd.linear_train(x, w, b)
    named = [("dx", x, x_grad), ("dw", w, w_grad), ("db", b, b is not None)]
    wrt = [(n, t) for n, t, need in named if need]
    out = dict(y=y.detach(), dx=None, dw=None, db=None)
    if wrt:
        out.update(zip([n for n, _ in wrt], torch.autograd.grad(y, [t for _, t in wrt], d["gy"].cuda())))
    return out


def _lin_abi(case):
    """the raw entry points; every output starts as NaN, with 64 floats of guard behind it that must stay NaN"""
    from ssg_amd._lib import check, ptr, stream
    L = _lib()
    B, K, N, bias, _ = case
    d = ref.linear_reference(*case)[0]
    x, w, gy = d["x"].cuda(), d["w"].cuda(), d["gy"].cuda()
    b = d["b"].cuda() if bias else None
    bufs = dict(y=_nan(B * N + 64), dx=_nan(B * K + 64), dw=_nan(N * K + 64), db=_nan(N + 64))
    check(L.ssg_linear_fwd_f32(ptr(x), ptr(w), ptr(b), ptr(bufs["y"]), B, K, N, stream()), "ssg_linear_fwd_f32")
    check(L.ssg_linear_dgrad_f32(ptr(gy), ptr(w), ptr(bufs["dx"]), B, K, N, stream()), "ssg_linear_dgrad_f32")
    check(L.ssg_linear_wgrad_f32(ptr(gy), ptr(x), ptr(bufs["dw"]), ptr(bufs["db"]) if bias else None, B, K, N, stream()), "ssg_linear_wgrad_f32")
    torch.cuda.synchronize()
    out = {}
    for o, shape in (("y", (B, N)), ("dx", (B, K)), ("dw", (N, K)), ("db", (N,))):
        n = shape[0] * (shape[1] if len(shape) > 1 else 1)
        written = o != "db" or bias
        assert bool(torch.isnan(bufs[o][n:]).all()), "%s: written past its end" % o
        assert bool(torch.isnan(bufs[o][:n]).any()) != written, "%s: %s" % (o, "an element was not written" if written else "db written without a bias")
        out[o] = bufs[o][:n].view(shape) if written else None
    return out


def _lin_fracs(case, got):
    _, r64, A, L = ref.linear_reference(*case)
    rows = []
    for o in ref.linear_outs(case):
        g = got[o].detach().cpu().double()
        assert g.shape == r64[o].shape and bool(torch.isfinite(g).all()), o
        err = (g - r64[o]).abs()
        rows.append((o, float(err.max()), float((err / ref.bound(L[o], A[o]).clamp_min(1e-300)).max()), L[o]))
    return rows


def _lin_check(case, got):
    for o, e, frac, L in _lin_fracs(case, got):
        print("%s %s: max |dev - ref64| = %.3g, worst err / bound = %.3g (L = %d)" % (case[:4], o, e, frac, L))
        assert frac <= 1.0, "%s: %s misses (L + 2) 2^-24 A by a factor of %.3g" % (case[:4], o, frac)


@pytest.mark.parametrize("name", tuple(ref.LINEAR_CASES))
def test_linear_against_float64(name):
    case = ref.LINEAR_CASES[name]
    api, abi = _lin_api(case), _lin_abi(case)
    _lin_check(case, api)
    _lin_check(case, abi)
    for o in ref.linear_outs(case):                              # the autograd function adds nothing of its own
        assert torch.equal(api[o], abi[o]), o
    assert api["db"] is None or case[3]
    again_api, again_abi = _lin_api(case), _lin_abi(case)        # the same inputs give the same bits
    for o in ref.linear_outs(case):
        assert torch.equal(api[o], again_api[o]) and torch.equal(abi[o], again_abi[o]), o


def test_linear_bias_gradient_alone():
    """dw = NULL: the bias gradient alone, the same bits, and x is not needed"""
    from ssg_amd._lib import check, ptr, stream
    case = ref.LINEAR_CASES["ragged"]
    B, K, N, _, _ = case
    gy = ref.linear_reference(*case)[0]["gy"].cuda()
    db = _nan(N)
    check(_lib().ssg_linear_wgrad_f32(ptr(gy), None, None, ptr(db), B, K, N, stream()), "ssg_linear_wgrad_f32")
    assert torch.equal(db, _lin_abi(case)["db"])


def test_linear_frozen_input_and_frozen_weight():
    for name in ("ragged", "one_tile"):
        case = ref.LINEAR_CASES[name]
        base = _lin_api(case)
        got = _lin_api(case, x_grad=False)
        assert got["dx"] is None and torch.equal(got["dw"], base["dw"]) and torch.equal(got["y"], base["y"])
        got = _lin_api(case, w_grad=False)
        assert got["dw"] is None and torch.equal(got["dx"], base["dx"])
        assert (got["db"] is None) == (not case[3]) and (got["db"] is None or torch.equal(got["db"], base["db"]))
    # the graph has no edge towards a frozen operand, so nothing is computed for it
    import ssg_amd
    d = ref.linear_reference(*ref.LINEAR_CASES["one_tile"])[0]
    y = ssg_amd.linear_train(d["x"].cuda().requires_grad_(True), d["w"].cuda())
    assert [f is None for f, _ in y.grad_fn.next_functions][:2] == [False, True]
    y = ssg_amd.linear_train(d["x"].cuda(), d["w"].cuda().requires_grad_(True))
    assert [f is None for f, _ in y.grad_fn.next_functions][:2] == [True, False]


def test_linear_module_in_train_and_eval_mode_and_double_backward():
    import ssg_amd
    case = ref.LINEAR_CASES["ragged"]
    d = ref.linear_reference(*case)[0]
    m = ssg_amd.Linear(case[1], case[2]).cuda()
    with torch.no_grad():
        m.weight.copy_(d["w"])
        m.bias.copy_(d["b"])
    y = m(d["x"].cuda())
    assert torch.equal(y, _lin_api(case)["y"])
    with torch.no_grad():
        assert torch.equal(m.eval()(d["x"].cuda()), y)
    y.backward(d["gy"].cuda())
    base = _lin_api(case)
    assert torch.equal(m.weight.grad, base["dw"]) and torch.equal(m.bias.grad, base["db"])
    with pytest.raises(RuntimeError):                            # a double backward raises
        x, w = d["x"].cuda().requires_grad_(True), d["w"].cuda().requires_grad_(True)
        (gx,) = torch.autograd.grad(ssg_amd.linear_train(x, w), x, d["gy"].cuda(), create_graph=True)
        gx.sum().backward()


# ---- composition -----------------------------------------------------------------------------------------------------------------------

COMP_SHAPE = (8, 3, 16, 8)
COMP_MARGIN = 2.0 ** -15


def _comp_inputs(g):
    B = COMP_SHAPE[0]
    return torch.randn(*COMP_SHAPE, generator=g), [torch.randn(B, 256, generator=g) for _ in range(3)] + [torch.randn(B, 128, generator=g)]


@lru_cache(maxsize=None)
def _comp_data():
    """(model in float32 on the CPU, x, the coefficients of the loss): the first seed whose ReLU inputs all stay COMP_MARGIN away from
    0 in float64; the ReLUs run 5 times: the stem's, the bottleneck's three and the head's"""
    return tc.quiet_data(range(700, 800), lambda: ref.HeadNet(num_split=2, num_classes=0), _comp_inputs, 5, COMP_MARGIN)


def _comp_backward(model, x, coef):
    outs = ref.flat_outputs(model(x))
    assert [tuple(o.shape) for o in outs] == [tuple(c.shape) for c in coef]
    sum((o * c).sum() for o, c in zip(outs, coef)).backward()          # a fixed linear functional of all outputs


@lru_cache(maxsize=None)
def _comp_refs():
    return tc.reference_grads(_comp_data(), 5, COMP_MARGIN, _comp_backward)


def _comp_device():
    import ssg_amd
    model, x, coef = _comp_data()
    m = copy.deepcopy(model).cuda()
    ssg_amd.use_device_conv(m, strided=True)
    ssg_amd.use_device_maxpool(m)
    ssg_amd.use_device_batchnorm(m)
    ssg_amd.use_device_head(m)
    assert m._ssg_conv_skipped == [] and m._ssg_maxpool_skipped == [] and m._ssg_bn_skipped == [] and m._ssg_linear_skipped == []
    assert isinstance(m, ssg_amd.DeviceHeadMixin) and isinstance(m.feat, ssg_amd.Linear) and isinstance(m.feat_bn, ssg_amd.BatchNorm1d)
    assert isinstance(m.base.conv1, ssg_amd.StridedConv2d) and isinstance(m.base.maxpool, ssg_amd.MaxPool2d)
    m = m.to(memory_format=CL)
    out = m(x.cuda().contiguous(memory_format=CL))
    assert isinstance(out, tuple) and len(out) == 2 and isinstance(out[0], list) and len(out[0]) == 3      # the reference's structure
    return tc.grads(m, lambda mod: _comp_backward(mod, x.cuda().contiguous(memory_format=CL), [c.cuda() for c in coef]))


def measure_composition():
    """[(parameter, err_dev, err_f32)] of the composed model's parameter gradients"""
    g64, g32 = _comp_refs()
    return tc.composition_rows(g64, g32, _comp_device())


def test_composition_is_bit_reproducible():
    _comp_refs()
    a, b = _comp_device(), _comp_device()
    assert sorted(a) == sorted(b) and len(a) > 0
    for n in a:
        assert torch.equal(a[n], b[n]), n


def test_composition_against_float64():
    tc.check_composition(measure_composition(), F_COMP, 32)


def test_device_head_alone_keeps_the_output_structure():
    """use_device_head alone, in eval mode: the structure of the unswapped model's outputs with and without for_eval, and the for_eval
    x1 is the concatenation of the same sets"""
    import ssg_amd
    model, x, _ = _comp_data()
    plain = copy.deepcopy(model).eval()                         # the unswapped model stays on the CPU
    dev = ssg_amd.use_device_head(copy.deepcopy(model).cuda().eval())
    with torch.no_grad():
        for kw in (dict(), dict(for_eval=True)):
            want, got = plain(x, **kw), dev(x.cuda(), **kw)
            assert type(want) is type(got) and len(want) == len(got) and type(want[0]) is type(got[0])
            assert [a.shape for a in ref.flat_outputs(want)] == [b.shape for b in ref.flat_outputs(got)]
        (x1, x2), (cat, x2e) = dev(x.cuda()), dev(x.cuda(), for_eval=True)
        assert torch.equal(torch.cat(x1, dim=1), cat) and torch.equal(x2, x2e)


def measure():
    """[(case, shape, path, output, max |dev - ref64|, worst err / bound)] for tools/head_errors.py"""
    rows = []
    for name, case in ref.POOL_CASES.items():
        for mask in ref.POOL_MASKS:
            for path, got in (("stripe_pool_train", _pool_api(case, mask)), ("entry points", _pool_abi(case, mask))):
                for o, e, frac in _pool_fracs(case, got, mask):
                    if o == "dx" or mask == "all":               # the forward does not depend on the mask
                        rows.append((name, case[:5], path, "%s/%s" % (o, mask) if o == "dx" else o, e, frac))
    for name, case in ref.LINEAR_CASES.items():
        for path, got in (("linear_train", _lin_api(case)), ("entry points", _lin_abi(case))):
            for o, e, frac, _ in _lin_fracs(case, got):
                rows.append((name, case[:4], path, o, e, frac))
    return rows
