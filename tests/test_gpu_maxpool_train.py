"""GPU suite of the train-mode MaxPool2d(3, 2, 1) (csrc/conv_strided.hip, ssg_amd/conv_strided.py) against torch's `F.max_pool2d` and
its autograd on the CPU (tests/conv_strided_ref.py).

The forward moves bits: it equals the float32 CPU pool exactly.  The backward adds at most four dY per input element (the 2 x 2
windows that can hold it), so every element satisfies |dev - ref64| <= (4 + 2) * 2^-24 * A with A the same gather applied to |dY| in
float64 -- and where ties decide which element of a window receives the gradient, the device follows torch's CPU rule (the first
maximum in row-major window order), or this bound fails by a whole dY."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_strided_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CL = torch.channels_last


def _api(name):
    import ssg_amd
    x, gy = ref.pool_reference(name)[:2]
    xd = x.cuda().contiguous(memory_format=CL).requires_grad_(True)
    y = ssg_amd.max_pool2d_train(xd)
    (dx,) = torch.autograd.grad(y, xd, gy.cuda())
    return y.detach(), dx


def _abi(name):
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    x, gy = ref.pool_reference(name)[:2]
    B, C, H, W = x.shape
    OH, OW = gy.shape[2:]
    xd = x.cuda().permute(0, 2, 3, 1).contiguous()
    g = gy.cuda().permute(0, 2, 3, 1).contiguous()
    nan = float("nan")
    y = torch.full((B, OH, OW, C), nan, device="cuda")
    dx = torch.full((B, H, W, C), nan, device="cuda")
    idx = torch.full((B * OH * OW * C + 64,), 255, dtype=torch.uint8, device="cuda")       # 64 guard bytes behind the winners
    check(L.ssg_maxpool3x3s2_idx_nhwc(ptr(xd), ptr(y), ptr(idx), B, H, W, C, stream()), "pool forward")
    check(L.ssg_maxpool3x3s2_bwd_nhwc(ptr(g), ptr(idx), ptr(dx), B, H, W, C, stream()), "pool backward")
    torch.cuda.synchronize()
    assert bool((idx[-64:] == 255).all()) and bool((idx[:-64] < 9).all())
    return y.permute(0, 3, 1, 2), dx.permute(0, 3, 1, 2)


@pytest.mark.parametrize("name", ref.POOL_CASES)
def test_max_pool_forward_and_backward(name):
    x, gy, y32, dx64, A = ref.pool_reference(name)
    for route in (_api, _abi):
        y, dx = route(name)
        assert y.shape == y32.shape and torch.equal(y.cpu(), y32), route.__name__
        err, lim = (dx.cpu().double() - dx64).abs(), (4 + 2) * ref.U * A
        print("%s %s: max |dX - ref64| = %.3g" % (name, route.__name__, float(err.max())))
        assert dx.shape == x.shape and bool((err <= lim).all()), (route.__name__, float(err.max()))
    (y1, d1), (y2, d2), (y3, d3) = _api(name), _api(name), _abi(name)
    assert torch.equal(d1, d2) and torch.equal(y1, y2)                            # run to run
    assert torch.equal(d1, d3) and torch.equal(y1, y3)                            # the autograd function adds nothing of its own
    assert y1.is_contiguous(memory_format=CL) and d1.is_contiguous(memory_format=CL)


def test_ties_follow_the_first_maximum():
    """the cases are what they claim: whole windows tie at 0 after a ReLU, and maxima repeat inside overlapping windows"""
    x = ref.pool_reference("relu")[0]
    y = ref.pool_reference("relu")[2]
    assert bool((y == 0).any())                                                    # a window of zeros only
    x = ref.pool_reference("dup")[0]
    win = torch.nn.functional.unfold(torch.nn.functional.pad(x, (1, 1, 1, 1), value=-1.0), 3, stride=2).reshape(2, 8, 9, -1)
    assert bool(((win == win.max(2, keepdim=True).values).sum(2) > 1).any())       # a repeated maximum
    # and the device puts each window's gradient on one element only: dX sums to dY
    gy = ref.pool_reference("dup")[1]
    _, dx = _api("dup")
    assert abs(float(dx.double().sum()) - float(gy.double().sum())) <= 1e-4 * float(gy.abs().sum())


def test_nan_and_minus_inf_forward():
    import torch.nn.functional as Fn
    import ssg_amd
    x = ref.pool_input("even").clone()
    x[0, 3, 1, 2] = float("nan")
    x[1, 5, 2, 3] = float("-inf")
    x[1, 7] = float("-inf")                                                        # a whole plane: every window is -inf
    want = Fn.max_pool2d(x, 3, 2, 1)
    with torch.no_grad():
        got = ssg_amd.max_pool2d_train(x.cuda()).cpu()
    assert bool(torch.isnan(want).any()) and bool(torch.isinf(want).any())
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    fill = torch.full_like(want, 123.0)
    assert torch.equal(torch.where(torch.isnan(got), fill, got), torch.where(torch.isnan(want), fill, want))   # bit-equal outside the NaNs


def test_module_and_swap_run_on_the_device():
    import ssg_amd
    m = torch.nn.Sequential(torch.nn.MaxPool2d(3, 2, 1), torch.nn.MaxPool2d(2))
    ssg_amd.use_device_maxpool(m)
    assert isinstance(m[0], ssg_amd.MaxPool2d) and m._ssg_maxpool_skipped == ["1"]
    x, _, y32 = ref.pool_reference("odd")[:3]
    assert torch.equal(m[0](x.cuda()).cpu(), y32)
    with pytest.raises(ValueError, match="C % 4"):
        ssg_amd.max_pool2d_train(torch.zeros(1, 6, 4, 4, device="cuda"))
