"""GPU suite (-m gpu): the layer2 fused bottleneck block (csrc/bottleneck.hip, bottleneck_halves_kernel: four waves, y1 in channel
halves) against the three ssg_conv2d_nhwc_x launches it replaces.  Both run the same products in the same order, so every comparison
is bitwise on the h8l8 output container, and the range flag must agree.

Block: W = 16, C = 512, MID = 128; x is a ReLU output (about half of its values are zero), the weights are random convolutions
with BatchNorm scales spanning 10^4, folded with per-row power-of-two scales (resnet._fold).
"""
import copy

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C, MID, W = 512, 128, 16
_EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    from ssg_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def blk(dev):
    """folded conv1 / conv2 / conv3 of one identity block, as the embedder hands them to the kernels"""
    from ssg_amd import resnet
    g = torch.Generator().manual_seed(512128)

    def conv_bn(cout, cin, k, pad):
        sd = {"c.weight": torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5}
        f = 10.0 ** torch.randint(-2, 3, (cout,), generator=g).float()
        f = f / f.pow(2).mean().sqrt()
        var = torch.rand(cout, generator=g) + 0.5
        sd["b.weight"] = f * torch.sqrt(var + _EPS)
        sd["b.bias"] = 0.1 * torch.randn(cout, generator=g)
        sd["b.running_mean"] = 0.1 * torch.randn(cout, generator=g)
        sd["b.running_var"] = var
        return resnet._fold(sd, "c", "b", 1, pad, dev, split=True)
    return conv_bn(MID, C, 1, 0), conv_bn(MID, MID, 3, 1), conv_bn(C, MID, 1, 0)


def _x(L, dev, B, H, seed):
    from ssg_amd._lib import check, ptr, stream
    gd = torch.Generator(device=dev).manual_seed(seed)
    x = torch.relu(torch.randn(B, H, W, C, generator=gd, device=dev))
    xs = torch.empty_like(x)
    check(L.ssg_h8l8_encode(ptr(x), ptr(xs), x.numel(), 1.0, stream()), "enc")
    return xs


def _fused(L, xs, blk):
    """-> (out, flag) of ssg_bottleneck_nhwc_x"""
    from ssg_amd._lib import check, ptr, stream
    c1, c2, c3 = blk
    B, H = xs.shape[0], xs.shape[1]
    out = torch.empty_like(xs)
    flag = torch.zeros(1, dtype=torch.int32, device=xs.device)
    check(L.ssg_bottleneck_nhwc_x(ptr(xs), ptr(c1.w), ptr(c1.bias), ptr(c1.cscale), ptr(c2.w), ptr(c2.bias), ptr(c2.cscale), ptr(c3.w), ptr(c3.bias),
                                  ptr(c3.cscale), ptr(out), B, H, W, C, MID, ptr(flag), stream()), "bottleneck")
    return out, int(flag.item())


def _three(L, xs, blk):
    """-> (out, flag) of the three launches"""
    from ssg_amd.resnet import ResNet
    c1, c2, c3 = blk
    flag = torch.zeros(1, dtype=torch.int32, device=xs.device)
    o = ResNet._conv(L, xs, c1, out_split=True, ovf=flag)
    o = ResNet._conv(L, o, c2, out_split=True, ovf=flag)
    o = ResNet._conv(L, o, c3, res=xs, relu=True, out_split=True, ovf=flag)
    return o, int(flag.item())


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("B,H", [(1, 8), (1, 16), (2, 24), (3, 32)])
def test_halves_small_grid(B, H, L, dev, blk):
    """(1, 8): one tile, both halo rows outside the image; (1, 16): a halo shared between two tiles; (2, 24), (3, 32): interior
    tiles, image boundaries inside the grid"""
    assert L.ssg_bottleneck_supported(H, W, C, C, MID) == 1
    xs = _x(L, dev, B, H, 100 * H + B)
    o4, f4 = _fused(L, xs, blk)
    o3, f3 = _three(L, xs, blk)
    assert (f4, f3) == (0, 0)
    assert float(o3.abs().max()) > 0
    assert _same_bits(o4, o3), "fused block != the three launches"


@pytest.mark.parametrize("half", [0, 1])
def test_halves_channel_half_wiring(half, L, dev, blk):
    """conv1 non-zero only for the y1 channels of one half (weights and bias of the other half zero, so that half of y1 is exactly 0):
    a half that reached the wrong conv2 chunk, or the wrong LDS rows, would meet other W2 columns"""
    c1, c2, c3 = blk
    keep = torch.zeros(MID, dtype=torch.bool, device=dev)
    keep[half * 64:(half + 1) * 64] = True
    m1 = copy.copy(c1)
    m1.w = torch.where(keep.view(-1, 1), c1.w.view(torch.int32), 0).view(torch.float32).contiguous()   # (containers: no float arithmetic)
    m1.bias = (c1.bias * keep).contiguous()
    masked = (m1, c2, c3)
    xs = _x(L, dev, 2, 24, 7 + half)
    o4, f4 = _fused(L, xs, masked)
    o3, f3 = _three(L, xs, masked)
    full, _ = _three(L, xs, blk)
    assert (f4, f3) == (0, 0)
    assert not _same_bits(o3, full), "the mask changed nothing"
    assert _same_bits(o4, o3), "fused block != the three launches (y1 half %d only)" % half


def test_halves_co_residency_and_stage_reuse(L, dev, blk):
    """768 workgroups, more than one per CU and two at a time on each: the second phase-1 pass, the W2 / W3 stages and the patches
    reuse LDS that other waves were reading a barrier earlier"""
    xs = _x(L, dev, 192, 32, 19232)
    a, fa = _fused(L, xs, blk)
    b, fb = _fused(L, xs, blk)
    assert (fa, fb) == (0, 0)
    assert _same_bits(a, b), "second launch differs"
    del b
    o3, f3 = _three(L, xs, blk)
    assert f3 == 0
    assert _same_bits(a, o3), "fused block != the three launches"


def test_halves_overflow_flag(L, dev, blk):
    """one pixel of x scaled to 6e4 in every channel: its conv1 outputs leave the half range.  The fused block and the three launches both raise the
    flag, and agree on every pixel outside the 3 x 3 neighbourhood that conv2 spreads the non-finite values over"""
    from ssg_amd._lib import check, ptr, stream
    B, H, py, px = 2, 16, 9, 5
    xs = _x(L, dev, B, H, 4321)
    hot = torch.full((1, C), 6.0e4, device=dev)
    enc = torch.empty_like(hot)
    check(L.ssg_h8l8_encode(ptr(hot), ptr(enc), hot.numel(), 1.0, stream()), "enc")
    cold4, fc4 = _fused(L, xs, blk)
    assert fc4 == 0
    xs[1, py, px, :] = enc[0]
    o4, f4 = _fused(L, xs, blk)
    o3, f3 = _three(L, xs, blk)
    assert (f4, f3) == (1, 1)
    far = torch.ones(B, H, W, dtype=torch.bool, device=dev)
    far[1, py - 1:py + 2, px - 1:px + 2] = False
    assert _same_bits(o4[far], o3[far])
    assert _same_bits(o4[far], cold4[far]), "the hot pixel reached pixels beyond its 3 x 3 neighbourhood"
