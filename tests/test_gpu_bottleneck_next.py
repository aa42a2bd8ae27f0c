"""GPU suite (-m gpu): the next-conv instance of the layer1 fused bottleneck block (csrc/bottleneck.hip, bottleneck_kernel<..., NXT>,
reached through ssg_bottleneck_attach_next + ssg_bottleneck_nhwc_x).  The last layer1 block also runs conv1 of the following block on
the tile it has just produced and writes
    y1n    = relu(conv1_next(out))   -- must equal ssg_conv2d_nhwc_x(out, c1n) bit for bit, row-major or tiled c1n weights,
    out_s2 = out[:, ::2, ::2]        -- all the stride-2 downsample branch of the following block reads of out,
    out                              -- must equal the plain ssg_bottleneck_nhwc_x launch; skippable with a null pointer.
Every comparison is bitwise on the h8l8 containers; the range flag must agree with the two launches.

Block: W = 32, C = 256, MID = 64, MIDN = 128; x is a ReLU output, the weights are random convolutions with BatchNorm scales spanning
10^4, folded with per-row power-of-two scales (resnet._fold), as in test_gpu_bottleneck_l2_halves.py.
"""
import contextlib
import copy
import os

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C, MID, MIDN, W = 256, 64, 128, 32
_EPS = 1e-5
SHAPES = [(1, 4), (1, 8), (2, 12), (3, 12)]


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
    """folded conv1 / conv2 / conv3 of one identity block and conv1 of the next block, as the embedder hands them to the kernels"""
    from ssg_amd import resnet
    g = torch.Generator().manual_seed(25664128)

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
    return conv_bn(MID, C, 1, 0), conv_bn(MID, MID, 3, 1), conv_bn(C, MID, 1, 0), conv_bn(MIDN, C, 1, 0)


def _x(L, dev, B, H, seed):
    from ssg_amd._lib import check, ptr, stream
    gd = torch.Generator(device=dev).manual_seed(seed)
    x = torch.relu(torch.randn(B, H, W, C, generator=gd, device=dev))
    xs = torch.empty_like(x)
    check(L.ssg_h8l8_encode(ptr(x), ptr(xs), x.numel(), 1.0, stream()), "enc")
    return xs


def _block_rc(L, xs, blk, out, flag):
    """the bare return code of ssg_bottleneck_nhwc_x (whatever is attached rides along)"""
    from ssg_amd._lib import ptr, stream
    c1, c2, c3 = blk[:3]
    B, H = xs.shape[0], xs.shape[1]
    return L.ssg_bottleneck_nhwc_x(ptr(xs), ptr(c1.w), ptr(c1.bias), ptr(c1.cscale), ptr(c2.w), ptr(c2.bias), ptr(c2.cscale), ptr(c3.w), ptr(c3.bias),
                                   ptr(c3.cscale), ptr(out), B, H, xs.shape[2], xs.shape[3], MID, ptr(flag), stream())


def _plain(L, xs, blk):
    """-> (out, flag) of the plain launch"""
    from ssg_amd._lib import check
    out = torch.empty_like(xs)
    flag = torch.zeros(1, dtype=torch.int32, device=xs.device)
    check(_block_rc(L, xs, blk, out, flag), "bottleneck")
    return out, int(flag.item())


def _next(L, xs, blk, want_out=True, want_y1n=True, want_s2=True):
    """-> (out | None, y1n | None, out_s2 | None, flag) of the next-conv launch; the outputs start as a pattern no result holds"""
    from ssg_amd._lib import check, ptr
    c1n = blk[3]
    B, H = xs.shape[0], xs.shape[1]
    mk = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=xs.device)
    out = mk(B, H, W, C) if want_out else None
    y1n = mk(B, H, W, MIDN) if want_y1n else None
    s2 = mk(B, H // 2, W // 2, C) if want_s2 else None
    flag = torch.zeros(1, dtype=torch.int32, device=xs.device)
    check(L.ssg_bottleneck_attach_next(ptr(c1n.w), ptr(c1n.bias), ptr(c1n.cscale), ptr(y1n), ptr(s2), MIDN), "attach")
    check(_block_rc(L, xs, blk, out, flag), "bottleneck + next")
    return out, y1n, s2, int(flag.item())


def _conv1n(L, out, c1n, tiled):
    """-> (y1n, flag) of the launch the fusion removes"""
    from ssg_amd.resnet import ResNet
    flag = torch.zeros(1, dtype=torch.int32, device=out.device)
    if tiled:
        assert c1n.wt is not None, "no tiled copy of the c1n weights"
    return ResNet._conv(L, out, c1n, out_split=True, ovf=flag, tiled=tiled), int(flag.item())


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def refs(L, dev, blk):
    """per shape: x, the plain launch's out and flag -- computed once, shared, never written"""
    r = {}
    for B, H in SHAPES:
        xs = _x(L, dev, B, H, 1000 * H + B)
        out, f = _plain(L, xs, blk)
        r[(B, H)] = (xs, out, f)
    return r


@pytest.mark.parametrize("tiled", [False, True], ids=["rowmajor", "tiled"])
@pytest.mark.parametrize("B,H", SHAPES)
def test_next_matches_the_two_launches(B, H, tiled, L, blk, refs):
    """(1, 4): one tile, both halo rows are padding; (1, 8), (2, 12): halos across tiles and image boundaries; (3, 12): 9 tiles, not a
    multiple of the 8 XCDs"""
    assert L.ssg_bottleneck_next_supported(H, W, C, MID, MIDN) == 1
    xs, out0, f0 = refs[(B, H)]
    y0, fy = _conv1n(L, out0, blk[3], tiled)
    out, y1n, s2, f = _next(L, xs, blk)
    assert float(out0.abs().max()) > 0 and float(y0.abs().max()) > 0
    assert (f0, fy, f) == (0, 0, 0)
    assert _same_bits(out, out0), "out != the plain launch"
    assert _same_bits(y1n, y0), "y1n != ssg_conv2d_nhwc_x(out, c1n)"
    assert _same_bits(s2, out0[:, ::2, ::2]), "out_s2 != out[:, ::2, ::2]"


@pytest.mark.parametrize("B,H", SHAPES)
def test_next_null_outputs(B, H, L, blk, refs):
    """null out: the same y1n and out_s2; each of the other two skipped in turn leaves the rest unchanged"""
    xs, out0, _ = refs[(B, H)]
    y0, _ = _conv1n(L, out0, blk[3], False)
    out, y1n, s2, f = _next(L, xs, blk, want_out=False)
    assert out is None and f == 0
    assert _same_bits(y1n, y0) and _same_bits(s2, out0[:, ::2, ::2])
    out, y1n, s2, _ = _next(L, xs, blk, want_y1n=False)
    assert y1n is None and _same_bits(out, out0) and _same_bits(s2, out0[:, ::2, ::2])
    out, y1n, s2, _ = _next(L, xs, blk, want_s2=False)
    assert s2 is None and _same_bits(out, out0) and _same_bits(y1n, y0)


def test_next_range_flag_raised_by_y1n_alone(L, dev, blk, refs):
    """c1n rows scaled by 2^14 through the per-row scale the epilogue multiplies the accumulators by (the stored rows are h8l8
    containers): hi halves of y1n are infinite while out stays finite.  The flag is raised, as the separate c1n launch raises it,
    y1n carries the same bits, and out / out_s2 are still those of the plain launch."""
    xs, out0, f0 = refs[(2, 12)]
    hot = copy.copy(blk[3])
    hot.cscale = (blk[3].cscale * 16384.0).contiguous()
    y0, fy = _conv1n(L, out0, hot, False)
    assert f0 == 0 and fy == 1, "the scaled c1n does not leave the half range"
    out, y1n, s2, f = _next(L, xs, blk[:3] + (hot,))
    assert f == 1
    assert _same_bits(out, out0) and _same_bits(s2, out0[:, ::2, ::2])
    assert _same_bits(y1n, y0)


def test_attach_is_consumed_once(L, blk, refs):
    """the call after the fused one runs plain: it writes out and leaves y1n / out_s2 alone"""
    from ssg_amd._lib import check, ptr
    xs, out0, _ = refs[(1, 8)]
    c1n = blk[3]
    y1n = torch.full((1, 8, W, MIDN), float("nan"), device=xs.device)
    s2 = torch.full((1, 4, W // 2, C), float("nan"), device=xs.device)
    check(L.ssg_bottleneck_attach_next(ptr(c1n.w), ptr(c1n.bias), ptr(c1n.cscale), ptr(y1n), ptr(s2), MIDN), "attach")
    flag = torch.zeros(1, dtype=torch.int32, device=xs.device)
    check(_block_rc(L, xs, blk, None, flag), "fused")          # null out is legal only with a descriptor
    assert _same_bits(s2, out0[:, ::2, ::2]) and not torch.isnan(y1n).any()    # (finite halves never form a float32 NaN pattern)
    y1n.fill_(float("nan")); s2.fill_(float("nan"))
    out = torch.empty_like(xs)
    check(_block_rc(L, xs, blk, out, flag), "plain")
    torch.cuda.synchronize()
    assert _same_bits(out, out0)
    assert torch.isnan(y1n).all() and torch.isnan(s2).all(), "the second call still carried the descriptor"


def test_attach_with_unsupported_shape_is_an_error_and_clears(L, dev, blk, refs):
    """a layer2 block (W 16, C 512) has a plain kernel but no next-conv instance: error, not a plain launch; the slot is empty afterwards"""
    from ssg_amd._lib import check, ptr, stream
    assert L.ssg_bottleneck_supported(8, 16, 512, 512, 128) == 1 and L.ssg_bottleneck_next_supported(8, 16, 512, 128, MIDN) == 0
    c1n = blk[3]
    x2 = torch.zeros(1, 8, 16, 512, device=dev)
    out2 = torch.full_like(x2, float("nan"))
    y1n = torch.full((1, 8, 16, MIDN), float("nan"), device=dev)
    check(L.ssg_bottleneck_attach_next(ptr(c1n.w), ptr(c1n.bias), ptr(c1n.cscale), ptr(y1n), None, MIDN), "attach")
    z = torch.zeros(1, device=dev)   # (never read: the call fails before any launch)
    rc = L.ssg_bottleneck_nhwc_x(ptr(x2), ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), ptr(out2), 1, 8, 16, 512, 128, None, stream())
    assert rc == -1 and b"next-conv" in L.ssg_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out2).all() and torch.isnan(y1n).all(), "something was launched"
    xs, out0, _ = refs[(1, 8)]
    out, _ = _plain(L, xs, blk)
    assert _same_bits(out, out0) and torch.isnan(y1n).all(), "the failed call left the descriptor attached"


@contextlib.contextmanager
def _route(v):
    old = os.environ.get("SSG_BN_L1_NEXT")
    os.environ["SSG_BN_L1_NEXT"] = v
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SSG_BN_L1_NEXT", None)
        else:
            os.environ["SSG_BN_L1_NEXT"] = old


@pytest.fixture(scope="module")
def model(dev):
    import ssg_amd
    return ssg_amd.create("resnet50", num_classes=0, num_split=1, cluster=False, seed=1).cuda().eval()


def _embed_both_routes(model, imgs, monkeypatch):
    """-> (features with SSG_BN_L1_NEXT=0, with 1, [(x shape, stride2) of every dual launch of the second run])"""
    from ssg_amd.resnet import ResNet
    with _route("0"):
        a = model.embed_with_flip(imgs)
    seen = []
    real = ResNet._conv_dual

    def spy(L, o, x, c3, ds, **kw):
        seen.append((tuple(x.shape), kw.get("stride2")))
        return real(L, o, x, c3, ds, **kw)
    monkeypatch.setattr(ResNet, "_conv_dual", staticmethod(spy))
    with _route("1"):
        b = model.embed_with_flip(imgs)
    return a, b, seen


def test_embedder_routes_bit_equal(model, monkeypatch):
    """256 x 128 images, B = 3: the fused route gives the same features, and the layer2-entry dual launch is fed out_s2"""
    imgs = torch.randn(3, 3, 256, 128, generator=torch.Generator().manual_seed(11))
    a, b, seen = _embed_both_routes(model, imgs, monkeypatch)
    assert float(a.abs().max()) > 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    entry = [s for s in seen if s[0][3] == 256]          # the downsample operand of layer2's first block: layer1's 256 channels
    assert entry and all(s == ((3, 32, 16, 256), 1) for s in entry), seen
    assert all(s[1] is None for s in seen if s[0][3] != 256), seen


def test_embedder_other_input_size_keeps_the_old_route(model, monkeypatch):
    """64 x 32 images: layer1 is 16 x 8 pixels, no fused kernel: nothing changes, no dual launch reads a stride-1 operand"""
    imgs = torch.randn(3, 3, 64, 32, generator=torch.Generator().manual_seed(12))
    a, b, seen = _embed_both_routes(model, imgs, monkeypatch)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert seen and all(s[1] is None for s in seen), seen
