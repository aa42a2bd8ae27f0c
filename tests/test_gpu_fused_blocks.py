"""GPU suite (-m gpu): the fused stem and bottleneck kernels (csrc/stem_pool.hip, csrc/bottleneck.hip) through their C entry points,
against a float64 restatement of the same block (oracle/embed_oracle.py) -- at the batch sizes, workgroup counts and byte offsets
the embedder really runs them at, not only at the 2 or 3 images of the whole-model parity tests.

Per case: (1) the large launch equals the same images launched two at a time, bit for bit, twice in a row; (2) the values of the
images tests/embed_batch_ref.sample_images picks (batch ends, first / last tile of every XCD run, 2^30 / 2^31 byte-offset neighbours,
a seeded draw; every image when B <= 48) against float64; (3) the range flag stays down, and goes up for a bias channel at 1e5.

Tolerance of (2): err <= 4 * e32 + 2^-21 * max(1, |ref|max), with e32 the error of the float32 CPU restatement of the same block on
the same inputs against the float64 one.  2^-21: the representation step of the h8l8 format (test_conv_split_half_vs_fp64 grants the
same); 4: another fp32 summation order on the device, for a chain of three convolutions (the single-convolution twins use 2 and 3).
Nothing in the bound comes from the HIP path's output.  The reference consumes what the kernel consumes: the decoded input container
(the stem: images that are exact hi + lo sums) and the folded fp32 weights, in float64.  Every case prints one `fused-block-error`
line (pytest -s); profiles/fused_block_errors.txt is such a log.
Measured on an MI355X over the 76 lines: err / e32 between 0.35 and 2.53, err / bound at most 0.45 (the factor 4 is not needed in full).
"""
import pytest

import embed_batch_ref as ebr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    from ssg_amd import _lib
    return _lib.lib()


def _conv_bn(sd, g, name, cout, cin, k):
    """Kaiming (fan-in) convolution + BatchNorm whose per-channel scale gamma / sqrt(var + eps) takes the values 10^-2 .. 10^2
    (spanning 10^4), normalised to rms 1 so that a chain of them neither explodes nor dies"""
    sd[name + ".conv.weight"] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    f = 10.0 ** torch.randint(-2, 3, (cout,), generator=g).float()
    f = f / f.pow(2).mean().sqrt()
    var = torch.rand(cout, generator=g) + 0.5
    sd[name + ".bn.weight"] = f * torch.sqrt(var + _EPS)
    sd[name + ".bn.bias"] = 0.1 * torch.randn(cout, generator=g)
    sd[name + ".bn.running_mean"] = 0.1 * torch.randn(cout, generator=g)
    sd[name + ".bn.running_var"] = var


def _folded(sd, name):
    """the fp32 weights and bias resnet._fold hands the kernels (float64 fold, rounded once), as NCHW convolution weights"""
    w = sd[name + ".conv.weight"].double()
    scale = sd[name + ".bn.weight"].double() / torch.sqrt(sd[name + ".bn.running_var"].double() + _EPS)
    return (w * scale.view(-1, 1, 1, 1)).float(), (sd[name + ".bn.bias"].double() - sd[name + ".bn.running_mean"].double() * scale).float()


def _enc(L, x):
    from ssg_amd._lib import check, ptr, stream
    out = torch.empty_like(x)
    check(L.ssg_h8l8_encode(ptr(x), ptr(out), x.numel(), 1.0, stream()), "enc")
    return out


def _dec(L, x):
    from ssg_amd._lib import check, ptr, stream
    x = x.contiguous()
    out = torch.empty_like(x)
    check(L.ssg_h8l8_decode(ptr(x), ptr(out), x.numel(), 1.0, stream()), "dec")
    return out


def _nchw64(t):
    return t.cpu().permute(0, 3, 1, 2).contiguous().double()


def _judge(tag, got, ref64, ref32):
    """print the case's line, then the bound of the module docstring"""
    err = float((got - ref64).abs().max())
    e32 = float((ref32.double() - ref64).abs().max())
    scale = max(1.0, float(ref64.abs().max()))
    bound = 4.0 * e32 + 2.0 ** -21 * scale
    print("fused-block-error: %-44s images %2d  err %.3e  e32 %.3e  err/e32 %6.2f  |ref|max %9.3e  bound %.3e  err/bound %.3f"
          % (tag, got.shape[0], err, e32, err / e32 if e32 else float("inf"), scale, bound, err / bound))
    assert bool(torch.isfinite(got).all()) and err <= bound, (tag, err, e32, bound)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------ stem
@pytest.mark.parametrize("H,B", ebr.STEM_CASES)
def test_fused_stem_vs_fp64(H, B, L, dev):
    from oracle import embed_oracle
    from ssg_amd import resnet
    from ssg_amd._lib import check, ptr, stream
    assert L.ssg_stem_pool_supported(H, 128) == 1
    g = torch.Generator().manual_seed(1000 * H + B)
    sd = {}
    _conv_bn(sd, g, "s", 64, 3, 7)
    f = resnet._fold({"c.weight": sd["s.conv.weight"], "b.weight": sd["s.bn.weight"], "b.bias": sd["s.bn.bias"], "b.running_mean": sd["s.bn.running_mean"],
                      "b.running_var": sd["s.bn.running_var"]}, "c", "b", 2, 3, dev, split=True)
    wf, bf = _folded(sd, "s")
    gd = torch.Generator(device=dev).manual_seed(7 * H + B)
    x = torch.randn(B, 3, H, 128, generator=gd, device=dev)
    x[0, :, 0, 0] *= 1e-4                                   # a pixel of tiny values (half-subnormal lo parts)
    hi = x.half().float()
    x = hi + (x - hi).half().float()                        # exactly what the kernel's own hi / lo encoding keeps of an image
    OHP = H // 4
    flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def run(lo, hi_, flip, bias=f.bias):
        out = torch.empty(hi_ - lo, OHP, 32, 64, device=dev)
        check(L.ssg_stem_pool_nchw_x(ptr(x[lo:hi_]), flip, ptr(f.w), ptr(bias), ptr(f.cscale), ptr(out), hi_ - lo, H, 128, ptr(flag), stream()), "stem")
        return out
    idx = ebr.sample_images(B, ebr.stem_strips(H), OHP * 32 * 64 * 4)
    xs64 = x[torch.tensor(idx, device=dev)].cpu().double()
    for flip in (0, 1):
        big = run(0, B, flip)
        small = torch.cat([run(lo, min(lo + 2, B), flip) for lo in range(0, B, 2)], 0)
        assert _same_bits(big, small), "large launch != the same images two at a time (flip %d)" % flip
        assert _same_bits(run(0, B, flip), big), "second run differs (flip %d)" % flip
        got = _nchw64(_dec(L, big[torch.tensor(idx, device=dev)]))
        ref64 = embed_oracle.stem(xs64, wf.double(), bf, flip=bool(flip))
        ref32 = embed_oracle.stem(xs64.float(), wf, bf, flip=bool(flip))
        _judge("stem %dx128 B=%d flip=%d" % (H, B, flip), got, ref64, ref32)
    assert int(flag.item()) == 0
    hot = f.bias.clone(); hot[35] = 1.0e5
    run(0, B, 1, hot)
    assert int(flag.item()) == 1


# ------------------------------------------------------------------ bottleneck blocks
@pytest.mark.parametrize("C,MID,CIN,H,W,B", ebr.BNECK_CASES)
def test_fused_bottleneck_vs_fp64(C, MID, CIN, H, W, B, L, dev):
    from oracle import embed_oracle
    from ssg_amd import resnet
    from ssg_amd._lib import check, ptr, stream
    assert L.ssg_bottleneck_supported(H, W, CIN, C, MID) == 1
    down = CIN != C
    g = torch.Generator().manual_seed(C + 3 * CIN + 1000 * H + B)
    sd = {}
    _conv_bn(sd, g, "1", MID, CIN, 1); _conv_bn(sd, g, "2", MID, MID, 3); _conv_bn(sd, g, "3", C, MID, 1)
    if down:
        _conv_bn(sd, g, "d", C, CIN, 1)

    def fold(name, pad, split):
        return resnet._fold({"c.weight": sd[name + ".conv.weight"], "b.weight": sd[name + ".bn.weight"], "b.bias": sd[name + ".bn.bias"],
                             "b.running_mean": sd[name + ".bn.running_mean"], "b.running_var": sd[name + ".bn.running_var"]}, "c", "b", 1, pad, dev, split=split)
    c1, c2 = fold("1", 0, True), fold("2", 1, True)
    if down:        # conv3 | downsample weights along K under one row scale, biases summed (resnet.ResNet._prepare)
        c3, ds = fold("3", 0, False), fold("d", 0, False)
        wcat = torch.cat([c3.w, ds.w], dim=1).cpu()
        sc = resnet._row_scales(wcat)
        w3 = resnet._h8l8(wcat * sc.view(-1, 1)).to(dev); cs3 = (1.0 / sc).contiguous().to(dev); b3 = (c3.bias + ds.bias).contiguous()
    else:
        c3 = fold("3", 0, True)
        w3, cs3, b3 = c3.w, c3.cscale, c3.bias
    (w1f, b1f), (w2f, b2f), (w3f, _) = _folded(sd, "1"), _folded(sd, "2"), _folded(sd, "3")
    dsf = (_folded(sd, "d")[0], torch.zeros(C)) if down else None
    b3f = b3.cpu()                                          # (the downsample block: the fp32 sum of the two folded biases, as the kernel gets it)

    gd = torch.Generator(device=dev).manual_seed(11 * H + B + CIN)
    x = torch.relu(torch.randn(B, H, W, CIN, generator=gd, device=dev))
    x[0, 0, 0, :] *= 1e-4                                   # a pixel of tiny activations (half-subnormal lo parts)
    xs = _enc(L, x)
    del x
    flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def run(lo, hi, bias3=b3):
        out = torch.empty(hi - lo, H, W, C, device=dev)
        if down:
            check(L.ssg_bottleneck_ds_nhwc_x(ptr(xs[lo:hi]), ptr(c1.w), ptr(c1.bias), ptr(c1.cscale), ptr(c2.w), ptr(c2.bias), ptr(c2.cscale), ptr(w3), ptr(bias3),
                                             ptr(cs3), ptr(out), hi - lo, H, W, CIN, C, MID, ptr(flag), stream()), "bottleneck_ds")
        else:
            check(L.ssg_bottleneck_nhwc_x(ptr(xs[lo:hi]), ptr(c1.w), ptr(c1.bias), ptr(c1.cscale), ptr(c2.w), ptr(c2.bias), ptr(c2.cscale), ptr(w3), ptr(bias3),
                                          ptr(cs3), ptr(out), hi - lo, H, W, C, MID, ptr(flag), stream()), "bottleneck")
        return out
    big = run(0, B)
    small = torch.cat([run(lo, min(lo + 2, B)) for lo in range(0, B, 2)], 0)
    assert _same_bits(big, small), "large launch != the same images two at a time"
    del small
    assert _same_bits(run(0, B), big), "second run differs"
    assert int(flag.item()) == 0

    idx = torch.tensor(ebr.sample_images(B, ebr.bneck_tiles_img(C, H), H * W * C * 4), device=dev)
    x64 = _nchw64(_dec(L, xs[idx]))
    got = _nchw64(_dec(L, big[idx]))
    ref64 = embed_oracle.bottleneck(x64, (w1f, w2f, w3f), (b1f, b2f, b3f), dsf)
    ref32 = embed_oracle.bottleneck(x64.float(), (w1f, w2f, w3f), (b1f, b2f, b3f), dsf)
    assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32
    _judge("bottleneck %d/%d cin %d %dx%d B=%d" % (C, MID, CIN, H, W, B), got, ref64, ref32)

    hot = b3.clone(); hot[C // 2 + 3] = 1.0e5
    run(0, B, hot)
    assert int(flag.item()) == 1


def test_unsupported_shapes_are_refused_before_any_launch(L, dev):
    """the argument checks of the three entry points return before a launch: shapes without a kernel raise, nothing is written"""
    from ssg_amd._lib import check, ptr, stream
    t = torch.zeros(64, device=dev)
    out = torch.full((64,), 7.0, device=dev)
    for H, W in ((6, 128), (10, 128), (8, 64)):
        assert L.ssg_stem_pool_supported(H, W) == 0
        with pytest.raises(ValueError, match="unsupported shape"):
            check(L.ssg_stem_pool_nchw_x(ptr(t), 0, ptr(t), ptr(t), ptr(t), ptr(out), 1, H, W, None, stream()), "stem")
    for H, W, C, MID in ((10, 32, 256, 64), (12, 16, 256, 64), (12, 16, 512, 128), (8, 16, 512, 64)):
        assert L.ssg_bottleneck_supported(H, W, C, C, MID) == 0
        with pytest.raises(ValueError, match="unsupported block"):
            check(L.ssg_bottleneck_nhwc_x(ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(out), 1, H, W, C, MID, None, stream()), "bn")
    with pytest.raises(ValueError, match="unsupported block"):      # the downsample entry refuses an identity shape
        check(L.ssg_bottleneck_ds_nhwc_x(ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(out), 1, 12, 32, 256, 256, 64, None, stream()), "ds")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
