"""GPU suite (-m gpu): the BasicBlock embedders (resnet18 / resnet34) and the fused layer1 block (csrc/basicblock.hip).

1. ssg_basicblock_nhwc_x through its C entry point, in the manner of test_gpu_fused_blocks.test_fused_bottleneck_vs_fp64 (the same
   weight recipe: BatchNorm scales spanning 10^4, biases != 0, one pixel of tiny activations): bit-equal to the two
   ssg_conv2d_nhwc_x launches, to the same images launched one at a time and to a second run; against the float64 restatement
   (tests/basic_ref.basic_block) err <= 4 * e32 + 2^-21 * max(1, |ref|max), e32 = the error of the float32 CPU restatement on the
   same decoded inputs and folded weights (nothing in the bound comes from the kernel; 2^-21 = the h8l8 representation step, 4 =
   another fp32 summation order over a chain of convolutions, as test_gpu_fused_blocks grants); the range flag stays 0 and goes
   to 1 for a bias channel at 1e5 in conv2 AND, separately, in conv1 (the intermediate).  The cases put the first and the last
   band of an image next to each other (rows above / below the image are conv2's zero padding, not relu(b1)).
2. the whole models in both precisions against the golden of the real reference model and the float64 restatement, fused block
   on and off (bit-equal), no overflow fallback.
3. the drop-in surface on 512-wide features, 4. the embed -> distance -> eps -> DBSCAN chain on them against the oracle,
5. cluster=True on a 512-wide backbone.
Every case of 1 and 2 prints one `fused-block-error` line (pytest -s); profiles/basicblock_errors.txt is such a log.
"""
import contextlib
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest

import basic_ref
import test_gpu_fused_blocks as fb
from conftest import GOLDEN, bits
from oracle import embed_oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    from ssg_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------ 1. the fused block
BLOCK_CASES = ((4, 1),        # one band touching both image borders
               (8, 3),        # first and last band adjacent, odd batch
               (12, 2),       # first, inner and last band
               (64, 2))       # the real map


@pytest.mark.parametrize("H,B", BLOCK_CASES)
def test_fused_basicblock_vs_fp64(H, B, L, dev):
    from ssg_amd import resnet
    from ssg_amd._lib import check, ptr, stream
    W, C = 32, 64
    assert L.ssg_basicblock_supported(H, W, C) == 1
    g = torch.Generator().manual_seed(64 + 1000 * H + B)
    sd = {}
    fb._conv_bn(sd, g, "1", C, C, 3); fb._conv_bn(sd, g, "2", C, C, 3)

    def fold(name):
        return resnet._fold({"c.weight": sd[name + ".conv.weight"], "b.weight": sd[name + ".bn.weight"], "b.bias": sd[name + ".bn.bias"],
                             "b.running_mean": sd[name + ".bn.running_mean"], "b.running_var": sd[name + ".bn.running_var"]}, "c", "b", 1, 1, dev, split=True)
    c1, c2 = fold("1"), fold("2")
    (w1f, b1f), (w2f, b2f) = fb._folded(sd, "1"), fb._folded(sd, "2")
    gd = torch.Generator(device=dev).manual_seed(11 * H + B)
    x = torch.relu(torch.randn(B, H, W, C, generator=gd, device=dev))
    x[0, 0, 0, :] *= 1e-4                                   # a pixel of tiny activations (half-subnormal lo parts)
    xs = fb._enc(L, x)
    del x
    flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def run(lo, hi, bias1=c1.bias, bias2=c2.bias):
        out = torch.empty(hi - lo, H, W, C, device=dev)
        check(L.ssg_basicblock_nhwc_x(ptr(xs[lo:hi]), ptr(c1.w), ptr(bias1), ptr(c1.cscale), ptr(c2.w), ptr(bias2), ptr(c2.cscale), ptr(out),
                                      hi - lo, H, W, C, ptr(flag), stream()), "basicblock")
        return out

    def two_launches(bias1=c1.bias, bias2=c2.bias):
        o = torch.empty(B, H, W, C, device=dev); y = torch.empty(B, H, W, C, device=dev)
        check(L.ssg_conv2d_nhwc_x(ptr(xs), ptr(c1.w), ptr(bias1), None, ptr(o), B, H, W, C, C, 3, 3, 1, 1, 1, 3, 1.0, ptr(c1.cscale), ptr(flag), stream()), "conv1")
        check(L.ssg_conv2d_nhwc_x(ptr(o), ptr(c2.w), ptr(bias2), ptr(xs), ptr(y), B, H, W, C, C, 3, 3, 1, 1, 1, 3, 1.0, ptr(c2.cscale), ptr(flag), stream()), "conv2")
        return y
    big = run(0, B)
    assert fb._same_bits(big, two_launches()), "fused block != the two ssg_conv2d_nhwc_x launches"
    assert fb._same_bits(big, torch.cat([run(lo, lo + 1) for lo in range(B)], 0)), "large launch != the same images one at a time"
    assert fb._same_bits(run(0, B), big), "second run differs"
    assert int(flag.item()) == 0

    x64 = fb._nchw64(fb._dec(L, xs))
    got = fb._nchw64(fb._dec(L, big))
    ref64 = basic_ref.basic_block(x64, (w1f, w2f), (b1f, b2f))
    ref32 = basic_ref.basic_block(x64.float(), (w1f, w2f), (b1f, b2f))
    assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32
    fb._judge("basicblock 64 %dx%d B=%d" % (H, W, B), got, ref64, ref32)

    hot2 = c2.bias.clone(); hot2[C // 2 + 3] = 1.0e5        # the output leaves the half range
    run(0, B, bias2=hot2)
    assert int(flag.item()) == 1
    flag.zero_()
    hot1 = c1.bias.clone(); hot1[C // 2 + 3] = 1.0e5        # the INTERMEDIATE leaves the half range (the unfused path raises it for conv1's output)
    run(0, B, bias1=hot1)
    assert int(flag.item()) == 1
    flag.zero_()
    two_launches(bias1=hot1)
    assert int(flag.item()) == 1


def test_unsupported_basicblock_shapes_are_refused_before_any_launch(L, dev):
    from ssg_amd._lib import check, ptr, stream
    t = torch.zeros(64, device=dev)
    out = torch.full((64,), 7.0, device=dev)
    for H, W, C in ((10, 32, 64), (8, 16, 64), (8, 32, 128)):
        assert L.ssg_basicblock_supported(H, W, C) == 0
        with pytest.raises(ValueError, match="unsupported block"):
            check(L.ssg_basicblock_nhwc_x(ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(out), 1, H, W, C, None, stream()), "bb")
    with pytest.raises(ValueError, match="unsupported block"):      # out must not alias x
        check(L.ssg_basicblock_nhwc_x(ptr(out), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(out), 1, 8, 32, 64, None, stream()), "bb")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------ 2. whole models against the golden
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "embed_basic_ref.npz"))


@pytest.fixture(scope="module")
def imgs():
    return torch.randn(4, 3, 256, 128, generator=torch.Generator().manual_seed(1))       # the golden's images


@pytest.fixture(scope="module")
def ref_maps(imgs):
    """layer4 maps of the restatement, float64 and float32, both orientations, computed once per depth and left unchanged"""
    import ssg_amd
    cache = {}

    def get(depth):
        if depth not in cache:
            sd = ssg_amd.synthetic_state_dict(seed=1, depth=depth)
            with torch.no_grad():
                cache[depth] = (sd, {dt: [basic_ref.feature_map(sd, x, depth, dt) for x in (imgs, embed_oracle.fliplr(imgs))]
                                     for dt in (torch.float64, torch.float32)})
        return cache[depth]
    return get


def _ref_embed(sd, maps, dt, S, for_eval=False):
    sdd = {k: v.to(dt) for k, v in sd.items() if v.dtype.is_floating_point}
    a, b = (embed_oracle.heads(sdd, m, S, for_eval)[0] for m in maps[dt])
    if isinstance(a, list):
        return torch.stack([embed_oracle.sum_norm(x, y) for x, y in zip(a, b)])
    return embed_oracle.sum_norm(a, b).unsqueeze(0)


def _judge(tag, got, ref64, ref32, gold_ref=None):
    """the bound of the module docstring; the golden of the real reference model under the same bound plus the restatement's 1e-6"""
    got = got.double()
    err = float((got - ref64).abs().max())
    e32 = float((ref32.double() - ref64).abs().max())
    scale = max(1.0, float(ref64.abs().max()))
    bound = 4.0 * e32 + 2.0 ** -21 * scale
    print("fused-block-error: %-44s images %2d  err %.3e  e32 %.3e  err/e32 %6.2f  |ref|max %9.3e  bound %.3e  err/bound %.3f"
          % (tag, got.shape[-2], err, e32, err / e32 if e32 else float("inf"), scale, bound, err / bound))
    assert bool(torch.isfinite(got).all()) and err <= bound, (tag, err, e32, bound)
    if gold_ref is not None:
        gerr = float((got - torch.from_numpy(gold_ref).double()).abs().max())
        assert gerr <= bound + 1e-6, (tag, gerr, bound)


@pytest.mark.parametrize("precision", ("split", "f32"))
@pytest.mark.parametrize("depth", (18, 34))
def test_whole_model_vs_golden(depth, precision, gold, imgs, ref_maps, dev, monkeypatch):
    import ssg_amd
    monkeypatch.delenv("SSG_FUSED_BASICBLOCK", raising=False)
    sd, maps = ref_maps(depth)
    tag = "resnet%d %s" % (depth, precision)
    for S in (2, 1):
        m = ssg_amd.create("resnet%d" % depth, num_classes=0, num_split=S, cluster=False, seed=1, pretrained=False, precision=precision).cuda().eval()
        got = m.embed_with_flip(imgs).cpu()
        if S == 1:
            assert tuple(got.shape) == (4, 512)               # a single set comes back as [B, 512]
            got = got.unsqueeze(0)
        assert tuple(got.shape) == ((S + 1) if S > 1 else 1, 4, 512)
        key = "feats_r%d_S%d" % (depth, S)
        _judge("%s embed S=%d" % (tag, S), got, _ref_embed(sd, maps, torch.float64, S), _ref_embed(sd, maps, torch.float32, S),
               gold[key] if key in gold.files else None)
        if S == 2:
            ev = m.embed_with_flip(imgs, for_eval=True).cpu()
            assert tuple(ev.shape) == (4, 3 * 512)
            _judge("%s embed for_eval" % tag, ev.unsqueeze(0), _ref_embed(sd, maps, torch.float64, 2, True), _ref_embed(sd, maps, torch.float32, 2, True))
            x1, x2 = m(imgs, for_eval=True)
            r64 = embed_oracle.heads({k: v.double() for k, v in sd.items() if v.dtype.is_floating_point}, maps[torch.float64][0], 2, True)
            r32 = embed_oracle.heads(sd, maps[torch.float32][0], 2, True)
            assert tuple(x1.shape) == (4, 1536) and tuple(x2.shape) == (4, 2048)
            for name, g_, a, b in (("x1", x1, r64[0], r32[0]), ("x2", x2, r64[1], r32[1])):
                _judge("%s model(x, for_eval=True) %s" % (tag, name), g_.cpu().unsqueeze(0), a.unsqueeze(0), b.unsqueeze(0),
                       gold["%s_r18_S2_eval" % name][None] if depth == 18 else None)
        if precision == "split":
            monkeypatch.setenv("SSG_FUSED_BASICBLOCK", "0")
            plain = m.embed_with_flip(imgs).cpu()
            monkeypatch.setenv("SSG_FUSED_BASICBLOCK", "1")
            fused = m.embed_with_flip(imgs).cpu()
            monkeypatch.delenv("SSG_FUSED_BASICBLOCK")
            assert fb._same_bits(plain, fused), "fused layer1 blocks change the features"
            assert fb._same_bits(fused.reshape(got.shape), got)                 # (the default, whichever way it goes)
        assert m._twin is None and not m._overflowed(), "overflow fallback taken"


# ------------------------------------------------------------------ 3. drop-in surface
def test_dropin_surface_on_512_wide_features(imgs, dev):
    import ssg_amd
    from oracle import eval_oracle
    names = ["f%d" % i for i in range(4)]
    m = ssg_amd.create("resnet18", num_classes=0, num_split=2, pretrained=False).cuda()
    with contextlib.redirect_stdout(io.StringIO()):
        feats, labels = ssg_amd.extract_features(m, [(imgs, names, [0, 1, 2, 3], [0, 0, 0, 0])], for_eval=False)
    assert list(feats) == names
    for f in names:
        assert len(feats[f]) == 3 and all(tuple(v.shape) == (512,) for v in feats[f])
        assert all(abs(float(v.norm()) - 1.0) < 1e-5 for v in feats[f])
    im8 = torch.cat([imgs, imgs.flip(0) * 0.9], 0)            # 8 images, two per "identity"
    n8 = ["i%d" % i for i in range(8)]; pids = [0, 1, 2, 3, 3, 2, 1, 0]; cams = [0, 0, 0, 0, 1, 1, 1, 1]
    m1 = ssg_amd.create("resnet18", num_classes=0, num_split=1, pretrained=False).cuda()
    loader = [(im8, n8, pids, cams)]
    query = [(n8[i], pids[i], cams[i]) for i in range(4)]; gallery = [(n8[i], pids[i], cams[i]) for i in range(8)]
    with contextlib.redirect_stdout(io.StringIO()):
        top1 = ssg_amd.Evaluator(m1, print_freq=1).evaluate(loader, query, gallery)
        f8, _ = ssg_amd.extract_features(m1, loader)
        dist = ssg_amd.pairwise_distance(f8, query, gallery).numpy()
    assert tuple(f8["i0"].shape) == (512,) and dist.shape == (4, 8)
    assert top1 == eval_oracle.evaluate_all(dist, pids[:4], pids, cams[:4], cams)[2]


# ------------------------------------------------------------------ 4. embed -> grouping chain on 512-wide features
CHAIN_N, CHAIN_NS, CHAIN_IDS, CHAIN_RHO = 48, 16, 6, 0.1


def test_chain_on_512_wide_features_vs_oracle(dev, ora):
    """48 identity-carrying images -> extract_embeddings (resnet18, S = 2) -> compute_dist (k-reciprocal re-rank at its k1 = 20,
    k2 = 6) -> generate_selflabel, against the oracle on the same device features: distances bit for bit, eps, labels.
    rho = 0.1: eps is the mean of the 113 smallest of the 1128 pair distances (6 identities x 8 images have 168 same-identity
    pairs), so that DBSCAN (min_samples 4) finds identities (on the CPU restatement's features of such images: 3 to 6 clusters per
    split, none at the product's 1.6e-3); the oracle side, computed on the CPU, must return at least two clusters."""
    import ssg_amd
    from test_gpu_chain import identity_images
    timgs, _ = identity_images(CHAIN_N, CHAIN_IDS, 31, device=dev)
    simgs, _ = identity_images(CHAIN_NS, 4, 32, noise=0.5, device=dev)
    m = ssg_amd.create("resnet18", num_classes=0, num_split=2, pretrained=False, seed=1).cuda().eval()
    tf, _, _ = ssg_amd.extract_embeddings(m, ssg_amd.TensorBatchLoader(timgs, 20), for_eval=False)
    sf, _, _ = ssg_amd.extract_embeddings(m, ssg_amd.TensorBatchLoader(simgs, 20), for_eval=False)
    assert tuple(tf.shape) == (3, CHAIN_N, 512) and tuple(sf.shape) == (3, CHAIN_NS, 512) and bool(torch.isfinite(tf).all())
    tgts, srcs = [tf[s] for s in range(3)], [sf[s] for s in range(3)]
    args = SimpleNamespace(no_rerank=False, rho=CHAIN_RHO)
    with contextlib.redirect_stdout(io.StringIO()):
        e_list, r_list = ssg_amd.compute_dist(srcs, tgts, lambda_value=0.1, no_rerank=False, num_split=2)
        labels, clusters = ssg_amd.generate_selflabel(e_list, r_list, 0, args, [])
    oe, orr = ora.compute_dist([s.cpu().numpy() for s in srcs], [t.cpu().numpy() for t in tgts], 0.1, False)
    olabels, oeps = ora.generate_selflabel(oe, orr, 0, CHAIN_RHO, False)
    for s in range(3):
        assert np.array_equal(bits(r_list[s].final_dist().cpu().numpy()), bits(orr[s])), "final_dist of split %d" % s
        assert clusters[s].eps == oeps[s], "eps of split %d" % s
        assert np.array_equal(labels[s], olabels[s]), "labels of split %d" % s
    assert int(olabels[0].max()) + 1 >= 2, "the oracle side must find at least two clusters (choose rho accordingly)"


# ------------------------------------------------------------------ 5. cluster=True on a 512-wide backbone
def test_cluster_head_on_resnet18(imgs, dev):
    import ssg_amd
    m = ssg_amd.create("resnet18", num_classes=0, num_split=2, cluster=True, pretrained=False).cuda().eval()
    x1, x2 = m(imgs[:2], for_eval=True)                   # resnet.py:122-124: the concatenated sets, no assignment
    assert tuple(x1.shape) == (2, 1536) and tuple(x2.shape) == (2, 2048) and bool(torch.isfinite(x1).all())
    with pytest.raises(ValueError, match="1536.*2048"):
        m(imgs[:2])
    m1 = ssg_amd.create("resnet18", num_classes=0, num_split=1, cluster=True, pretrained=False).cuda().eval()
    with pytest.raises(ValueError, match="512.*2048"):    # resnet.py:131: a single [B, 512] set against the 2048-wide centres
        m1(imgs[:2])
