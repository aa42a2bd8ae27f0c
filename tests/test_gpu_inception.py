"""GPU suite (-m gpu): the InceptionNet embedder (ssg_amd/inception.py, csrc/inception.hip).

1. Values against the float64 restatement (tests/inception_ref.py, pinned to the reference model by tests/test_inception_host.py):
   feature_map(x) in both orientations, model(x) for (num_features 256, norm False / True), (0, False) and cut_at_pooling, and
   embed_with_flip(x), for precision in {split, f32} and weights in {synthetic, checkpoint-like}, at 3 images of 144 x 56 (maps
   73 x 29 -> 37 x 15 -> 19 x 8 -> 10 x 4; the stem's M = 24 192 is exactly 378 64-pixel tiles, everything behind the first pool is
   ragged), 2 images of 142 x 54 (even maps 72 x 28 -> 36 x 14 -> 18 x 7 -> 9 x 4) and 1 image of 64 x 32 (33 x 17 -> ... -> 5 x 3).
2. embed_with_flip on the reference golden's four images against the reference model's recorded output.
3. Every new kernel through the C ABI against torch on the CPU: the three pools bit for bit (odd sizes, channel-slice destinations whose
   surroundings must stay untouched), the convolutions (32 output channels from the 4-channel image layout and from 32 channels; 64
   channels into a slice, stride 2 and 1x1) against a float64 convolution.
4. Harness: extract_embeddings over uneven batches, refresh() from device-resident weights, no range flag.
5. Downstream: 256-wide unit-norm inception features through re_ranking_device -> eps_rule_dbscan == the oracle, bit for bit.

Tolerance of 1-3, the project's rule (tests/test_gpu_embed_outputs.py): err <= mult * e32 + 2^-21 * max(1, |ref|max), e32 = the error of
the float32 CPU restatement of the same quantity against the float64 one; mult = 4 up to the pooled map, 7 behind the `feat` GEMM, 2
for a single convolution.  Nothing in it comes from the HIP path.  Every check prints an `inception-output-error` line (pytest -s);
profiles/inception_errors.txt is such a log.
"""
import os
import warnings

import numpy as np
import pytest

import inception_ref as iref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional

SIZES = [(144, 56, 3), (142, 54, 2), (64, 32, 1)]          # H, W, images
_SDS, _MODELS, _REF = {}, {}, {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda", 0)


def _sd(name, nf=256):
    """'synthetic': reset_params' draw (seed 3); 'checkpoint-like': BatchNorm scales over more than 10^3 (tools/synth.py); nf = 0 is
    the same dict without feat / feat_bn"""
    if name not in _SDS:
        from ssg_amd import inception
        from synth import checkpoint_like_inception_state_dict
        _SDS[name] = inception.synthetic_state_dict(seed=3) if name == "synthetic" else checkpoint_like_inception_state_dict(7)
    sd = _SDS[name]
    return sd if nf else type(sd)((k, v) for k, v in sd.items() if not k.startswith("feat"))


def _model(name, precision, nf=256, norm=False, cut=False):
    import ssg_amd
    key = (name, precision, nf, norm, cut)
    if key not in _MODELS:
        m = ssg_amd.create("inception", num_features=nf, norm=norm, cut_at_pooling=cut, precision=precision).cuda().eval()
        m.load_state_dict(_sd(name, 0 if cut else nf), strict=True)
        _MODELS[key] = m
    return _MODELS[key]


def _images(H, W, B):
    return torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(1000 * H + W + B))


def _reference(name, H, W, B):
    """{dtype: state dict, (dtype, flip): block-6b map NCHW} of the float64 and the float32 restatement (shared by both precisions)"""
    key = (name, H, W, B)
    if key not in _REF:
        x = _images(H, W, B)
        r = {}
        for dt in (torch.float64, torch.float32):
            sd = {k: v.to(dt) for k, v in _sd(name).items() if v.dtype.is_floating_point}
            with torch.no_grad():
                r[dt] = sd
                r[(dt, False)] = iref.feature_map(sd, x.to(dt))
                r[(dt, True)] = iref.feature_map(sd, iref.fliplr(x).to(dt))
        _REF[key] = r
    return _REF[key]


def _judge(tag, triples, mult):
    """triples of (got, float64 reference, float32 restatement): assert the bound of the module docstring on each, print the worst"""
    worst = None
    for got, ref64, ref32 in triples:
        got = got.detach().cpu().double()
        assert got.shape == ref64.shape and ref64.dtype == torch.float64 and ref32.dtype == torch.float32, (tag, got.shape, ref64.shape)
        err = float((got - ref64).abs().max())
        e32 = float((ref32.double() - ref64).abs().max())
        scale = max(1.0, float(ref64.abs().max()))
        bound = mult * e32 + 2.0 ** -21 * scale
        rec = (err / bound, err, e32, scale, bound, bool(torch.isfinite(got).all()))
        if worst is None or rec[0] > worst[0] or not rec[5]:
            worst = rec
    r, err, e32, scale, bound, finite = worst
    print("inception-output-error: %-62s err %.3e  e32 %.3e  err/e32 %6.2f  |ref|max %9.3e  bound %.3e  err/bound %.3f"
          % (tag, err, e32, err / e32 if e32 else float("inf"), scale, bound, r))
    assert finite and r <= 1.0, (tag, err, e32, bound)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. values against the float64 restatement
@pytest.mark.parametrize("H,W,B", SIZES)
@pytest.mark.parametrize("name", ("synthetic", "checkpoint-like"))
@pytest.mark.parametrize("precision", ("split", "f32"))
def test_outputs_match_the_float64_restatement(precision, name, H, W, B, dev):
    x = _images(H, W, B)
    r = _reference(name, H, W, B)
    tag = "%s %s %dx%d B=%d" % (precision, name, H, W, B)
    sds = {dt: r[dt] for dt in (torch.float64, torch.float32)}
    nofeat = {dt: {k: v for k, v in sds[dt].items() if not k.startswith("feat")} for dt in sds}
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # a range-flag warning (fp32 recompute) fails the test
        m = _model(name, precision)
        for flip in (False, True):
            fm = m.feature_map(x, flip=flip)
            assert fm.shape[3] == 1536
            _judge(tag + " feature_map flip=%d" % flip, [(fm, r[(torch.float64, flip)].permute(0, 2, 3, 1), r[(torch.float32, flip)].permute(0, 2, 3, 1))], 4.0)
        with torch.no_grad():
            heads = {(nf, norm): [iref.head(sds[dt] if nf else nofeat[dt], r[(dt, False)], norm) for dt in (torch.float64, torch.float32)]
                     for nf, norm in ((256, False), (256, True), (0, False))}
            flipped = [iref.head(sds[dt], r[(dt, True)], False) for dt in (torch.float64, torch.float32)]
        for (nf, norm), (h64, h32) in heads.items():
            got = _model(name, precision, nf, norm)(x)
            assert tuple(got.shape) == (B, nf or 1536)
            _judge(tag + " model(x) num_features=%d norm=%s" % (nf, norm), [(got, h64, h32)], 7.0 if nf else 4.0)
        got = m(x, True)                                    # for_eval is accepted and ignored
        assert _same_bits(got, m(x)) and _same_bits(got, m.forward(x, False))
        cut = _model(name, precision, cut=True)(x)
        _judge(tag + " cut_at_pooling", [(cut, r[(torch.float64, False)], r[(torch.float32, False)])], 4.0)
        both = m.embed_with_flip(x)
        _judge(tag + " embed_with_flip", [(both, iref.sum_norm(heads[(256, False)][0], flipped[0]), iref.sum_norm(heads[(256, False)][1], flipped[1]))], 7.0)
    if precision == "split":
        assert not m._overflowed()


# ---- 2. the reference model's recorded output
@pytest.mark.parametrize("precision", ("split", "f32"))
def test_embed_with_flip_matches_the_reference_golden(precision, dev):
    import ssg_amd
    from conftest import GOLDEN
    from ssg_amd import inception
    gold = np.load(os.path.join(GOLDEN, "embed_inception_ref.npz"))
    imgs = torch.randn(4, 3, 144, 56, generator=torch.Generator().manual_seed(int(gold["image_seed"])))
    sd = inception.synthetic_state_dict(seed=int(gold["weight_seed"]))
    m = ssg_amd.create("inception", seed=int(gold["weight_seed"]), precision=precision).cuda().eval()
    got = m.embed_with_flip(imgs).cpu()
    ref = torch.from_numpy(gold["embed_with_flip_f256"])
    r64, r32 = iref.embed_with_flip(sd, imgs, dtype=torch.float64), iref.embed_with_flip(sd, imgs, dtype=torch.float32)
    e32 = float((r32.double() - r64).abs().max())
    err = float((got.double() - ref.double()).abs().max())
    bound = 7.0 * e32 + 2.0 ** -21 * max(1.0, float(ref.abs().max()))
    print("inception-output-error: %-62s err %.3e  e32 %.3e  err/e32 %6.2f  |ref|max %9.3e  bound %.3e  err/bound %.3f"
          % (precision + " embed_with_flip vs the reference golden", err, e32, err / e32, float(ref.abs().max()), bound, err / bound))
    assert tuple(got.shape) == (4, 256) and err <= bound
    assert float((got.norm(dim=1) - 1.0).abs().max()) < 1e-6


# ---- 3. the kernels through the C ABI
def _abi():
    from ssg_amd import _lib
    return _lib.lib(), _lib.check, _lib.ptr, _lib.stream


def _slice_ptr(t, coff):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + 4 * coff)


SENTINEL = 12345.0


def _check_slice(tag, out, coff, width, expected):
    """out [B,OH,OW,ld] on the device: the slice holds `expected` bit for bit, every other container still the sentinel"""
    got = out.cpu()
    assert _same_bits(got[..., coff:coff + width], expected), tag
    rest = torch.cat([got[..., :coff], got[..., coff + width:]], dim=-1)
    assert bool((rest == SENTINEL).all()), tag + ": bytes outside the slice were written"


POOL_SHAPES = [(1, 9, 5), (1, 10, 4), (2, 8, 8), (2, 73, 29)]          # B, H, W


@pytest.mark.parametrize("split", (0, 1))
@pytest.mark.parametrize("B,H,W", POOL_SHAPES)
def test_pools_are_bit_exact(B, H, W, split, dev):
    """MaxPool2d(2,2,1) dense (C = 32), MaxPool2d(3,2,1) into a slice (C = 64 at channels 128..191 of 256), AvgPool2d(3,1,1) dense and
    into a slice.  h8l8: the pool of the decoded containers, encoded again (inception_ref.pool_ref states the average's order)."""
    L, check, ptr, stream = _abi()
    g = torch.Generator().manual_seed(100 * H + W + B)
    for kind, k, s, p, C, ld, coff in (("max", 2, 2, 1, 32, 32, 0), ("max", 3, 2, 1, 64, 256, 128), ("avg", 3, 1, 1, 32, 32, 0), ("avg", 3, 1, 1, 64, 192, 64)):
        x = torch.randn(B, H, W, C, generator=g) * 3.0
        if kind == "max":
            x = x.relu()                                     # ties and zeros, as behind a ReLU
        xin = iref.encode_h8l8(x) if split else x
        src = iref.decode_h8l8(xin) if split else x
        ref = iref.pool_ref(src, kind, k, s, p)
        exp = iref.encode_h8l8(ref) if split else ref
        out = torch.full(tuple(ref.shape[:3]) + (ld,), SENTINEL, dtype=torch.float32, device=dev)
        xd = xin.to(dev)
        if kind == "max":
            check(L.ssg_inc_maxpool_nhwc_x(ptr(xd), _slice_ptr(out, coff), B, H, W, C, k, s, p, split, ld, stream()), "maxpool")
            assert ref.shape[1] == (H + 2 * p - k) // s + 1 and (k != 2 or H % 2 or ref.shape[1] == H // 2 + 1)
        else:
            check(L.ssg_inc_avgpool3_nhwc_x(ptr(xd), _slice_ptr(out, coff), B, H, W, C, split, ld, stream()), "avgpool")
        _check_slice("%s k=%d s=%d C=%d split=%d %dx%dx%d" % (kind, k, s, C, split, B, H, W), out, coff, C, exp)


def test_pool_and_conv_argument_checks(dev):
    L, check, ptr, stream = _abi()
    x = torch.zeros(1, 4, 4, 32, device=dev); out = torch.zeros(1, 4, 4, 64, device=dev)
    assert L.ssg_inc_maxpool_nhwc_x(ptr(x), ptr(out), 1, 4, 4, 30, 2, 2, 1, 0, 32, stream()) == -1          # C % 4
    assert L.ssg_inc_avgpool3_nhwc_x(ptr(x), ptr(out), 1, 4, 4, 32, 1, 16, stream()) == -1                  # out_ld < C
    assert L.ssg_inc_avgpool3_nhwc_x(ptr(x), _slice_ptr(out, 4), 1, 4, 4, 32, 1, 64, stream()) == -1        # h8l8 slice offset % 8
    assert L.ssg_inc_conv2d_nhwc_x(ptr(x), ptr(x), ptr(x), ptr(out), 1, 4, 4, 32, 48, 1, 1, 0, 1, 0, None, 64, None, stream()) == -1     # Cout % 32
    assert L.ssg_inc_conv2d_nhwc_x(ptr(x), ptr(x), ptr(x), ptr(out), 1, 4, 4, 32, 32, 1, 1, 0, 1, 1, None, 64, None, stream()) == -1     # split without ch_scale
    with pytest.raises(ValueError, match="2 GiB"):
        check(L.ssg_inc_conv2d_nhwc_x(ptr(x), ptr(x), ptr(x), ptr(out), 4096, 512, 512, 32, 32, 3, 1, 1, 1, 0, None, 32, None, stream()), "conv")


def _conv_case(cin, cout, k, stride, seed):
    """a convolution + BatchNorm drawn like the checkpoint-like weights -> (state dict of the unit 'u', fp64 / fp32 reference functions)"""
    g = torch.Generator().manual_seed(seed)
    sd = {"u.0.weight": torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cout * k * k)) ** 0.5}
    var = torch.exp(torch.empty(cout).uniform_(float(np.log(1e-3)), float(np.log(1e2)), generator=g))
    s = torch.exp(2.3 * torch.randn(cout, generator=g)); s = s / s.pow(2).mean().sqrt()
    sd.update({"u.1.weight": s * torch.sqrt(var + 1e-5), "u.1.bias": 0.05 * torch.randn(cout, generator=g),
               "u.1.running_mean": 0.1 * torch.randn(cout, generator=g), "u.1.running_var": var})
    return sd


CONVS = [(3, 32, 3, 1, 32, 0), (32, 32, 3, 1, 32, 0), (32, 64, 1, 1, 256, 128), (64, 64, 3, 2, 192, 64), (64, 128, 3, 1, 128, 0)]     # cin, cout, k, stride, out_ld, coff


@pytest.mark.parametrize("split", (0, 1))
@pytest.mark.parametrize("B,H,W", [(1, 9, 5), (1, 10, 4), (2, 8, 16)])     # M = 45, 40 and (stride 1) 256 = four 64-pixel tiles
@pytest.mark.parametrize("cin,cout,k,stride,ld,coff", CONVS)
def test_convolutions_against_float64(cin, cout, k, stride, ld, coff, B, H, W, split, dev):
    """relu(bn(conv(x))) of one unit: the kernel on the folded weights against the float64 convolution, mult = 2 (a single GEMM, the factor
    of tests/test_gpu_fused_blocks.py), e32 from the float32 CPU convolution; a slice destination keeps its surroundings"""
    from ssg_amd import resnet
    L, check, ptr, stream = _abi()
    pad = 1 if k == 3 else 0
    sd = _conv_case(cin, cout, k, stride, 7 * cin + cout + k)
    x = torch.randn(B, cin, H, W, generator=torch.Generator().manual_seed(H * W + B + cin))
    refs = {}
    for dt in (torch.float64, torch.float32):
        s = {kk: v.to(dt) for kk, v in sd.items()}
        refs[dt] = iref.unit(s, x.to(dt), "u", stride).permute(0, 2, 3, 1).contiguous()
    f = resnet._fold(sd, "u.0", "u.1", stride, pad, dev, split=bool(split))
    OH, OW = refs[torch.float64].shape[1:3]
    out = torch.full((B, OH, OW, ld), SENTINEL, dtype=torch.float32, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    if cin == 3:
        xin = torch.empty((B, H, W, 4), dtype=torch.float32, device=dev)
        xd = x.to(dev)
        check((L.ssg_nchw_to_nhwc4_h4l4 if split else L.ssg_nchw_to_nhwc4)(ptr(xd), ptr(xin), B, H, W, 0, stream()), "layout")
    else:
        nhwc = x.permute(0, 2, 3, 1).contiguous()
        xin = (iref.encode_h8l8(nhwc) if split else nhwc).to(dev)
    check(L.ssg_inc_conv2d_nhwc_x(ptr(xin), ptr(f.w), ptr(f.bias), _slice_ptr(out, coff), B, H, W, f.cin, cout, k, stride, pad, 1, 3 if split else 0,
                                  ptr(f.cscale), ld, ptr(ovf), stream()), "ssg_inc_conv2d_nhwc_x")
    got = out.cpu()
    rest = torch.cat([got[..., :coff], got[..., coff + cout:]], dim=-1)
    assert bool((rest == SENTINEL).all()), "bytes outside the slice were written"
    val = got[..., coff:coff + cout].contiguous()
    if split:
        val = iref.decode_h8l8(val)
        assert int(ovf.item()) == 0
    _judge("conv %d->%d %dx%d s%d %dx%dx%d %s" % (cin, cout, k, k, stride, B, H, W, "split" if split else "f32"), [(val, refs[torch.float64], refs[torch.float32])], 2.0)


def test_head_finish_relu_and_l2norm(dev):
    L, check, ptr, stream = _abi()
    x = torch.randn(5, 256, generator=torch.Generator().manual_seed(8))
    x[3] = 0.0                                               # F.normalize's eps: a zero row stays zero
    xd = x.to(dev)
    out = torch.empty_like(xd)
    check(L.ssg_inc_head_finish(ptr(xd), ptr(out), 5, 256, 0, stream()), "relu")
    assert torch.equal(out.cpu(), x.relu())
    check(L.ssg_inc_head_finish(ptr(xd), ptr(out), 5, 256, 1, stream()), "l2norm")
    ref = F.normalize(x.double())         # |out| <= 0.4 here; sum of 256 squares, sqrt and one division in fp32: below 2^-20 relative
    assert float((out.cpu().double() - ref).abs().max()) <= 2.0 ** -22 and float(out[3].abs().max()) == 0.0


# ---- 4. harness
@pytest.mark.parametrize("precision", ("split", "f32"))
def test_extraction_harness_and_refresh(precision, dev):
    import ssg_amd
    x = _images(144, 56, 4)
    m = _model("checkpoint-like", precision)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        one = m.embed_with_flip(x)
        feats, names, pids = ssg_amd.extract_embeddings(m, ssg_amd.TensorBatchLoader(x, 3), for_eval=False)            # batches 3 + 1
        assert _same_bits(feats, one) and len(names) == 4
        assert _same_bits(ssg_amd.extract_embeddings(m, ssg_amd.TensorBatchLoader(x, 3), for_eval=True)[0], one)      # whatever for_eval says
        fd, _ = ssg_amd.extract_features(m, ssg_amd.TensorBatchLoader(x, 3, ["a", "b", "c", "d"]), print_freq=100, for_eval=False)
        assert list(fd) == ["a", "b", "c", "d"] and _same_bits(torch.stack(list(fd.values())), one.cpu())
        assert _same_bits(ssg_amd.extract_cnn_feature(m, x, True), m(x).cpu())                                         # the single-tensor branch
        # refresh() from device-resident weights == load_state_dict() of the same weights, bit for bit (csrc/fold.hip == the host fold)
        fresh = ssg_amd.create("inception", precision=precision).cuda().eval()
        fresh.refresh({k: v.to(dev) for k, v in _sd("checkpoint-like").items()}, strict=True)
        assert all(v.is_cuda for k, v in fresh._sd.items())
        for a, b in zip(fresh._prepare()["stem"] + [fresh._prepare()["feat"]], m._prepare()["stem"] + [m._prepare()["feat"]]):
            assert _same_bits(a.w, b.w) and _same_bits(a.bias, b.bias)
        assert _same_bits(fresh.embed_with_flip(x), one)
    if precision == "split":
        assert not m._overflowed() and m._twin is None                 # no range flag on these inputs


def test_range_flag_recomputes_in_fp32(dev):
    """activations that leave the half range (pixels up to 6e4, which the image layout still holds, and a conv1 BatchNorm scale of 100):
    the split model warns once and returns the bits of the precision='f32' model"""
    import ssg_amd
    x = _images(64, 32, 1).clamp(-1.0, 1.0) * 6.0e4
    big = {"conv1.1.weight": torch.full((32,), 100.0)}
    m = ssg_amd.create("inception", seed=3, precision="split").cuda().eval()
    ref = ssg_amd.create("inception", seed=3, precision="f32").cuda().eval()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # (the other 240 keys keep their values)
        m.load_state_dict(big, strict=False); ref.load_state_dict(big, strict=False)
    with pytest.warns(UserWarning, match="half range"):
        got = m.embed_with_flip(x)
    assert m._twin is not None and _same_bits(got, ref.embed_with_flip(x)) and bool(torch.isfinite(got).all())


# ---- 5. downstream chain
def test_inception_features_through_the_grouping_chain(dev, ora):
    """tests/test_gpu_chain.py's chain at small size on a 256-wide set: N = 96 inception embeddings of identity-carrying 144 x 56 images
    and 64 seeded source features -> re_ranking_device -> eps_rule_dbscan == the oracle on the same features, bit for bit"""
    import ssg_amd
    from ssg_amd import cluster, rerank
    N, Ns = 96, 64
    g = torch.Generator().manual_seed(21)
    pat = torch.randn(12, 3, 18, 7, generator=g)
    imgs = pat[torch.arange(N) % 12].repeat_interleave(8, dim=2).repeat_interleave(8, dim=3) + 0.35 * torch.randn(N, 3, 144, 56, generator=g)
    m = _model("checkpoint-like", "split")
    tgt, _, _ = ssg_amd.extract_embeddings(m, ssg_amd.TensorBatchLoader(imgs, 40), for_eval=False)
    assert tuple(tgt.shape) == (N, 256) and float((tgt.norm(dim=1) - 1.0).abs().max()) < 1e-5
    src = torch.randn(Ns, 256, generator=g); src = (src / src.norm(dim=1, keepdim=True)).to(dev)
    h = rerank.re_ranking_device(src, tgt, lambda_value=0.1)
    oe, of = ora.re_ranking(src.cpu().numpy(), tgt.cpu().numpy(), lambda_value=0.1)
    assert np.array_equal(h.euclid.cpu().numpy().view(np.uint16), oe.view(np.uint16)), "euclidean_dist"
    assert np.array_equal(h.final_dist().cpu().numpy(), of), "final_dist"
    h2 = rerank.re_ranking_device(src, tgt, lambda_value=0.1, validate=False)
    eps, cnt, top, lab, _ = cluster.eps_rule_dbscan(h2, 1.6e-3, min_samples=4)
    oeps, ocnt, otop = ora.eps_rule(of, 1.6e-3)
    assert (eps, cnt, top) == (oeps, ocnt, otop), "eps rule"
    assert np.array_equal(lab, ora.dbscan(of, oeps, 4)), "labels"
    print("inception chain: N=%d eps %.5f, %d clusters, %d noise" % (N, eps, lab.max() + 1, int((lab < 0).sum())))
