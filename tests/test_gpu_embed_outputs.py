"""GPU suite (-m gpu): the outputs of the embedder that nobody normalises, at more than one input size.

Every other value check of the embedder's tail compares (a + b) / ||a + b|| per pooled set at 256 x 128, which divides out any factor
common to one (image, set) row.  Here, against the float64 restatement (oracle/embed_oracle.py: feature_map, heads, sum_norm -- pinned to
the reference model's goldens by tests/test_embed_oracle.py), per input size, state dict, precision and num_split in 1, 2, 3:
  1. feature_map(x) and feature_map(x, flip=True), the decoded layer4 map;
  2. x1, x2 = model(x, False): every un-normalised pooled set and x2 = relu(feat_bn(feat(x1[0])));
  3. model(x, True)[0] == torch.cat(x1, 1) bit for bit;
  4. embed_with_flip(x, for_eval=True): the S + 1 sets under ONE norm (the ratio between the whole-map set and the stripes is part of
     the value), and extract_embeddings over the uneven batches 3 + 1 returns the same bits;
  5. embed_with_flip(x), per set, inside the 5e-6 every golden test uses;
  6. split: no range flag, no warning, and the same bits with SSG_FUSED_STEM=0 SSG_FUSED_BOTTLENECK=0 (launch per layer).
Sizes: 256 x 128 (the anchor), 384 x 128 (six stem strips, 12 x 4 map), 224 x 112 (W != 128: layout kernel + plain stem + stand-alone
max-pool, 7 x 4 map), 250 x 100 (H % 4 != 0: odd maps 125 x 50 -> 63 x 25 -> 32 x 13 -> 16 x 7 -> 8 x 4), 200 x 72 (7 x 3 map: a row in
no stripe), 64 x 32 (2 x 1 map: one-row stripes; num_split = 3 raises SSGError).

Tolerance of 1, 2, 4 -- the rule of tests/test_gpu_fused_blocks.py: err <= 4 * e32 + 2^-21 * max(1, |ref|max), e32 = the error of the
float32 CPU restatement of the same quantity against the float64 one.  Nothing in it comes from the HIP path.  Every check prints an
`embed-output-error` line (pytest -s); profiles/embed_output_errors.txt is such a log.
x2 is the one output with another multiple, 7: it is one more fp32 GEMM (K = 2048, fp32 matrix cores in both precisions) behind the
pooled map, and its terms cancel (sum |w g| is about 7 |x2|max under the synthetic weights).  The factor 4 covers "another fp32 summation
order on the device" for the chain that ends in x1 (tests/test_gpu_fused_blocks.py; its single-GEMM twins are granted 2 and 3); the
GEMM behind it adds its own order on top of the error it is handed, so 4 + 3.  Measured with the factor 4 on an MI355X: x2 fits at every
size under the checkpoint-like weights (err / e32 <= 3.43) and with precision='f32' (<= 3.75); with precision='split' under the synthetic
weights it came to err / e32 = 5.60 at 256 x 128 (err 3.85e-4 at |ref|max 145, e32 6.9e-5; the f32 path 3.38 on the same images) and
5.01 at 384 x 128 (f32: 2.95), while x1 -- the GEMM's input -- stayed at 2.78 and 2.01.  (e32 is a property of the host's float32
convolutions and moves by some percent between hosts: a second run on another host gave 5.95 for the same err.)  Every other output
holds the factor 4; the closest is a three-stripe x1 under checkpoint-like weights with precision='f32' at 384 x 128, err / e32 4.46,
0.95 of its bound.
"""
import warnings

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = [(256, 128, 4), (384, 128, 4), (224, 112, 4), (250, 100, 4), (200, 72, 4), (64, 32, 1), (64, 32, 5)]       # H, W, images
_SDS, _MODELS, _REF = {}, {}, {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda", 0)


def _sd(name):
    """'synthetic': seeded Kaiming weights; 'checkpoint-like': per-channel BatchNorm scales over 10^3 (tools/synth.py).  feat_bn drawn away
    from the identity, as test_x2_branch_matches_torch does, so that x2 checks the folding"""
    if name not in _SDS:
        import ssg_amd
        from synth import checkpoint_like_state_dict
        sd = dict(ssg_amd.synthetic_state_dict(seed=3) if name == "synthetic" else checkpoint_like_state_dict(7))
        g = torch.Generator().manual_seed(0)
        sd["feat_bn.running_mean"] = torch.randn(2048, generator=g) * 0.01; sd["feat_bn.running_var"] = torch.rand(2048, generator=g) + 0.5
        sd["feat_bn.weight"] = torch.rand(2048, generator=g) + 0.5; sd["feat_bn.bias"] = torch.randn(2048, generator=g) * 0.01
        _SDS[name] = sd
    return _SDS[name]


def _model(name, precision, num_split):
    """one model (one set of folded weights) per (state dict, precision); num_split only selects the pooling"""
    import ssg_amd
    if (name, precision) not in _MODELS:
        m = ssg_amd.create("resnet50", num_classes=0, num_split=2, cluster=False, pretrained=False, precision=precision).cuda().eval()
        m.load_state_dict(_sd(name), strict=False)
        _MODELS[(name, precision)] = m
    m = _MODELS[(name, precision)]
    m.num_split = num_split
    return m


def _images(H, W, B):
    return torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(1000 * H + W + B))


def _reference(name, H, W, B):
    """{(dtype, flip): layer4 map NCHW} of the float64 and the float32 restatement (shared by both precisions and every num_split)"""
    from oracle import embed_oracle as eo
    key = (name, H, W, B)
    if key not in _REF:
        x = _images(H, W, B)
        r = {}
        for dt in (torch.float64, torch.float32):
            sd = {k: v.to(dt) for k, v in _sd(name).items() if v.dtype.is_floating_point}
            with torch.no_grad():
                r[dt] = sd
                r[(dt, False)] = eo.feature_map(sd, x.to(dt))
                r[(dt, True)] = eo.feature_map(sd, eo.fliplr(x).to(dt))
        _REF[key] = r
    return _REF[key]


def _as_list(x1):
    return list(x1) if isinstance(x1, (list, tuple)) else [x1]


def _judge(tag, triples, mult=4.0):
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
    print("embed-output-error: %-58s err %.3e  e32 %.3e  err/e32 %6.2f  |ref|max %9.3e  bound %.3e  err/bound %.3f"
          % (tag, err, e32, err / e32 if e32 else float("inf"), scale, bound, r))
    assert finite and r <= 1.0, (tag, err, e32, bound)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _map_height(H):
    for _ in range(5):          # conv1, max-pool, layer2-4: each (H - 1) // 2 + 1
        H = (H - 1) // 2 + 1
    return H


@pytest.mark.parametrize("precision", ["split", "f32"])
@pytest.mark.parametrize("name", ["synthetic", "checkpoint-like"])
@pytest.mark.parametrize("H,W,B", SIZES)
def test_unnormalised_and_jointly_normalised_outputs(H, W, B, name, precision, dev, monkeypatch):
    import ssg_amd
    from oracle import embed_oracle as eo
    from ssg_amd import _lib
    L = _lib.lib()
    assert L.ssg_stem_pool_supported(H, W) == (1 if (W == 128 and H % 4 == 0) else 0)
    x = _images(H, W, B)
    ref = _reference(name, H, W, B)
    h4 = _map_height(H)
    assert ref[(torch.float64, False)].shape == (B, 2048, h4, _map_height(W))
    tag = "%dx%d B=%d %s %s" % (H, W, B, name, precision)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                          # no overflow fallback may be needed at any size
        m = _model(name, precision, 2)
        # 1. the layer4 map, both orientations
        fmaps = {}
        for flip in (False, True):
            fm = m.feature_map(x, flip=flip)
            assert fm.shape == (B, h4, _map_height(W), 2048)
            fmaps[flip] = fm
            _judge(tag + " feature_map flip=%d" % flip, [(fm.permute(0, 3, 1, 2), ref[(torch.float64, flip)], ref[(torch.float32, flip)])])
        assert not _same_bits(fmaps[False], fmaps[True])
        for S in (1, 2, 3):
            m = _model(name, precision, S)
            if S > h4:
                for call in (lambda: m(x, False), lambda: m(x, True), lambda: m.embed_with_flip(x), lambda: m.embed_with_flip(x, for_eval=True)):
                    with pytest.raises(ssg_amd.SSGError, match="num_split"):
                        call()
                    torch.cuda.synchronize()
                continue
            r64 = [eo.heads(ref[torch.float64], ref[(torch.float64, f)], S) for f in (False, True)]       # [(x1, x2) original, flipped]
            r32 = [eo.heads(ref[torch.float32], ref[(torch.float32, f)], S) for f in (False, True)]
            # 2. the un-normalised sets and x2
            x1, x2 = m(x, False)
            assert (isinstance(x1, list) and len(x1) == S + 1) if S > 1 else torch.is_tensor(x1)
            sets = _as_list(x1)
            _judge(tag + " S=%d x1 (un-normalised sets)" % S, list(zip(sets, _as_list(r64[0][0]), _as_list(r32[0][0]))))
            _judge(tag + " S=%d x2" % S, [(x2, r64[0][1], r32[0][1])], mult=7.0)
            # 3. for_eval only concatenates
            cat, x2e = m(x, True)
            assert _same_bits(cat, torch.cat(sets, 1)) and _same_bits(x2e, x2)
            # 4. one norm over all sets
            joint = m.embed_with_flip(x, for_eval=True)
            assert joint.shape == (B, len(sets) * 2048)
            j64, j32 = (eo.sum_norm(torch.cat(_as_list(r[0][0]), 1), torch.cat(_as_list(r[1][0]), 1)) for r in (r64, r32))
            _judge(tag + " S=%d embed_with_flip(for_eval=True)" % S, [(joint, j64, j32)])
            assert float((joint.double().norm(dim=1) - 1).abs().max()) < 1e-6
            feats, names, _ = ssg_amd.extract_embeddings(m, ssg_amd.TensorBatchLoader(x, 3), for_eval=True)
            assert len(names) == B and _same_bits(feats, joint), "extraction in batches of 3 differs from the single batch"
            # 5. per-set features
            per = m.embed_with_flip(x)
            p64 = torch.stack([eo.sum_norm(a, b) for a, b in zip(_as_list(r64[0][0]), _as_list(r64[1][0]))])
            per3 = per if per.dim() == 3 else per[None]
            assert per3.shape == p64.shape
            e5 = float((per3.cpu().double() - p64).abs().max())
            print("embed-output-error: %-58s err %.3e  (bound 5e-6)" % (tag + " S=%d embed_with_flip per set" % S, e5))
            assert e5 < 5e-6
            if S > 1:       # the joint form is the per-set form rescaled by ||set|| / ||all sets||: both views of one sum
                w = torch.stack([(a + b).norm(dim=1) for a, b in zip(r64[0][0], r64[1][0])])
                w = w / w.pow(2).sum(0).sqrt()
                assert float((joint.cpu().double().view(B, S + 1, 2048).permute(1, 0, 2) - per3.cpu().double() * w.unsqueeze(2)).abs().max()) < 1e-5
        # 6. split: flag down, and the launch-per-layer path gives the same bits
        assert not m._overflowed()
        if precision == "split":
            m = _model(name, precision, 2 if h4 >= 2 else 1)
            fused = [m._fmap(x, flip=f)[0].clone() for f in (False, True)] + [m.embed_with_flip(x, for_eval=True).clone()] + [t.clone() for t in _as_list(m(x, False)[0])]
            monkeypatch.setenv("SSG_FUSED_STEM", "0"); monkeypatch.setenv("SSG_FUSED_BOTTLENECK", "0")
            plain = [m._fmap(x, flip=f)[0].clone() for f in (False, True)] + [m.embed_with_flip(x, for_eval=True).clone()] + [t.clone() for t in _as_list(m(x, False)[0])]
            assert not m._overflowed()
            for i, (a, b) in enumerate(zip(fused, plain)):
                assert _same_bits(a, b), "output %d differs between the fused kernels and the launch-per-layer path" % i
