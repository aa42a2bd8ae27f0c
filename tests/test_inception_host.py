"""CPU suite: the InceptionNet embedder on the host side -- factory, state-dict names / order / shapes against the real reference model's
listing, the restatement tests/inception_ref.py against the reference golden (tests/golden/embed_inception_ref.npz, tools/make_golden.py
--only-embed-inception), the host fold of its convolutions and of feat + feat_bn against float64, load_state_dict's leniency.
No GPU work."""
import os

import numpy as np
import pytest

import inception_ref
import ssg_amd
from conftest import GOLDEN

torch = pytest.importorskip("torch")
F = torch.nn.functional


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "embed_inception_ref.npz"))


@pytest.fixture(scope="module")
def imgs():
    return torch.randn(4, 3, 144, 56, generator=torch.Generator().manual_seed(1))        # the golden's images (image_seed = 1)


def test_factory_has_the_six_names_of_the_reference():
    from ssg_amd import inception, resnet
    assert ssg_amd.names() == ["inception", "resnet101", "resnet152", "resnet18", "resnet34", "resnet50"]
    assert resnet.names() == ["resnet101", "resnet152", "resnet18", "resnet34", "resnet50"]
    m = ssg_amd.create("inception")
    assert isinstance(m, inception.InceptionNet) and isinstance(m, ssg_amd.InceptionNet)
    assert (m.num_features, m.norm, m.cut_at_pooling, m.precision, m.training) == (256, False, False, os.environ.get("SSG_EMBED_PRECISION", "split"), False)
    assert ssg_amd.create("inception", num_features=0).num_features == 1536               # inception.py:82
    assert isinstance(ssg_amd.create("resnet18", pretrained=False), resnet.ResNet)
    with pytest.raises(KeyError):
        ssg_amd.create("resnet20")
    with pytest.raises(NotImplementedError, match="training-only path"):
        ssg_amd.create("inception", num_classes=1)
    with pytest.raises(ValueError, match="precision"):
        ssg_amd.create("inception", precision="bf16")
    assert m.eval() is m and m.module is m and m.train(False) is m
    with pytest.raises(NotImplementedError):
        m.train()
    with pytest.raises(ssg_amd.SSGError, match="GPU only"):
        m(torch.zeros(1, 3, 16, 8))                                                      # no CPU fallback


def test_state_dict_is_the_reference_models_listing(gold):
    from ssg_amd import inception
    sd = inception.synthetic_state_dict(seed=1)
    assert len(sd) == 241
    assert inception_ref.key_listing(sd) == [str(s) for s in gold["keys"]]               # the reference model's own state_dict(), in its order
    m = ssg_amd.create("inception", seed=1)
    assert list(m.state_dict()) == list(sd) and all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    assert tuple(sd["conv1.0.weight"].shape) == (32, 3, 3, 3) and tuple(sd["inception6b.branches.1.2.0.weight"].shape) == (256, 256, 3, 3)
    assert tuple(sd["feat.weight"].shape) == (256, 1536) and tuple(sd["feat.bias"].shape) == (256,)
    assert "feat.weight" not in inception.synthetic_state_dict(seed=1, num_features=0) and len(inception.synthetic_state_dict(1, 0)) == 234
    # reset_params (inception.py:127-139): identity BatchNorm, He fan-out convolutions, feat std 0.001
    assert float(sd["inception4a.branches.3.1.1.weight"].min()) == 1.0 and float(sd["feat_bn.running_var"].max()) == 1.0
    w = sd["inception5a.branches.1.1.0.weight"]
    assert abs(float(w.std()) / (2.0 / (128 * 9)) ** 0.5 - 1.0) < 0.02 and abs(float(sd["feat.weight"].std()) / 1e-3 - 1.0) < 0.02


@pytest.mark.parametrize("tag,nf,norm", (("model_f256", 256, False), ("model_f256_norm", 256, True), ("model_f0", 0, False)))
def test_restatement_matches_the_reference_golden(tag, nf, norm, gold, imgs):
    from ssg_amd import inception
    sd = inception.synthetic_state_dict(seed=1, num_features=nf)
    mine = inception_ref.forward(sd, imgs, norm).numpy()
    assert mine.shape == gold[tag].shape == (4, nf or 1536)
    assert np.abs(mine - gold[tag]).max() < 1e-6
    if tag == "model_f256":
        both = inception_ref.embed_with_flip(sd, imgs).numpy()
        assert np.abs(both - gold["embed_with_flip_f256"]).max() < 1e-6
        assert np.abs(np.linalg.norm(both, axis=1) - 1.0).max() < 1e-6
        fm = inception_ref.forward(sd, imgs[:1], cut_at_pooling=True)
        assert tuple(fm.shape) == (1, 1536, 10, 4)                                       # 144 x 56 -> 73 x 29 -> 37 x 15 -> 19 x 8 -> 10 x 4


def _unpack(f, cin, k):
    """folded fp32 weight rows [Cout][Kpad] (the kernels' reduction order) -> [Cout, Cin, k, k]"""
    cout = f.w.shape[0]
    if cin == 3:
        return f.w[:, :k * k * 4].reshape(cout, k * k, 4)[:, :, :3].permute(0, 2, 1).reshape(cout, 3, k, k)
    return f.w.reshape(cout, cin // 32, k * k, 32).permute(0, 1, 3, 2).reshape(cout, cin, k, k)


@pytest.mark.parametrize("prefix,stride", (("conv1", 1), ("conv2", 1), ("inception4a.branches.3.1", 1), ("inception4b.branches.0.1", 2),
                                           ("inception6b.branches.1.0", 1)))
def test_host_fold_against_float64_conv_and_batchnorm(prefix, stride):
    """conv + eval BatchNorm in float64 == the convolution with the folded fp32 weights plus the folded bias, to the rounding of the
    fp32 weights (2^-24 relative each: the bound is 2^-23 of sum |x| |w'| + |b'|); the split-half rows decode to the fp32 rows within
    2^-22 relative + 2^-25 of the row's scale (hi + lo carry 22 significand bits)."""
    from synth import checkpoint_like_inception_state_dict
    from ssg_amd import resnet
    sd = checkpoint_like_inception_state_dict(7)
    w = sd[prefix + ".0.weight"]
    cout, cin, k, _ = w.shape
    pad = 1 if k == 3 else 0
    f = resnet._fold(sd, prefix + ".0", prefix + ".1", stride, pad, "cpu")
    assert (f.cin, f.cout, f.k, f.stride, f.pad) == (4 if cin == 3 else cin, cout, k, stride, pad) and f.w.shape[1] == (64 if cin == 3 else cin * k * k)
    x = torch.randn(2, cin, 9, 5, generator=torch.Generator().manual_seed(3)).double()
    sd64 = {kk: v.double() for kk, v in sd.items() if kk.startswith(prefix)}
    ref = inception_ref._bn(F.conv2d(x, sd64[prefix + ".0.weight"], None, stride, pad), sd64, prefix + ".1")
    wf = _unpack(f, cin, k).double()
    got = F.conv2d(x, wf, None, stride, pad) + f.bias.double().view(1, -1, 1, 1)
    bound = 2.0 ** -23 * (F.conv2d(x.abs(), wf.abs(), None, stride, pad) + f.bias.double().abs().view(1, -1, 1, 1)) + 1e-300
    assert bool(((got - ref).abs() <= bound).all()), float(((got - ref).abs() / bound).max())
    if cin == 3:
        assert float(f.w[:, 36:].abs().max()) == 0.0 and float(f.w[:, 3:36:4].abs().max()) == 0.0      # the padding channel and the row's tail
    fs = resnet._fold(sd, prefix + ".0", prefix + ".1", stride, pad, "cpu", split=True)
    hl = fs.w.view(torch.float16).reshape(cout, -1, 2, 4 if cin == 3 else 8).float()
    dec = (hl[:, :, 0] + hl[:, :, 1]).reshape(cout, -1)
    scaled = f.w / fs.cscale.view(-1, 1)                       # the fp32 row times its power of two (exact)
    assert bool(((dec - scaled).abs() <= 2.0 ** -22 * scaled.abs() + 2.0 ** -25).all())
    assert bool((scaled.abs().amax(dim=1) <= 16384).all()) and torch.equal(fs.bias, f.bias)


def test_feat_and_feat_bn_fold_into_one_linear():
    from synth import checkpoint_like_inception_state_dict
    sd = checkpoint_like_inception_state_dict(7)
    assert float(sd["feat.bias"].abs().max()) > 0
    m = ssg_amd.create("inception")
    m.load_state_dict(sd, strict=True)
    f = m._fold_feat()
    assert tuple(f.w.shape) == (256, 1536) and tuple(f.bias.shape) == (256,) and not f.split
    x = torch.rand(5, 1536, generator=torch.Generator().manual_seed(4)).double()
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith("feat")}
    ref = inception_ref._bn(F.linear(x, sd64["feat.weight"], sd64["feat.bias"]), sd64, "feat_bn")
    got = F.linear(x, f.w.double(), f.bias.double())
    # fp32 weights and bias, and one fp32 rounding of (running_mean - feat.bias) times the BatchNorm scale
    scale = (sd64["feat_bn.weight"] / torch.sqrt(sd64["feat_bn.running_var"] + 1e-5)).abs()
    bound = 2.0 ** -23 * (F.linear(x.abs(), f.w.double().abs()) + f.bias.double().abs()) + 2.0 ** -24 * scale * (sd64["feat_bn.running_mean"].abs() + sd64["feat.bias"].abs())
    assert bool(((got - ref).abs() <= bound).all()), float(((got - ref).abs() / bound).max())


def test_load_state_dict_leniency():
    from ssg_amd import inception
    m = ssg_amd.create("inception", seed=1)
    other = inception.synthetic_state_dict(seed=9)
    assert not torch.equal(other["conv2.0.weight"], m.state_dict()["conv2.0.weight"])
    missing, unexpected = m.load_state_dict(other, strict=True)
    assert not missing and not unexpected and m._weights == "loaded"
    assert all(torch.equal(m.state_dict()[k], other[k]) for k in other)
    m2 = ssg_amd.create("inception", seed=1)
    m2.load_state_dict({"state_dict": {"module." + k: v for k, v in other.items()}}, strict=True)       # nn.DataParallel checkpoint
    assert all(torch.equal(m2.state_dict()[k], other[k]) for k in other)
    with pytest.raises(RuntimeError, match="size mismatch"):
        m.load_state_dict({"feat.weight": torch.zeros(256, 2048)}, strict=False)
    with pytest.raises(RuntimeError):
        m.load_state_dict(ssg_amd.synthetic_state_dict(seed=1, depth=18), strict=True)                  # a ResNet's keys
    with pytest.warns(UserWarning, match="keep their previous values"):
        m.load_state_dict({"conv1.0.weight": other["conv1.0.weight"]}, strict=False)
    with pytest.raises(ssg_amd.SSGError, match="cuda"):
        m.refresh(other)                                                                                # refresh() is the device route


def test_checkpoint_like_draw_spreads_the_batchnorm_scales():
    from synth import checkpoint_like_inception_state_dict
    sd = checkpoint_like_inception_state_dict(7)
    assert list(sd) == list(ssg_amd.create("inception").state_dict())
    sc = (sd["inception5a.branches.0.1.1.weight"] / torch.sqrt(sd["inception5a.branches.0.1.1.running_var"] + 1e-5)).abs()
    assert float(sc.max() / sc.min()) > 1e3
    out = inception_ref.forward(sd, torch.randn(1, 3, 64, 32, generator=torch.Generator().manual_seed(2)))
    assert bool(torch.isfinite(out).all()) and float(out.max()) > 0                                     # neither explodes nor dies
