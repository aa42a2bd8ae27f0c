"""CPU suite: the BasicBlock embedders (resnet18 / resnet34) on the host side -- factory, state-dict names and shapes, the seeded
draw order of the Bottleneck depths, the restatement tests/basic_ref.py against the golden of the real reference model
(tests/golden/embed_basic_ref.npz, tools/make_golden.py --only-embed-basic) and the cluster=True construction.  No GPU work."""
import os
import warnings

import numpy as np
import pytest

import basic_ref
import ssg_amd
from conftest import GOLDEN
from oracle import embed_oracle

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "embed_basic_ref.npz"))


@pytest.fixture(scope="module")
def imgs():
    return torch.randn(4, 3, 256, 128, generator=torch.Generator().manual_seed(1))       # the golden's images (image_seed = 1)


def _create(name, **kw):
    return ssg_amd.create(name, num_classes=0, pretrained=False, **kw)


@pytest.mark.parametrize("depth", (18, 34))
def test_factory_and_state_dict_names_and_shapes(depth, gold):
    from ssg_amd import resnet
    assert "resnet18" in ssg_amd.names() and "resnet34" in ssg_amd.names()
    assert resnet.names() == ["resnet101", "resnet152", "resnet18", "resnet34", "resnet50"]
    m = _create("resnet%d" % depth, num_split=2)
    assert m.depth == depth and m.out_planes == 512 and _create("resnet50").out_planes == 2048
    sd = ssg_amd.synthetic_state_dict(seed=1, depth=depth)
    mine = ["%s %s" % (k, "x".join(str(d) for d in v.shape)) for k, v in sd.items()]
    assert mine == [str(s) for s in gold["keys_r%d" % depth]]             # the reference model's own state_dict(), in its order
    assert tuple(sd["base.fc.weight"].shape) == (1000, 512) and tuple(sd["feat.weight"].shape) == (2048, 512)
    assert "base.layer1.0.downsample.0.weight" not in sd and "base.layer1.0.conv3.weight" not in sd
    assert tuple(sd["base.layer2.0.downsample.0.weight"].shape) == (128, 64, 1, 1) and tuple(sd["base.layer2.0.conv1.weight"].shape) == (128, 64, 3, 3)
    assert list(m.state_dict()) == list(sd) and all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    assert tuple(ssg_amd.synthetic_state_dict(seed=1, depth=depth, num_features=256)["feat.weight"].shape) == (256, 512)
    with pytest.raises(KeyError):
        ssg_amd.create("resnet20")


def test_depth50_seeded_tensors_are_unchanged():
    """the draw order of the Bottleneck depths is what tests/golden/embed_ref.npz was made from: the existing restatement on the
    seed-1 weights still reproduces the reference model's recorded features (one image, S = 2; the bound of make_golden.py)"""
    ref = np.load(os.path.join(GOLDEN, "embed_ref.npz"))["feats_S2"]
    sd = ssg_amd.synthetic_state_dict(seed=1)
    x = torch.randn(4, 3, 256, 128, generator=torch.Generator().manual_seed(1))[:1]
    mine = torch.stack(embed_oracle.embed_with_flip(sd, x, 2)).numpy()
    assert np.abs(mine - ref[:, :1]).max() < 1e-6
    assert tuple(sd["base.fc.weight"].shape) == (1000, 2048) and tuple(sd["feat.weight"].shape) == (2048, 2048)
    assert tuple(sd["base.layer1.0.conv1.weight"].shape) == (64, 64, 1, 1) and "base.layer1.0.downsample.0.weight" in sd


@pytest.mark.parametrize("depth,S", ((18, 2), (18, 1), (34, 2)))
def test_restatement_matches_the_reference_golden(depth, S, gold, imgs):
    sd = ssg_amd.synthetic_state_dict(seed=1, depth=depth)
    mine = torch.stack(basic_ref.embed_with_flip(sd, imgs, depth, S)).numpy()
    ref = gold["feats_r%d_S%d" % (depth, S)]
    assert mine.shape == ref.shape == ((S + 1) if S > 1 else 1, 4, 512)
    assert np.abs(mine - ref).max() < 1e-6
    if (depth, S) == (18, 2):
        x1, x2 = basic_ref.forward(sd, imgs, 18, 2, for_eval=True)
        assert tuple(x1.shape) == (4, 3 * 512) and tuple(x2.shape) == (4, 2048)
        assert np.abs(x1.numpy() - gold["x1_r18_S2_eval"]).max() < 1e-6 and np.abs(x2.numpy() - gold["x2_r18_S2_eval"]).max() < 1e-6


def test_basic_block_restatement_is_base_py():
    """basic_block from raw BatchNorm tuples == the same block from folded weights and biases (what the kernel tests hand it)"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 8, 6, 5, generator=g).double()
    w1, w2 = torch.randn(8, 8, 3, 3, generator=g).double(), torch.randn(8, 8, 3, 3, generator=g).double()
    bns = [(torch.rand(8, generator=g).double() + 0.5, torch.randn(8, generator=g).double(), torch.randn(8, generator=g).double(),
            torch.rand(8, generator=g).double() + 0.5) for _ in range(2)]
    a = basic_ref.basic_block(x, (w1, w2), bns)
    folded = []
    for w, (ga, be, mu, var) in zip((w1, w2), bns):
        sc = ga / torch.sqrt(var + 1e-5)
        folded.append((w * sc.view(-1, 1, 1, 1), be - mu * sc))
    b = basic_ref.basic_block(x, (folded[0][0], folded[1][0]), (folded[0][1], folded[1][1]))
    assert float((a - b).abs().max()) < 1e-12 and float(a.min()) == 0.0


@pytest.mark.parametrize("depth", (18, 34))
def test_state_dict_round_trip(depth):
    m = _create("resnet%d" % depth, num_split=2, seed=1)
    other = ssg_amd.synthetic_state_dict(seed=9, depth=depth)
    assert not torch.equal(other["base.layer3.0.downsample.0.weight"], m.state_dict()["base.layer3.0.downsample.0.weight"])
    missing, unexpected = m.load_state_dict(other, strict=True)
    assert not missing and not unexpected and m._weights == "loaded"
    assert all(torch.equal(m.state_dict()[k], other[k]) for k in other)
    m2 = _create("resnet%d" % depth, num_split=2, seed=1)
    m2.load_state_dict({"state_dict": {"module." + k: v for k, v in other.items()}}, strict=True)       # nn.DataParallel checkpoint
    assert all(torch.equal(m2.state_dict()[k], other[k]) for k in other)
    with pytest.raises(RuntimeError, match="size mismatch"):
        m.load_state_dict({"feat.weight": torch.zeros(2048, 2048)}, strict=False)                     # a ResNet-50 head does not fit
    with pytest.raises(RuntimeError):
        m.load_state_dict(ssg_amd.synthetic_state_dict(seed=1, depth=50), strict=True)


def test_cluster_head_constructs_on_a_512_wide_backbone():
    """resnet.py:76-77: the DEC centres stay [32, 2048] whatever the backbone; the mismatch only shows in the forward
    (resnet.py:129-131), where a ValueError names the two widths -- raised before any GPU work"""
    from ssg_amd import resnet
    m = _create("resnet18", num_split=1, cluster=True)
    assert tuple(m.state_dict()[resnet._DEC_KEY].shape) == (32, 2048) and m.out_planes == 512
    sd0 = ssg_amd.synthetic_state_dict(seed=1, depth=18)
    assert all(torch.equal(m.state_dict()[k], sd0[k]) for k in sd0)       # drawn last: every other tensor is the cluster=False one
    with pytest.raises(ValueError, match="512.*2048.*resnet.py:129"):
        m(torch.zeros(1, 3, 64, 32))
    m2 = _create("resnet34", num_split=2, cluster=True)
    with pytest.raises(ValueError, match="1536.*2048.*resnet.py:129"):
        m2(torch.zeros(1, 3, 64, 32))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = m._f32_twin()
    assert t.out_planes == 512 and t.depth == 18 and t.precision == "f32"
