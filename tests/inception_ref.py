"""Plain PyTorch CPU restatement of the InceptionNet embedder, fp32 or fp64 (TEST INFRASTRUCTURE ONLY).

In the manner of tests/basic_ref.py, from a state dict with the reference's key names:
  reid/models/inception.py:12-47    conv + eval BatchNorm + ReLU units; a block = its branches concatenated along the channels
                                    ('Avg': 1x1-3x3 | 1x1-3x3-3x3 | 1x1 | avgpool(3,1,1)-1x1; 'Max': 1x1-3x3(s) | 1x1-3x3-3x3(s) | maxpool(3,s,1))
  reid/models/inception.py:90-119   three 3x3 stem units, MaxPool2d(2,2,1), six blocks, global average pool, feat + feat_bn,
                                    F.normalize when norm, else ReLU when there is an embedding
  reid/evaluators.py:12-16,41-43    fliplr, sum of both orientations, one L2 norm
It is pinned against the real reference model by tools/make_golden.py (embed_fixture_inception) ->
tests/golden/embed_inception_ref.npz.  `pool_ref` / `encode_h8l8` / `decode_h8l8` restate the pool kernels of csrc/inception.hip and
the split-half container format for the unit tests.
"""
import torch
import torch.nn.functional as F

from oracle.embed_oracle import _bn, fliplr, sum_norm

BLOCKS = (("inception4a", "Avg", 1), ("inception4b", "Max", 2), ("inception5a", "Avg", 1), ("inception5b", "Max", 2),
          ("inception6a", "Avg", 1), ("inception6b", "Max", 2))


def unit(sd, x, p, stride=1):
    """_make_conv (inception.py:12-18): conv (3x3 pad 1, or 1x1 pad 0, no bias) -> eval BatchNorm -> ReLU; p = the Sequential's key prefix"""
    w = sd[p + ".0.weight"]
    return F.relu(_bn(F.conv2d(x, w, None, stride, 1 if w.shape[-1] == 3 else 0), sd, p + ".1"))


def block(sd, x, name, pool, stride):
    p = name + ".branches."
    outs = [unit(sd, unit(sd, x, p + "0.0"), p + "0.1", stride),
            unit(sd, unit(sd, unit(sd, x, p + "1.0"), p + "1.1"), p + "1.2", stride)]
    if pool == "Avg":
        outs.append(unit(sd, x, p + "2"))
        outs.append(unit(sd, F.avg_pool2d(x, 3, 1, 1), p + "3.1"))
    else:
        outs.append(F.max_pool2d(x, 3, stride, 1))
    return torch.cat(outs, 1)


def _cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items() if v.dtype.is_floating_point}


def feature_map(sd, x, dtype=None):
    """x [B,3,H,W] -> block-6b map [B,1536,h,w] (inception.py:91-100); dtype: cast x and the weights first"""
    if dtype is not None:
        sd, x = _cast(sd, dtype), x.to(dtype)
    for p in ("conv1", "conv2", "conv3"):
        x = unit(sd, x, p)
    x = F.max_pool2d(x, 2, 2, 1)
    for name, pool, stride in BLOCKS:
        x = block(sd, x, name, pool, stride)
    return x


def head(sd, fmap, norm=False):
    """inception.py:105-114 (eval mode, num_classes = 0) in the dtype of fmap and sd"""
    x = F.adaptive_avg_pool2d(fmap, 1).view(fmap.size(0), -1)
    emb = "feat.weight" in sd
    if emb:
        x = _bn(F.linear(x, sd["feat.weight"], sd["feat.bias"]), sd, "feat_bn")
    if norm:
        return F.normalize(x)
    return F.relu(x) if emb else x


def forward(sd, x, norm=False, cut_at_pooling=False, dtype=torch.float32):
    """model(x), computed and returned in `dtype`.  A state dict without `feat.*` is the num_features = 0 model."""
    sd = _cast(sd, dtype)
    with torch.no_grad():
        fm = feature_map(sd, x.to(dtype))
        return fm if cut_at_pooling else head(sd, fm, norm)


def embed_with_flip(sd, imgs, norm=False, dtype=torch.float32):
    """evaluators.py:41-43 on model(x): (model(x) + model(fliplr(x))) / its L2 norm -> [B, D]"""
    return sum_norm(forward(sd, imgs, norm, False, dtype), forward(sd, fliplr(imgs), norm, False, dtype))


def key_listing(sd):
    """'name d0xd1x...' per entry, in order: the form tests/golden/embed_inception_ref.npz records the reference's state dict in"""
    return ["%s %s" % (k, "x".join(str(d) for d in v.shape)) for k, v in sd.items()]


# ---- the split-half container format and the pool kernels of csrc/inception.hip, restated for the unit tests
def encode_h8l8(v):
    """float32 [..., C] (C % 8 == 0) -> float32 containers [..., C]: per 8 channels [8 x half hi][8 x half lo]"""
    shp = v.shape
    v = v.reshape(-1, shp[-1] // 8, 8)
    hi = v.half()
    lo = (v - hi.float()).half()
    return torch.stack([hi, lo], dim=2).reshape(-1, 2 * shp[-1]).contiguous().view(torch.float32).reshape(shp)


def decode_h8l8(c):
    shp = c.shape
    h = c.contiguous().view(torch.float16).reshape(-1, shp[-1] // 8, 2, 8).float()
    return (h[:, :, 0] + h[:, :, 1]).reshape(shp)


def pool_ref(x, kind, k=3, stride=1, pad=1):
    """x [B,H,W,C] float32 NHWC -> the pool as csrc/inception.hip computes it, float32 NHWC.  'max': F.max_pool2d (exact).  'avg':
    AvgPool2d(3,1,1) with count_include_pad as the fixed float32 sum of the nine taps in row-major order (rows outer) from +0, taps in
    the padding adding +0, then one float32 division by 9."""
    n = x.permute(0, 3, 1, 2).contiguous()
    if kind == "max":
        return F.max_pool2d(n, k, stride, pad).permute(0, 2, 3, 1).contiguous()
    B, C, H, W = n.shape
    p = F.pad(n, (1, 1, 1, 1))
    acc = torch.zeros_like(n)
    for r in range(3):
        for s in range(3):
            acc = acc + p[:, :, r:r + H, s:s + W]
    return (acc / torch.tensor(9.0, dtype=torch.float32)).permute(0, 2, 3, 1).contiguous()
