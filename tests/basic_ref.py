"""Plain PyTorch CPU restatement of the BasicBlock networks (ResNet-18 / ResNet-34), fp32 or fp64 (TEST INFRASTRUCTURE ONLY).

oracle/embed_oracle.py restates the Bottleneck ResNet-50; this module adds, in the same manner,
  reid/models/base.py:25-54,96-152   BasicBlock ResNet (conv / eval BatchNorm / ReLU / maxpool; downsample 1x1 stride s in the
                                     first blocks of layer2-4 only)
and reuses embed_oracle.pooled / heads / sum_norm / fliplr for everything behind layer4 (resnet.py:93-124, evaluators.py:12-35),
which does not depend on the backbone.  It is pinned against the real reference model by tools/make_golden.py
(embed_fixture_basic) -> tests/golden/embed_basic_ref.npz.
"""
import torch
import torch.nn.functional as F

from oracle import embed_oracle
from oracle.embed_oracle import _bn, _bn_t, fliplr, heads, sum_norm

LAYERS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}


def basic_block(x, convs, bns, stride=1, downsample=None):
    """one BasicBlock (base.py:38-54): convs = (w1 3x3 stride s, w2 3x3), bns = their BatchNorm 4-tuples (or folded biases, see
    embed_oracle._bn_t), downsample = (w 1x1 stride s, bn) or None (identity shortcut); NCHW, in the dtype of x."""
    out = F.relu(_bn_t(F.conv2d(x, convs[0].to(x.dtype), None, stride, 1), bns[0]))
    out = _bn_t(F.conv2d(out, convs[1].to(x.dtype), None, 1, 1), bns[1])
    res = x if downsample is None else _bn_t(F.conv2d(x, downsample[0].to(x.dtype), None, stride), downsample[1])
    return F.relu(out + res)


def _bn4(sd, name):
    return (sd[name + ".weight"], sd[name + ".bias"], sd[name + ".running_mean"], sd[name + ".running_var"])


def feature_map(sd, x, depth, dtype=None):
    """x [B,3,H,W] -> layer4 output [B,512,H/32,W/32] (resnet.py:87-92); dtype: cast x and the weights first."""
    if dtype is not None:
        sd = {k: v.to(dtype) for k, v in sd.items() if v.dtype.is_floating_point}
        x = x.to(dtype)
    x = F.relu(_bn(F.conv2d(x, sd["base.conv1.weight"], None, 2, 3), sd, "base.bn1"))
    x = F.max_pool2d(x, 3, 2, 1)
    for li, n in enumerate(LAYERS[depth]):
        for b in range(n):
            p = "base.layer%d.%d" % (li + 1, b)
            stride = 2 if (b == 0 and li > 0) else 1
            ds = None
            if (p + ".downsample.0.weight") in sd:
                ds = (sd[p + ".downsample.0.weight"], _bn4(sd, p + ".downsample.1"))
            x = basic_block(x, (sd[p + ".conv1.weight"], sd[p + ".conv2.weight"]), (_bn4(sd, p + ".bn1"), _bn4(sd, p + ".bn2")), stride, ds)
    return x


def forward(sd, x, depth, num_split, for_eval=False, dtype=torch.float32):
    """resnet.py:86-124: model(x, for_eval) -> (x1, x2), computed and returned in `dtype`."""
    sd = {k: v.to(dtype) for k, v in sd.items() if v.dtype.is_floating_point}
    with torch.no_grad():
        return heads(sd, feature_map(sd, x.to(dtype), depth), num_split, for_eval)


def embed_with_flip(sd, imgs, depth, num_split, dtype=torch.float32, for_eval=False):
    """evaluators.py:28-35 as embed_oracle.embed_with_flip states it, over the BasicBlock backbone: a list of S+1 [B,512]
    (per-set norm), or [B,(S+1)*512] under one norm when for_eval and num_split > 1."""
    a = forward(sd, imgs, depth, num_split, for_eval, dtype)[0]
    b = forward(sd, fliplr(imgs), depth, num_split, for_eval, dtype)[0]
    if isinstance(a, list):
        return [sum_norm(x, y) for x, y in zip(a, b)]
    return sum_norm(a, b) if (for_eval and num_split > 1) else [sum_norm(a, b)]


assert embed_oracle.pooled is not None      # (the pooling is embed_oracle's: heads() calls it)
