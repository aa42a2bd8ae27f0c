"""Plain PyTorch CPU restatement of the embedding path, fp32 or fp64 (TEST INFRASTRUCTURE ONLY).

Floating-point kernels keep a torch fp32 reference (the task's rule for fp kernels); this
restates, with torch.nn.functional on the CPU:
  reid/models/base.py:57-93,96-152   Bottleneck ResNet-50 (conv / eval BatchNorm / ReLU / maxpool)
  reid/models/resnet.py:86-111       stop before avgpool; global + stripe average pooling
  reid/models/resnet.py:112-124      x2 = relu(feat_bn(feat(x1[0]))); for_eval: the sets concatenated
  reid/evaluators.py:12-16,28-35     fliplr, sum of both orientations, L2 normalisation (per set, or of the concatenation)
from a state_dict with the reference's key names.  It is pinned against the real reference
model (run with stub torchvision/h5py/metric_learn modules) by tools/make_golden.py ->
tests/golden/embed_ref.npz.

`dtype=torch.float64` runs the same statements in double precision: the reference the kernel tests measure BOTH the HIP path
and the fp32 restatement against.  `stem` / `bottleneck` restate one fused launch each (csrc/stem_pool.hip,
csrc/bottleneck.hip) from the raw convolution weights and BatchNorm tensors, NCHW, in the dtype of their input.
"""
import torch
import torch.nn.functional as F

_LAYERS = (3, 4, 6, 3)


def _bn(x, sd, name):
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"], False, 0.0, 1e-5)


def _bn_t(x, bn):
    """eval BatchNorm from (weight, bias, running_mean, running_var); a single 1-D tensor instead is the bias of a convolution
    whose weights already carry the folded BatchNorm scale (what the kernels are given)"""
    if torch.is_tensor(bn):
        return x + bn.to(x.dtype).view(1, -1, 1, 1)
    g, b, m, v = (t.to(x.dtype) for t in bn)
    return F.batch_norm(x, m, v, g, b, False, 0.0, 1e-5)


def stem(x, w, bn, flip=False):
    """x [B,3,H,W] -> conv 7x7 s2 p3 -> eval BN -> ReLU -> maxpool 3x3 s2 p1 (base.py:101-105), of fliplr(x) when flip."""
    if flip:
        x = fliplr(x)
    return F.max_pool2d(F.relu(_bn_t(F.conv2d(x, w.to(x.dtype), None, 2, 3), bn)), 3, 2, 1)


def bottleneck(x, convs, bns, downsample=None):
    """the stride-1 Bottleneck (base.py:57-90): convs = (w1 1x1, w2 3x3, w3 1x1), bns = their BatchNorm 4-tuples,
    (or folded biases, see _bn_t), downsample = (w 1x1, bn) or None (identity shortcut)."""
    out = F.relu(_bn_t(F.conv2d(x, convs[0].to(x.dtype)), bns[0]))
    out = F.relu(_bn_t(F.conv2d(out, convs[1].to(x.dtype), None, 1, 1), bns[1]))
    out = _bn_t(F.conv2d(out, convs[2].to(x.dtype)), bns[2])
    res = x if downsample is None else _bn_t(F.conv2d(x, downsample[0].to(x.dtype)), downsample[1])
    return F.relu(out + res)


def feature_map(sd, x, dtype=None):
    """x [B,3,H,W] -> layer4 output [B,2048,H/32,W/32] (resnet.py:87-92); dtype: cast x and the weights first."""
    if dtype is not None:
        sd = {k: v.to(dtype) for k, v in sd.items() if v.dtype.is_floating_point}
        x = x.to(dtype)
    x = F.relu(_bn(F.conv2d(x, sd["base.conv1.weight"], None, 2, 3), sd, "base.bn1"))
    x = F.max_pool2d(x, 3, 2, 1)
    for li, n in enumerate(_LAYERS):
        for b in range(n):
            p = "base.layer%d.%d" % (li + 1, b)
            stride = 2 if (b == 0 and li > 0) else 1
            out = F.relu(_bn(F.conv2d(x, sd[p + ".conv1.weight"]), sd, p + ".bn1"))
            out = F.relu(_bn(F.conv2d(out, sd[p + ".conv2.weight"], None, stride, 1), sd, p + ".bn2"))
            out = _bn(F.conv2d(out, sd[p + ".conv3.weight"]), sd, p + ".bn3")
            res = x
            if (p + ".downsample.0.weight") in sd:
                res = _bn(F.conv2d(x, sd[p + ".downsample.0.weight"], None, stride), sd, p + ".downsample.1")
            x = F.relu(out + res)
    return x


def pooled(fmap, num_split):
    """resnet.py:93-111 -> list of S+1 [B,2048] (or a single tensor when num_split <= 1)."""
    if num_split > 1:
        h = fmap.size(2)
        x1 = [F.avg_pool2d(fmap, fmap.size()[2:]).view(fmap.size(0), -1)]
        for s in range(num_split):
            xx = fmap[:, :, h // num_split * s: h // num_split * (s + 1), :]
            x1.append(F.avg_pool2d(xx, xx.size()[2:]).view(xx.size(0), -1))
        return x1
    return F.avg_pool2d(fmap, fmap.size()[2:]).view(fmap.size(0), -1)


def fliplr(img):
    return img.index_select(3, torch.arange(img.size(3) - 1, -1, -1).long())


def heads(sd, fmap, num_split, for_eval=False):
    """resnet.py:93-124 from the layer4 map on (num_classes = 0, eval mode), in the dtype of fmap and sd: -> (x1, x2).
    x1 = the un-normalised pooled sets (a list of S+1 [B,2048], their concatenation [B,(S+1)*2048] when for_eval, a single
    [B,2048] when num_split <= 1); x2 = relu(feat_bn(feat(global average)))."""
    x1 = pooled(fmap, num_split)
    x2 = None
    if "feat.weight" in sd:          # num_features > 0
        x2 = F.relu(_bn(F.linear(x1[0] if num_split > 1 else x1, sd["feat.weight"]), sd, "feat_bn"))
    if num_split > 1 and for_eval:
        x1 = torch.cat(x1, dim=1)
    return x1, x2


def forward(sd, x, num_split, for_eval=False, dtype=torch.float32):
    """resnet.py:86-124: model(x, for_eval) -> (x1, x2), computed and returned in `dtype`."""
    sd = {k: v.to(dtype) for k, v in sd.items() if v.dtype.is_floating_point}
    with torch.no_grad():
        return heads(sd, feature_map(sd, x.to(dtype)), num_split, for_eval)


def sum_norm(a, b):
    """evaluators.py:31-35 / 41-43 on one feature set: (a + b) / ||a + b|| per row."""
    s = a + b
    return s / torch.norm(s, p=2, dim=1, keepdim=True)


def embed_with_flip(sd, imgs, num_split, dtype=torch.float32, for_eval=False):
    """evaluators.py:28-35: per set (a + b) / ||a + b||, computed and returned in `dtype` (a list of S+1 [B,2048]);
    for_eval (evaluators.py:40-43): the model hands over the concatenated sets, so ONE norm over all (S+1)*2048 columns
    -> [B,(S+1)*2048] (a single set, num_split <= 1, comes back as a list of one either way)."""
    a = forward(sd, imgs, num_split, for_eval, dtype)[0]
    b = forward(sd, fliplr(imgs), num_split, for_eval, dtype)[0]
    if isinstance(a, list):
        return [sum_norm(x, y) for x, y in zip(a, b)]
    return sum_norm(a, b) if (for_eval and num_split > 1) else [sum_norm(a, b)]
