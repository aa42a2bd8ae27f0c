"""InceptionNet embedder -- host-side mirror of reid/models/inception.py:50-143, forward only, in the manner of `resnet.ResNet`.

`create('inception', num_features=256, norm=False)` returns an object with the reference's call surface: `state_dict()` /
`load_state_dict()` with the reference's 241 keys in its order (`conv1.0.weight`, `conv1.1.running_mean`, ...,
`inception4a.branches.0.0.0.weight`, ..., `feat.weight`, `feat.bias`, `feat_bn.*`), `eval()`, `cuda()` and `model(x)` ->
[B, num_features] (inception.py:90-119): relu(feat_bn(feat(gap))) or, with norm=True, its F.normalize; num_features=0 gives the pooled
[B, 1536] map (normalised when norm); cut_at_pooling=True gives the NCHW block-6b map [B, 1536, h, w].  The reference's drivers feed it
144 x 56 images (selftraining.py:105); the maps are then 73 x 29 -> 37 x 15 -> 19 x 8 -> 10 x 4.

The forward runs on HIP kernels (csrc/inception.hip, csrc/conv.hip) through the C ABI: NHWC, eval-mode BatchNorm folded into the convolution
weights at load time (the host fold `resnet._fold`, or csrc/fold.hip when the weights are on the device: same bits), bias + ReLU in the
GEMM epilogue, every branch of a block written straight into its channel slice of the block's output (no concatenation pass), the
pools MaxPool2d(2,2,1), AvgPool2d(3,1,1) and MaxPool2d(3,2,1) as their own launches.

precision='split' (default, or SSG_EMBED_PRECISION): every convolution, the stem's three 32-channel layers included, takes split-half
(h8l8; the image h4l4) operands and runs on the fp16 matrix cores with fp32 accumulation; the pools work on the split-half maps.  The
layers behind the global average pool -- `feat` + `feat_bn` as ONE folded Linear (ssg_linear_fwd_f32, K = 1536), ReLU / L2 norm --
run in fp32 in both modes.  precision='f32' keeps every convolution on the fp32 matrix cores.  The split-half range flag and the
automatic fp32 recompute behave as on ResNet.

Batch limit: no tensor may leave the 2 GiB range of the kernels' checks (ValueError, as on the ResNet path).  At 144 x 56 the largest
tensor is block 4a's output, 73 * 29 * 256 * 4 bytes per image: B <= 990.

There is no training path (num_classes > 0 raises) and no fused block: one launch per layer.  The 32-channel layers and every layer
that writes a channel slice run on csrc/inception.hip; the dense inner 1x1 / 3x3 layers of a branch (Cout % 64 == 0) are in the ResNet
regime and run on csrc/conv.hip (`model.dense_conv`, SSG_INC_DENSE_CONV=0: those on csrc/inception.hip too; measured slower,
profiles/inception_times.txt).
"""
from collections import OrderedDict

import ctypes
import os

import torch

from . import _lib
from ._lib import check, ptr, stream
from . import resnet as _rn
from .resnet import ResNet, _bn_keys, _use_device_fold, _fold, _fold_device

_IN_SPLIT, _OUT_SPLIT = 1, 2
_STEM = (("conv1", 3, 32), ("conv2", 32, 32), ("conv3", 32, 32))
_BLOCKS = (("inception4a", 64, "Avg", 1), ("inception4b", 64, "Max", 2), ("inception5a", 128, "Avg", 1),
           ("inception5b", 128, "Max", 2), ("inception6a", 256, "Avg", 1), ("inception6b", 256, "Max", 2))


def _arch():
    """-> (stem, blocks, width): stem = [(prefix, cin, cout)]; blocks = [dict(name, cin, planes, pool, stride, cout, convs)] with
    convs = {tag: (prefix, cin, cout, k, stride)} in the reference's module order (inception.py:21-47): b0a 1x1, b0b 3x3 stride s;
    b1a 1x1, b1b 3x3, b1c 3x3 stride s; 'Avg' blocks add b2 1x1 and b3 (AvgPool2d(3,1,1) then 1x1), 'Max' blocks MaxPool2d(3,s,1)."""
    blocks, cin = [], 32
    for name, pl, pool, s in _BLOCKS:
        p = name + ".branches."
        convs = OrderedDict()
        convs["b0a"] = (p + "0.0", cin, pl, 1, 1); convs["b0b"] = (p + "0.1", pl, pl, 3, s)
        convs["b1a"] = (p + "1.0", cin, pl, 1, 1); convs["b1b"] = (p + "1.1", pl, pl, 3, 1); convs["b1c"] = (p + "1.2", pl, pl, 3, s)
        if pool == "Avg":
            convs["b2"] = (p + "2", cin, pl, 1, 1); convs["b3"] = (p + "3.1", cin, pl, 1, 1)
        cout = pl * 4 if pool == "Avg" else pl * 2 + cin
        blocks.append(dict(name=name, cin=cin, planes=pl, pool=pool, stride=s, cout=cout, convs=convs))
        cin = cout
    return list(_STEM), blocks, cin


WIDTH = _arch()[2]      # 1536


def synthetic_state_dict(seed=1, num_features=256, cut_at_pooling=False):
    """Deterministic weights with the reference's keys, order and shapes, drawn as inception.py:127-139 reset_params draws them:
    Kaiming-normal fan_out convolutions, identity BatchNorm, `feat` with std 0.001 and zero bias."""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()

    def conv_bn(p, cin, cout, k):
        sd[p + ".0.weight"] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cout * k * k)) ** 0.5
        bn(p + ".1", cout)

    def bn(p, c):
        sd[p + ".weight"] = torch.ones(c); sd[p + ".bias"] = torch.zeros(c)
        sd[p + ".running_mean"] = torch.zeros(c); sd[p + ".running_var"] = torch.ones(c)
        sd[p + ".num_batches_tracked"] = torch.zeros((), dtype=torch.long)

    stem, blocks, width = _arch()
    for p, cin, cout in stem:
        conv_bn(p, cin, cout, 3)
    for blk in blocks:
        for p, cin, cout, k, _ in blk["convs"].values():
            conv_bn(p, cin, cout, k)
    if not cut_at_pooling and num_features > 0:
        sd["feat.weight"] = torch.randn(num_features, width, generator=g) * 0.001
        sd["feat.bias"] = torch.zeros(num_features)
        bn("feat_bn", num_features)
    return sd


class InceptionNet(ResNet):
    """Mirror of reid.models.inception.InceptionNet (inception.py:50-143), forward only.  The state-dict, device and refresh surface
    is `resnet.ResNet`'s."""

    def __init__(self, cut_at_pooling=False, num_features=256, norm=False, dropout=0, num_classes=0, checkpoint=None, seed=1, precision=None):
        if num_classes > 0:
            raise NotImplementedError("num_classes > 0 (dropout + classifier head, inception.py:115-118) is a training-only path; "
                                      "the grouping path uses num_classes=0 (selftraining.py:121-123)")
        if num_features < 0:
            raise ValueError("num_features must be >= 0")
        self.cut_at_pooling, self.norm, self.dropout, self.num_classes = bool(cut_at_pooling), bool(norm), dropout, num_classes
        self.has_embedding = (not self.cut_at_pooling) and num_features > 0
        self.num_features = num_features if self.has_embedding else WIDTH        # inception.py:82
        self.out_planes = self.num_features       # width of the one feature set the extraction harness gets (evaluators.extract_embeddings)
        self.num_split, self.cluster, self.training = 1, False, False
        self.precision = precision or os.environ.get("SSG_EMBED_PRECISION", "split")
        if self.precision not in ("split", "f32"):
            raise ValueError("precision must be 'split' or 'f32'")
        self.device = torch.device("cpu")
        self._sd = synthetic_state_dict(seed, num_features, self.cut_at_pooling)
        self._folded = None
        self._twin = None
        self.flip_streams = True
        # SSG_INC_DENSE_CONV=0: every convolution on csrc/inception.hip (default: the dense inner layers of a branch on csrc/conv.hip)
        self.dense_conv = os.environ.get("SSG_INC_DENSE_CONV", "1") != "0"
        self._weights = "synthetic"
        if checkpoint:
            self.load_state_dict(torch.load(checkpoint, map_location="cpu"), strict=False)

    def _report_missing(self, who, missing):
        miss = [k for k in missing if not k.endswith("num_batches_tracked")]
        if miss:
            import warnings
            warnings.warn("ssg_amd InceptionNet.%s: %d tensors were not in the state dict and keep their previous values (first: %s)"
                          % (who, len(miss), miss[0]), stacklevel=3)
        else:
            self._weights = "loaded"

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("ssg_amd.inception.InceptionNet is an inference-only embedder")
        return self.eval()

    # ---- weights
    def _fold_feat(self):
        """feat + feat_bn as one Linear (w [N, 1536], bias [N]) in fp32.  The Linear's own bias b goes into the BatchNorm mean first
        (bn(Wx + b) = bn'(Wx) with mean' = mean - b, one float32 subtraction), then the convolution fold runs as for a 1x1 layer."""
        keys = _bn_keys("feat", "feat_bn")
        if _use_device_fold(self._sd, keys + ("feat.bias",)):
            src = [self._sd[k].detach().to(self.device, torch.float32) for k in keys]
            src[0] = src[0].unsqueeze(-1).unsqueeze(-1)
            src[3] = src[3] - self._sd["feat.bias"].detach().to(self.device, torch.float32)
            return _fold_device([src], 1, 0, self.device)
        sd = self._host_sd(keys + ("feat.bias",))
        return _fold({"c.weight": sd["feat.weight"].view(self.num_features, WIDTH, 1, 1), "b.weight": sd["feat_bn.weight"], "b.bias": sd["feat_bn.bias"],
                      "b.running_mean": sd["feat_bn.running_mean"].float() - sd["feat.bias"].float(), "b.running_var": sd["feat_bn.running_var"]},
                     "c", "b", 1, 0, self.device)

    def _prepare(self):
        if self._folded is not None:
            return self._folded
        if self.device.type != "cuda":
            raise _lib.SSGError("the embedder runs on the GPU only: call model.cuda() first (no CPU fallback)")
        sp = self.precision == "split"
        stem, blocks, _ = _arch()
        net = dict(split=sp, stem=[self._fold_one(p + ".0", p + ".1", 1, 1, sp) for p, _, _ in stem], blocks=[])
        for blk in blocks:
            net["blocks"].append({tag: self._fold_one(p + ".0", p + ".1", s, 1 if k == 3 else 0, sp) for tag, (p, _, _, k, s) in blk["convs"].items()})
        if self.has_embedding:
            net["feat"] = self._fold_feat()
        self._folded = net
        return net

    # ---- forward
    @staticmethod
    def _slice(out, coff):
        return ctypes.c_void_p(out.data_ptr() + 4 * coff)

    def _conv(self, L, x, f, sp, ovf, out=None, coff=0):
        """x -> relu(conv + folded BatchNorm), dense, or into the channels [coff, coff + f.cout) of `out`"""
        B, H, W, _ = x.shape
        OH = (H + 2 * f.pad - f.k) // f.stride + 1; OW = (W + 2 * f.pad - f.k) // f.stride + 1
        if out is None:
            if self.dense_conv and f.cin != 4 and f.cout % 64 == 0:
                # a dense [M, Cout] output in the ResNet regime (a branch's inner 1x1 / 3x3): the LDS-staged kernels of csrc/conv.hip
                return ResNet._conv(L, x, f, out_split=sp, ovf=ovf, tiled=True)
            out = torch.empty((B, OH, OW, f.cout), dtype=torch.float32, device=x.device)
        flags = (_IN_SPLIT | _OUT_SPLIT) if sp else 0
        check(L.ssg_inc_conv2d_nhwc_x(ptr(x), ptr(f.w), ptr(f.bias), self._slice(out, coff), B, H, W, f.cin, f.cout, f.k, f.stride, f.pad, 1, flags,
                                      ptr(f.cscale), out.shape[3], ptr(ovf), stream()), "ssg_inc_conv2d_nhwc_x")
        return out

    def _maxpool(self, L, x, k, stride, pad, sp, out=None, coff=0):
        B, H, W, C = x.shape
        OH = (H + 2 * pad - k) // stride + 1; OW = (W + 2 * pad - k) // stride + 1
        if out is None:
            out = torch.empty((B, OH, OW, C), dtype=torch.float32, device=x.device)
        check(L.ssg_inc_maxpool_nhwc_x(ptr(x), self._slice(out, coff), B, H, W, C, k, stride, pad, 1 if sp else 0, out.shape[3], stream()),
              "ssg_inc_maxpool_nhwc_x")
        return out

    def _fmap(self, x, flip=False, hooks=None):
        """-> (block-6b map [B,h,w,1536], is_split): with precision='split' the float32 tensor is a container of h8l8 split halves"""
        L = _lib.lib()
        net = self._prepare()
        sp = net["split"]
        x = x.to(self.device, torch.float32).contiguous()
        B, C, H, W = x.shape
        if C != 3:
            raise ValueError("expected RGB images [B,3,H,W]")
        ovf = self._overflow_flag() if sp else None
        y = torch.empty((B, H, W, 4), dtype=torch.float32, device=self.device)
        if sp:
            check(L.ssg_nchw_to_nhwc4_h4l4(ptr(x), ptr(y), B, H, W, 1 if flip else 0, stream()), "ssg_nchw_to_nhwc4_h4l4")
        else:
            check(L.ssg_nchw_to_nhwc4(ptr(x), ptr(y), B, H, W, 1 if flip else 0, stream()), "ssg_nchw_to_nhwc4")
        for f in net["stem"]:                                       # inception.py:91-93
            y = self._conv(L, y, f, sp, ovf)
        y = self._maxpool(L, y, 2, 2, 1, sp)                        # pool3
        for blk, cv in zip(_arch()[1], net["blocks"]):             # inception.py:46-47: torch.cat of the branches, written in place
            pl, s = blk["planes"], blk["stride"]
            _, H2, W2, _ = y.shape
            OH, OW = (H2 + 2 - 3) // s + 1, (W2 + 2 - 3) // s + 1
            out = torch.empty((B, OH, OW, blk["cout"]), dtype=torch.float32, device=self.device)
            self._conv(L, self._conv(L, y, cv["b0a"], sp, ovf), cv["b0b"], sp, ovf, out, 0)
            t = self._conv(L, self._conv(L, y, cv["b1a"], sp, ovf), cv["b1b"], sp, ovf)
            self._conv(L, t, cv["b1c"], sp, ovf, out, pl)
            if blk["pool"] == "Avg":
                self._conv(L, y, cv["b2"], sp, ovf, out, 2 * pl)
                a = torch.empty_like(y)
                check(L.ssg_inc_avgpool3_nhwc_x(ptr(y), ptr(a), B, H2, W2, blk["cin"], 1 if sp else 0, blk["cin"], stream()), "ssg_inc_avgpool3_nhwc_x")
                self._conv(L, a, cv["b3"], sp, ovf, out, 3 * pl)
            else:
                self._maxpool(L, y, 3, s, 1, sp, out, 2 * pl)
            y = out
        return y, sp

    def _f32_twin(self):
        if getattr(self, "_twin", None) is None:
            import warnings
            warnings.warn("ssg_amd InceptionNet: an activation left the half range of the split-half path (|v| >= 65520); this batch and "
                          "any later one that overflows is recomputed with precision='f32'", stacklevel=3)
            t = InceptionNet.__new__(InceptionNet)
            t.__dict__.update({k: v for k, v in self.__dict__.items() if k not in ("_folded", "_ovf", "_twin")})
            t.precision, t._folded, t._ovf, t._twin = "f32", None, None, None
            self._twin = t
        return self._twin

    def feature_map(self, x, flip=False):
        """images [B,3,H,W] float32 (NCHW, any device) -> the block-6b map [B,h,w,1536] NHWC fp32 (inception.py:91-100)"""
        return super().feature_map(x, flip)

    def _head(self, gap):
        """[B,1536] pooled map -> model(x) (inception.py:108-114)"""
        L = _lib.lib()
        B = gap.shape[0]
        y = gap
        if self.has_embedding:
            f = self._prepare()["feat"]
            y = torch.empty((B, self.num_features), dtype=torch.float32, device=gap.device)
            check(L.ssg_linear_fwd_f32(ptr(gap), ptr(f.w), ptr(f.bias), ptr(y), B, WIDTH, self.num_features, stream()), "ssg_linear_fwd_f32")
        if self.norm or self.has_embedding:
            out = torch.empty_like(y)
            check(L.ssg_inc_head_finish(ptr(y), ptr(out), B, y.shape[1], 1 if self.norm else 0, stream()), "ssg_inc_head_finish")
            y = out
        return y

    def _features(self, x, flip=False):
        return self._head(self.pooled(*self._fmap(x, flip))[0].contiguous())

    def __call__(self, x, for_eval=None):
        """model(x): [B, num_features]; cut_at_pooling: the NCHW map [B,1536,h,w].  for_eval is accepted and ignored (the reference's
        forward takes no such argument: its cnn.py:16 cannot drive this model)."""
        if self.cut_at_pooling:
            return self.feature_map(x).permute(0, 3, 1, 2).contiguous()
        out = self._features(x)
        if self._overflowed():
            return self._f32_twin()(x)
        return out

    forward = __call__

    def embed_with_flip(self, x, for_eval=False, check_overflow=True):
        """reid/evaluators.py:41-43 on model(x): (model(x) + model(fliplr(x))) under one L2 norm -> [B, D].  The flip is fused into the
        layout kernel; with precision='split' the two orientations run on two HIP streams, as on ResNet."""
        if self.cut_at_pooling:
            raise ValueError("embed_with_flip needs a feature vector per image: cut_at_pooling=True returns the map")
        L = _lib.lib()
        x = x.to(self.device, torch.float32)
        if self.flip_streams and self.precision == "split" and os.environ.get("SSG_FLIP_STREAMS", "1") != "0":
            cur = torch.cuda.current_stream(self.device)
            ready = torch.cuda.Event(); ready.record(cur)
            ab = []
            for st, flip in zip(self._side_streams(), (False, True)):
                st.wait_event(ready)
                with torch.cuda.stream(st):
                    r = self._features(x, flip)
                r.record_stream(cur)
                ab.append(r)
            for st in self._side_streams():
                cur.wait_stream(st)
            a, b = ab
        else:
            a = self._features(x, False)
            b = self._features(x, True)
        if check_overflow and self._overflowed():
            return self._f32_twin().embed_with_flip(x)
        out = torch.empty_like(a)
        check(L.ssg_flip_sum_l2norm(ptr(a), ptr(b), ptr(out), a.shape[0], a.shape[1], stream()), "ssg_flip_sum_l2norm")
        return out


def inception(**kwargs):
    return InceptionNet(**kwargs)


_factory = dict(_rn._factory, inception=inception)


def names():
    """reid/models/__init__.py names(): all six"""
    return sorted(_factory)


def create(name, *args, **kwargs):
    """reid/models/__init__.py create(): models.create('resnet50', num_classes=0, num_split=2, cluster=False) or
    models.create('inception', num_features=256, norm=False)."""
    if name not in _factory:
        raise KeyError("Unknown model:", name)
    return _factory[name](*args, **kwargs)
