"""Yardstick of the train-mode head tests (tests/test_head_host.py, tests/test_gpu_head.py): seeded cases, torch's `F.avg_pool2d` /
`F.linear` and their autograd in float64 on the CPU, the absolute-value companion A of each output, and a hand-built look-alike of the
reference's model (a tiny `base` with conv1 .. layer4, avgpool entries, `feat`, `feat_bn`, `relu`, `drop`, `classifier_x2`) whose
forward pools with separate `F.avg_pool2d` calls as the reference does.  The unit roundoff, the (L + 2) 2^-24 A bound and the model
blocks come from tests/conv_train_ref.py.

None of the three Linear kernels cuts its reduction across workgroups (there is no ssg_linear_*_num_slices), so there is no
multi-slice case to look for: the fixed cut inside a workgroup -- wave w of 4 takes steps [128 t + 32 w, 128 t + 32 w + 32) of the
reduction -- is met by the case table itself, with reductions of 1, 5, 32, 33, 64, 70 (a ragged third wave), 96, 128 (exactly one
stage), 192, 512, 751 (a ragged last stage) and 2048."""
from functools import lru_cache

import torch
import torch.nn.functional as Fn
from torch import nn

from conv_train_ref import Bottleneck, downsample  # noqa: F401
from train_common import U, bound  # noqa: F401

# name -> (B, h, w, C, S, seed)
POOL_CASES = {
    "even": (2, 8, 4, 64, 2, 601),
    "ragged_h": (3, 7, 3, 64, 2, 602),          # h % S != 0: the last row is in no stripe
    "three": (1, 6, 2, 128, 3, 603),
    "single": (2, 4, 4, 64, 1, 604),            # a single set
    "rows": (1, 5, 1, 64, 5, 605),              # one-row stripes, w = 1
    "real_c": (2, 8, 4, 2048, 2, 606),          # the real C
}
# which sets receive a gradient: all of them, set 0 alone, the last stripe alone
POOL_MASKS = ("all", "set0", "last")

# name -> (B, K, N, bias, seed)
LINEAR_CASES = {
    "smallest": (1, 32, 1, True, 611),
    "one_tile": (5, 64, 64, False, 612),
    "ragged": (33, 96, 70, True, 613),          # ragged B and N, K an odd multiple of 32
    "tiles": (32, 128, 192, False, 614),
    "feat18": (128, 512, 2048, False, 615),     # resnet18's feat
    "classifier": (64, 2048, 751, True, 616),   # classifier_x2
}
LINEAR_OUTS = ("y", "dx", "dw", "db")


def nsets(S):
    return S + 1 if S > 1 else 1


def present(S, mask):
    """the indices of the sets that receive a gradient under a named mask"""
    n = nsets(S)
    return list(range(n)) if mask == "all" else [0] if mask == "set0" else [n - 1]


def pool_sets(x, S):
    """the reference's pools: the global average, then one average per stripe of h // S rows"""
    B, C, h, w = x.shape
    out = [Fn.avg_pool2d(x, (h, w)).view(B, C)]
    if S > 1:
        hs = h // S
        for s in range(S):
            out.append(Fn.avg_pool2d(x[:, :, hs * s: hs * (s + 1), :], (hs, w)).view(B, C))
    return out


def _pool_dx(x, S, gs, idx):
    x = x.clone().requires_grad_(True)
    sets = pool_sets(x, S)
    (dx,) = torch.autograd.grad([sets[i] for i in idx], x, [gs[i] for i in idx])
    return dx


@lru_cache(maxsize=None)
def pool_reference(B, h, w, C, S, seed):
    """dict: x [B,C,h,w] and gs [nsets][B,C] float32; sets / A_sets float64; dx[mask] / A_dx[mask] float64 -- computed once, never
    modified.  A of a set is the same average of |x|; A of dX is |g0| / (h w) + |g_s| / ((h // S) w) over the present sets."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, h, w, generator=g, dtype=torch.float32)
    gs = [torch.randn(B, C, generator=g, dtype=torch.float32) for _ in range(nsets(S))]
    x64, g64 = x.double(), [t.double() for t in gs]
    d = dict(x=x, gs=gs, sets=pool_sets(x64, S), A_sets=pool_sets(x64.abs(), S), dx={}, A_dx={})
    d["L"] = [h * w] + [(h // S) * w] * (nsets(S) - 1)
    for m in POOL_MASKS:
        idx = present(S, m)
        d["dx"][m] = _pool_dx(x64, S, g64, idx)
        d["A_dx"][m] = _pool_dx(x64, S, [t.abs() for t in g64], idx)
    return d


def linear_outputs(x, w, b, gy, dtype):
    """{y, dx, dw, db} of F.linear and its autograd in `dtype` on the CPU (db None without a bias)"""
    x = x.to(dtype).clone().requires_grad_(True)
    w = w.to(dtype).clone().requires_grad_(True)
    b = None if b is None else b.to(dtype).clone().requires_grad_(True)
    y = Fn.linear(x, w, b)
    grads = torch.autograd.grad(y, (x, w) if b is None else (x, w, b), gy.to(dtype))
    return dict(y=y.detach(), dx=grads[0], dw=grads[1], db=None if b is None else grads[2])


@lru_cache(maxsize=None)
def linear_reference(B, K, N, bias, seed):
    """(case {x, w, b, gy}, ref64, A, L) -- computed once, never modified"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, K, generator=g, dtype=torch.float32)
    w = torch.randn(N, K, generator=g, dtype=torch.float32) * (1.0 / K ** 0.5)
    b = torch.randn(N, generator=g, dtype=torch.float32) if bias else None
    gy = torch.randn(B, N, generator=g, dtype=torch.float32)
    d = dict(x=x, w=w, b=b, gy=gy)
    ref = linear_outputs(x, w, b, gy, torch.float64)
    A = linear_outputs(x.abs(), w.abs(), None if b is None else b.abs(), gy.abs(), torch.float64)
    L = dict(y=K + (1 if bias else 0), dx=N, dw=B, db=B)        # the bias costs one more term on y
    return d, ref, A, L


def linear_outs(case):
    return LINEAR_OUTS if case[3] else LINEAR_OUTS[:3]


# ---- the look-alike model -----------------------------------------------------------------------------------------------------------------

class Base(nn.Module):
    """the entries the reference's forward walks: a 7x7 stem, the pool, one stride-2 bottleneck as layer4, then avgpool and fc"""

    def __init__(self, planes=64):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer4 = nn.Sequential(Bottleneck(64, planes, 2, downsample(64, planes * 4, 2)))
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(planes * 4, 10)


class HeadNet(nn.Module):
    """attributes and module names of the reference's ResNet; the forward pools the way the reference does, one F.avg_pool2d per set
    and one more for the embedding"""

    def __init__(self, num_split=2, num_classes=0, num_features=128, dropout=0.1, cluster=False):
        super().__init__()
        self.num_split, self.num_classes, self.num_features, self.dropout, self.cluster = num_split, num_classes, num_features, dropout, cluster
        self.base = Base()
        planes = self.base.fc.in_features
        if dropout > 0:
            self.drop = nn.Dropout(dropout)
        if num_features > 0:
            self.feat = nn.Linear(planes, num_features, bias=False)
            self.feat_bn = nn.BatchNorm1d(num_features)
            self.relu = nn.ReLU(inplace=True)
        if num_classes > 0:
            self.classifier_x2 = nn.Linear(num_features, num_classes)

    def forward(self, x, for_eval=False):
        for name, module in self.base._modules.items():
            if name == "avgpool":
                break
            x = module(x)
        sets = pool_sets(x, self.num_split)
        x1 = sets if self.num_split > 1 else sets[0]
        if self.num_features > 0:
            x2 = self.relu(self.feat_bn(self.feat(Fn.avg_pool2d(x, x.shape[2:]).flatten(1))))
        if self.num_classes > 0:
            x2 = self.classifier_x2(self.drop(x2))
        if for_eval and isinstance(x1, list):
            return torch.cat(x1, dim=1), x2
        if self.cluster:
            return x1, x2, self.assignment(torch.cat(x1, dim=1) if isinstance(x1, list) else x1)
        return x1, x2


def flat_outputs(out):
    """the tensors of a model output (tuple of tensors and lists of tensors) in order"""
    flat = []
    for o in out:
        flat.extend(o if isinstance(o, (list, tuple)) else [o])
    return flat
