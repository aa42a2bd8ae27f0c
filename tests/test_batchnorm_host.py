"""CPU suite of the device batch norm (ssg_amd/batchnorm.py, csrc/batchnorm.hip): the yardstick tests/batchnorm_ref.py against torch's
own F.batch_norm + add + relu under autograd in float64, the module surface (nothing here launches a kernel: eval mode is torch's own
forward), the entry points' argument validation and ssg_bn_num_partials."""
import copy
import os
import sys

import pytest

torch = pytest.importorskip("torch")
from torch import nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batchnorm_ref as ref  # noqa: E402

TOL = 1e-12          # of each array's largest magnitude


@pytest.mark.parametrize("shape,kind", [((3, 5, 7, 5), None), ((4, 6, 8, 4), "large_mean"), ((3, 5, 7, 5), "const"), ((7, 130), None), ((2, 3, 1, 1), None)])
@pytest.mark.parametrize("variant", ["plain", "relu", "relu_res"])
def test_yardstick_vs_torch_float64(shape, kind, variant):
    d = ref.make_case(shape, 11, kind)
    relu, with_res = variant != "plain", variant == "relu_res"
    assert ref.min_margin(d["x"], d["weight"], d["bias"], d["eps"], d["residual"] if with_res else None) >= ref.MARGIN
    x = d["x"].double().requires_grad_(True)
    w, b = d["weight"].double().requires_grad_(True), d["bias"].double().requires_grad_(True)
    r = d["residual"].double().requires_grad_(True) if with_res else None
    rm, rv = d["running_mean"].double(), d["running_var"].double()
    y = F.batch_norm(x, rm, rv, w, b, True, 0.1, d["eps"])
    if with_res:
        y = y + r
    if relu:
        y = torch.relu(y)
    (y * d["gy"].double()).sum().backward()

    fwd = ref.forward(d["x"], d["weight"], d["bias"], d["eps"], relu, d["residual"] if with_res else None)
    bwd = ref.backward(d["x"], d["weight"], fwd, d["gy"], relu)
    n = ref.count(d["x"])
    rrm, rrv = ref.running_update(d["running_mean"], d["running_var"], fwd["mean"], fwd["var"], n, 0.1)
    pairs = [("y", fwd["y"], y.detach()), ("running_mean", rrm, rm), ("running_var", rrv, rv), ("dx", bwd["dx"], x.grad),
             ("dweight", bwd["dweight"], w.grad), ("dbias", bwd["dbias"], b.grad)]
    if with_res:
        pairs.append(("dresidual", bwd["dresidual"], r.grad))
    for name, mine, theirs in pairs:
        assert ref.rel_err(mine, theirs) <= TOL, (name, ref.rel_err(mine, theirs))


def test_cumulative_average_of_the_yardstick_vs_torch_module():
    m = nn.BatchNorm2d(6, momentum=None).double().train()
    xs = [torch.randn(4, 6, 8, 4, generator=torch.Generator().manual_seed(s)).double() for s in (1, 2)]
    rm, rv = m.running_mean.clone(), m.running_var.clone()
    for k, x in enumerate(xs):
        m(x)
        f = ref.forward(x, m.weight.detach(), m.bias.detach(), m.eps)
        rm, rv = ref.running_update(rm, rv, f["mean"], f["var"], ref.count(x), 1.0 / (k + 1))
    assert int(m.num_batches_tracked) == 2
    assert ref.rel_err(rm, m.running_mean) <= TOL and ref.rel_err(rv, m.running_var) <= TOL


# ---------------------------------------------------------------- test-local blocks with the attribute shape of torchvision's
class Mix(nn.Module):
    """stands where a block has a convolution: per-channel scale plus the neighbouring channel (no BLAS, no MIOpen)"""

    def __init__(self, c, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = nn.Parameter(torch.randn(c, generator=g))
        self.b = nn.Parameter(torch.randn(c, generator=g))

    def forward(self, x):
        return x * self.a.view(1, -1, 1, 1) + torch.roll(x, 1, 1) * self.b.view(1, -1, 1, 1)


class Bottleneck(nn.Module):
    def __init__(self, c, downsample=None):
        super().__init__()
        self.conv1, self.bn1 = Mix(c, 1), nn.BatchNorm2d(c)
        self.conv2, self.bn2 = Mix(c, 2), nn.BatchNorm2d(c)
        self.conv3, self.bn3 = Mix(c, 3), nn.BatchNorm2d(c)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        residual = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            residual = self.downsample(x)
        out += residual
        return self.relu(out)


class BasicBlock(nn.Module):
    def __init__(self, c, downsample=None):
        super().__init__()
        self.conv1, self.bn1 = Mix(c, 4), nn.BatchNorm2d(c)
        self.relu = nn.ReLU(inplace=True)
        self.conv2, self.bn2 = Mix(c, 5), nn.BatchNorm2d(c)
        self.downsample = downsample

    def forward(self, x):
        residual = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.downsample is not None:
            residual = self.downsample(x)
        out += residual
        return self.relu(out)


class OddBlock(nn.Module):
    """not the shape of a residual block: keeps its forward"""

    def __init__(self, c):
        super().__init__()
        self.conv1, self.bn1, self.relu = Mix(c, 6), nn.BatchNorm2d(c), nn.ReLU()
        self.extra = nn.BatchNorm2d(c, affine=False)

    def forward(self, x):
        return self.extra(self.relu(self.bn1(self.conv1(x))))


class Net(nn.Module):
    """stem (conv1, bn1, relu, maxpool), layer1 of two blocks, a block of another shape, and a BatchNorm1d the swap takes too"""

    def __init__(self, c=6):
        super().__init__()
        self.conv1, self.bn1, self.relu, self.maxpool = Mix(c, 7), nn.BatchNorm2d(c), nn.ReLU(inplace=True), nn.Identity()
        self.layer1 = nn.Sequential(Bottleneck(c, nn.Sequential(Mix(c, 8), nn.BatchNorm2d(c))), BasicBlock(c))
        self.odd = OddBlock(c)
        self.feat_bn = nn.BatchNorm1d(c)
        self.no_stats = nn.BatchNorm1d(c, track_running_stats=False)

    def forward(self, x):
        for name, module in self._modules.items():          # the reference's loop over base._modules (reid/models/resnet.py)
            if name == "odd":
                break
            x = module(x)
        x = self.odd(x).mean((2, 3))
        return self.feat_bn(x) + self.no_stats(x)


def randomise(net, seed=5):
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            if m.affine:
                m.weight.data = torch.rand(m.weight.shape, generator=g) + 0.5
                m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.3
            if m.track_running_stats:
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
    return net


def test_module_state_dict_keys_and_constructor():
    from ssg_amd import batchnorm as bn
    import ssg_amd
    assert ssg_amd.BatchNorm2d is bn.BatchNorm2d and ssg_amd.use_device_batchnorm is bn.use_device_batchnorm
    assert ssg_amd.batch_norm_train is bn.batch_norm_train and ssg_amd.BatchNorm1d is bn.BatchNorm1d
    for mine, theirs in ((bn.BatchNorm2d(5, relu=True), nn.BatchNorm2d(5)), (bn.BatchNorm1d(5), nn.BatchNorm1d(5))):
        assert isinstance(mine, type(theirs))
        assert list(mine.state_dict()) == list(theirs.state_dict())
        mine.load_state_dict(theirs.state_dict())
    assert "relu=True" in repr(bn.BatchNorm2d(5, relu=True))
    for kw in (dict(affine=False), dict(track_running_stats=False)):
        with pytest.raises(ValueError):
            bn.BatchNorm2d(5, **kw)


@pytest.mark.parametrize("fuse", [False, True])
def test_use_device_batchnorm_keeps_parameters_and_eval_bits(fuse):
    from ssg_amd import batchnorm as bn
    net = randomise(Net()).eval()
    plain = copy.deepcopy(net)
    before = dict(net.named_parameters())
    buffers = dict(net.named_buffers())
    keys = list(net.state_dict())
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    assert bn.use_device_batchnorm(net, fuse=fuse) is net
    assert net._ssg_bn_skipped == ["odd.extra", "no_stats"]
    assert list(net.state_dict()) == keys and list(net._modules) == list(plain._modules)
    after = dict(net.named_parameters())
    assert after.keys() == before.keys() and all(after[k] is before[k] for k in before)            # Parameter identity
    assert all(v is buffers[k] for k, v in net.named_buffers())
    assert {id(p) for grp in opt.param_groups for p in grp["params"]} == {id(p) for p in net.parameters()}
    swapped = [n for n, m in net.named_modules() if isinstance(m, (bn.BatchNorm1d, bn.BatchNorm2d))]
    assert swapped == ["bn1", "layer1.0.bn1", "layer1.0.bn2", "layer1.0.bn3", "layer1.0.downsample.1", "layer1.1.bn1", "layer1.1.bn2", "odd.bn1", "feat_bn"]
    assert isinstance(net.feat_bn, bn.BatchNorm1d) and not net.feat_bn.training
    if fuse:
        assert isinstance(net.relu, nn.Identity) and net.bn1.relu
        assert type(net.layer1[0]).__name__ == "FusedBottleneck" and isinstance(net.layer1[0], Bottleneck)
        assert type(net.layer1[1]).__name__ == "FusedBasicBlock"
        assert [net.layer1[0].bn1.relu, net.layer1[0].bn2.relu, net.layer1[0].bn3.relu, net.layer1[0].downsample[1].relu] == [True, True, True, False]
        assert type(net.odd) is OddBlock and not net.odd.bn1.relu                                 # another shape: the plain swap
    else:
        assert isinstance(net.relu, nn.ReLU) and type(net.layer1[0]) is Bottleneck and not net.layer1[0].bn3.relu
    x = torch.randn(3, 6, 5, 4, generator=torch.Generator().manual_seed(9))
    assert torch.equal(net(x), plain(x))                                                          # eval mode: torch's own forward, same bits
    bn.use_device_batchnorm(net, fuse=fuse)                                                       # a second call changes nothing
    assert torch.equal(net(x), plain(x)) and net._ssg_bn_skipped == ["odd.extra", "no_stats"]
    # under nn.DataParallel the walk goes through .module
    wrapped = nn.DataParallel(randomise(Net()).eval()) if torch.cuda.is_available() else None
    if wrapped is None:
        class Wrapper(nn.Module):                          # the same attribute shape without needing a GPU
            def __init__(self, module):
                super().__init__()
                self.module = module
        wrapped = Wrapper(randomise(Net()).eval())
    bn.use_device_batchnorm(wrapped, fuse=fuse)
    assert wrapped._ssg_bn_skipped == ["module.odd.extra", "module.no_stats"] and isinstance(wrapped.module.bn1, bn.BatchNorm2d)


def test_eval_mode_is_bit_equal_to_the_torch_module():
    from ssg_amd import batchnorm as bn
    x = torch.randn(4, 5, 3, 2, generator=torch.Generator().manual_seed(3))
    r = torch.randn(4, 5, 3, 2, generator=torch.Generator().manual_seed(4))
    theirs = randomise(nn.BatchNorm2d(5)).eval()
    mine = bn.BatchNorm2d(5, relu=True).eval()
    mine.load_state_dict(theirs.state_dict())
    assert torch.equal(mine(x), torch.relu(theirs(x)))
    assert torch.equal(mine(x, r), torch.relu(theirs(x) + r))
    mine.relu = False
    assert torch.equal(mine(x), theirs(x))
    t1, m1 = randomise(nn.BatchNorm1d(5)).eval(), bn.BatchNorm1d(5).eval()
    m1.load_state_dict(t1.state_dict())
    assert torch.equal(m1(x[:, :, 0, 0]), t1(x[:, :, 0, 0]))


def test_one_value_per_channel_raises_torchs_text():
    from ssg_amd import batchnorm as bn
    for shape, cls, tcls in (((1, 3, 1, 1), bn.BatchNorm2d, nn.BatchNorm2d), ((1, 3), bn.BatchNorm1d, nn.BatchNorm1d)):
        x = torch.zeros(shape)
        with pytest.raises(ValueError) as theirs:
            tcls(3).train()(x)
        with pytest.raises(ValueError) as mine:
            cls(3).train()(x)
        assert str(mine.value) == str(theirs.value)
    with pytest.raises(ValueError, match="residual"):
        bn.batch_norm_train(torch.zeros(2, 3), torch.ones(3), torch.zeros(3), None, None, residual=torch.zeros(2, 4))
    with pytest.raises(ValueError, match="go together"):
        bn.batch_norm_train(torch.zeros(2, 3), torch.ones(3), torch.zeros(3), torch.zeros(3), None)


def test_entry_points_validate_before_any_launch():
    from ssg_amd import _lib
    L = _lib.lib()
    one = 8                                      # a non-NULL, never dereferenced pointer: every call below is refused before a launch

    def calls(N, C, HW, cl, p=one):
        return (("ssg_bn_stats_f32", lambda: L.ssg_bn_stats_f32(p, N, C, HW, cl, 1e-5, 0.1, None, None, None, p, p, 1 << 30, None)),
                ("ssg_bn_apply_f32", lambda: L.ssg_bn_apply_f32(p, p, p, p, None, 1, N, C, HW, cl, p, None)),
                ("ssg_bn_backward_reduce_f32", lambda: L.ssg_bn_backward_reduce_f32(p, p, None, p, N, C, HW, cl, p, None, None, p, 1 << 30, None)),
                ("ssg_bn_backward_apply_f32", lambda: L.ssg_bn_backward_apply_f32(p, p, None, p, p, p, N, C, HW, cl, p, None, None)))

    for (N, C, HW, cl), word in (((4, 0, 8, 0), "C=0"), ((4, -3, 8, 1), "C=-3"), ((1, 3, 1, 0), "fewer than 2"), ((0, 3, 4, 0), "N=0"),
                                 ((2, 3, 0, 0), "HW=0"), ((1 << 15, 1 << 8, 1 << 8, 0), "2^31"), ((1 << 15, 1 << 8, 1 << 8, 1), "2^31"),
                                 ((2, 70000, 4, 0), "65535")):
        for name, call in calls(N, C, HW, cl):
            assert call() == -1, (name, N, C, HW, cl)
            msg = L.ssg_last_error().decode()
            assert name in msg and word in msg, msg
        assert L.ssg_bn_num_partials(N, C, HW, cl) == -1 and L.ssg_bn_workspace_bytes(N, C, HW, cl) == 0
    for name, call in calls(4, 3, 8, 0, None):                                                  # a good shape, NULL pointers
        assert call() == -1 and ("%s: NULL pointer" % name) in L.ssg_last_error().decode(), name
    # the workspace: missing, too small
    need = L.ssg_bn_workspace_bytes(4, 3, 8, 0)
    assert L.ssg_bn_stats_f32(one, 4, 3, 8, 0, 1e-5, 0.1, None, None, None, one, None, need, None) == -1 and b"workspace" in L.ssg_last_error()
    assert L.ssg_bn_stats_f32(one, 4, 3, 8, 0, 1e-5, 0.1, None, None, None, one, one, need - 8, None) == -1 and b"workspace" in L.ssg_last_error()
    assert L.ssg_bn_backward_reduce_f32(one, one, None, one, 4, 3, 8, 0, one, None, None, one, need - 8, None) == -1
    # eps, momentum; the cumulative average needs the counter
    assert L.ssg_bn_stats_f32(one, 4, 3, 8, 0, -1.0, 0.1, None, None, None, one, one, need, None) == -1 and b"eps" in L.ssg_last_error()
    assert L.ssg_bn_stats_f32(one, 4, 3, 8, 0, 1e-5, 1.5, None, None, None, one, one, need, None) == -1 and b"momentum" in L.ssg_last_error()
    assert L.ssg_bn_stats_f32(one, 4, 3, 8, 0, 1e-5, -1.0, None, None, None, one, one, need, None) == -1 and b"num_batches_tracked" in L.ssg_last_error()


def test_num_partials_and_workspace():
    from ssg_amd import _lib
    L = _lib.lib()
    # NCHW: a workgroup takes at least 4096 values of a channel, 2048 workgroups are aimed at, at most 256 per channel
    assert L.ssg_bn_num_partials(2, 3, 1, 0) == 1 and L.ssg_bn_num_partials(32, 8, 128, 0) == 1       # 4096 values: one workgroup
    assert L.ssg_bn_num_partials(33, 8, 128, 0) == 2                                                  # 4224 values: the smallest split
    assert L.ssg_bn_num_partials(128, 64, 64 * 32, 0) == 32                                           # layer1 at B = 128: 64 * 32 = 2048 workgroups
    assert L.ssg_bn_num_partials(128, 2048, 16 * 8, 0) == 1
    assert L.ssg_bn_num_partials(128, 3, 1 << 20, 0) == 256
    # channel contiguous: column tiles of 64 channels (256 from C = 256 on, four per lane), at least 64 rows per workgroup
    assert L.ssg_bn_num_partials(7, 130, 1, 0) == 1 and L.ssg_bn_num_partials(7, 130, 1, 1) == 1
    assert L.ssg_bn_num_partials(128, 2048, 1, 0) == 2                                                # feat_bn
    assert L.ssg_bn_num_partials(3, 5, 35, 1) == 2 and L.ssg_bn_num_partials(128, 64, 2048, 1) == 256
    for N, C, HW, cl in ((33, 8, 128, 0), (128, 64, 2048, 0), (7, 130, 1, 0), (128, 64, 2048, 1)):
        assert L.ssg_bn_workspace_bytes(N, C, HW, cl) == 16 * C * L.ssg_bn_num_partials(N, C, HW, cl)
