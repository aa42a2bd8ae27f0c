"""Host half of the train-mode head tests (no GPU): the names, the argument checks that come before any launch, the class rules of the
Python layer, and use_device_head on a hand-built look-alike of the reference's model (tests/head_ref.py)."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_ref as ref  # noqa: E402

nn = torch.nn


@pytest.fixture(scope="module")
def L():
    from ssg_amd import _lib
    return _lib.lib()


def test_new_names_resolve():
    import ssg_amd
    for n in ("stripe_pool_train", "linear_train", "Linear", "DeviceHeadMixin", "use_device_head"):
        assert callable(getattr(ssg_amd, n)), n
    assert issubclass(ssg_amd.Linear, nn.Linear)
    m = ssg_amd.Linear(64, 7)
    assert list(m.state_dict()) == ["weight", "bias"] and m.weight.shape == (7, 64)
    assert list(ssg_amd.Linear(64, 7, bias=False).state_dict()) == ["weight"]


def test_no_reduction_is_cut_across_workgroups(L):
    """the Linear kernels have no slice count and no workspace to query: the header declares neither"""
    from ssg_amd import _lib
    declared = _lib.parse_header()
    assert not [n for n in declared if n.startswith("ssg_linear_") and ("num_slices" in n or "workspace" in n)]
    for n in ("ssg_linear_fwd_f32", "ssg_linear_dgrad_f32", "ssg_linear_wgrad_f32", "ssg_gap_stripes_bwd"):
        assert n in declared and hasattr(L, n)


def test_bad_arguments_are_refused_before_any_launch(L):
    # NULL pointers
    assert L.ssg_linear_fwd_f32(None, None, None, None, 4, 64, 8, None) == -1 and b"NULL" in L.ssg_last_error()
    assert L.ssg_linear_dgrad_f32(None, None, None, 4, 64, 8, None) == -1 and b"NULL" in L.ssg_last_error()
    assert L.ssg_linear_wgrad_f32(None, None, None, None, 4, 64, 8, None) == -1 and b"NULL" in L.ssg_last_error()
    assert L.ssg_gap_stripes_bwd(None, 1, None, 2, 8, 4, 64, 2, None) == -1 and b"NULL" in L.ssg_last_error()
    # K % 32 != 0, N = 0, B = 0 (and their negatives)
    for (B, K, N) in [(4, 48, 8), (4, 0, 8), (4, 64, 0), (0, 64, 8), (4, 33, 8), (-1, 64, 8), (4, 64, -3), (4, -32, 8)]:
        assert L.ssg_linear_fwd_f32(None, None, None, None, B, K, N, None) == -1 and b"ssg_linear_fwd_f32" in L.ssg_last_error()
        assert b"K % 32" in L.ssg_last_error()
        assert L.ssg_linear_dgrad_f32(None, None, None, B, K, N, None) == -1 and b"ssg_linear_dgrad_f32" in L.ssg_last_error()
        assert L.ssg_linear_wgrad_f32(None, None, None, None, B, K, N, None) == -1 and b"ssg_linear_wgrad_f32" in L.ssg_last_error()
    # the pool: S > h, unsupported C, empty sides, a mask that names a set that does not exist
    for (B, H, W, C, S, mask) in [(2, 4, 4, 64, 5, 1), (2, 8, 4, 66, 2, 1), (2, 8, 4, 0, 2, 1), (0, 8, 4, 64, 2, 1), (2, 0, 4, 64, 2, 1), (2, 8, 0, 64, 2, 1),
                                  (2, 8, 4, 64, 0, 1), (2, 8, 4, 64, 2, 8), (2, 8, 4, 64, 1, 2), (2, 8, 4, 64, 2, -1)]:
        assert L.ssg_gap_stripes_bwd(None, mask, None, B, H, W, C, S, None) == -1 and b"ssg_gap_stripes_bwd" in L.ssg_last_error()
    assert L.ssg_gap_stripes_bwd(None, 1, None, 2, 8, 4, 66, 2, None) == -1 and b"C % 4" in L.ssg_last_error()
    assert L.ssg_gap_stripes(None, None, 2, 4, 4, 64, 5, None) == -1                        # the forward refuses S > h as it always did


def test_unsupported_arguments_raise_valueerror_naming_the_rule():
    import ssg_amd
    x, w = torch.zeros(4, 64), torch.zeros(8, 64)
    for args, word in [((torch.zeros(4, 48), torch.zeros(8, 48)), "K % 32"), ((x, torch.zeros(0, 64)), "at least 1"), ((torch.zeros(0, 64), w), "B >= 1"),
                       ((x, torch.zeros(8, 32)), "features"), ((x, torch.zeros(64, 8).t()), "contiguous"), ((x, w, torch.zeros(7)), "bias"),
                       ((x.double(), w.double()), "float32"), ((x, w, torch.zeros(8).double()), "float32"), ((torch.zeros(2, 4, 64), w), r"\[B, K\]"),
                       ((x, torch.zeros(64)), r"\[N, K\]")]:
        with pytest.raises(ValueError, match=word):
            ssg_amd.linear_train(*args)
    for args in [(48, 8), (0, 8), (64, 0)]:
        with pytest.raises(ValueError):
            ssg_amd.Linear(*args)
    m = torch.zeros(2, 64, 4, 4)
    for args, word in [((m, 5), "height"), ((torch.zeros(2, 66, 4, 4), 2), "C % 4"), ((m, 0), "num_split"), ((m.double(), 2), "float32"),
                       ((torch.zeros(2, 64, 4), 2), r"\[B, C, h, w\]"), ((torch.zeros(0, 64, 4, 4), 2), "empty")]:
        with pytest.raises(ValueError, match=word):
            ssg_amd.stripe_pool_train(*args)


def test_forward_without_a_gpu_raises_ssgerror():
    import ssg_amd
    assert issubclass(ssg_amd.SSGError, RuntimeError)
    if not torch.cuda.is_available():                        # there is no CPU fallback
        with pytest.raises(ssg_amd.SSGError):
            ssg_amd.linear_train(torch.zeros(4, 64), torch.zeros(8, 64))
        with pytest.raises(ssg_amd.SSGError):
            ssg_amd.stripe_pool_train(torch.zeros(2, 64, 4, 4), 2)


def _model(num_split, num_classes=5):
    m = ref.HeadNet(num_split=num_split, num_classes=num_classes)
    m.odd = nn.Linear(48, 8)                                  # K % 32 != 0
    m.wide = nn.Linear(64, 8).double()                        # not float32
    return m


@pytest.mark.parametrize("num_split", [1, 2])
def test_use_device_head_on_a_look_alike(num_split):
    import ssg_amd
    m = _model(num_split)
    old_cls = type(m)
    before = dict(m.named_parameters())
    keys = list(m.state_dict().keys())
    opt = torch.optim.SGD([dict(params=m.base.parameters(), lr=0.01), dict(params=[p for n, p in m.named_parameters() if not n.startswith("base.")])], lr=0.1)
    assert ssg_amd.use_device_head(m) is m
    assert m._ssg_linear_skipped == ["odd", "wide"]
    for name in ("feat", "classifier_x2"):
        assert type(getattr(m, name)) is ssg_amd.Linear, name
    assert type(m.base.fc) is ssg_amd.Linear and type(m.odd) is nn.Linear and type(m.wide) is nn.Linear
    assert m.feat.bias is None and m.classifier_x2.bias is not None and m.classifier_x2.out_features == 5
    after = dict(m.named_parameters())
    assert list(after) == list(before) and all(after[k] is before[k] for k in before)       # the same Parameter objects
    assert list(m.state_dict().keys()) == keys
    assert all(any(p is q for q in after.values()) for g in opt.param_groups for p in g["params"])
    assert isinstance(m, ssg_amd.DeviceHeadMixin) and isinstance(m, old_cls) and type(m) is not old_cls
    assert type(m).__mro__[1] is ssg_amd.DeviceHeadMixin and type(m).__mro__[2] is old_cls
    assert type(m).forward is ssg_amd.DeviceHeadMixin.forward and "forward" not in m.__dict__   # no method bound on the instance
    # a second call changes nothing
    cls, mods = type(m), dict(m.named_modules())
    ssg_amd.use_device_head(m)
    assert type(m) is cls and m._ssg_linear_skipped == ["odd", "wide"] and all(v is mods[k] for k, v in m.named_modules())
    # two models of one class share the swapped class
    assert type(ssg_amd.use_device_head(_model(num_split))) is cls


def test_use_device_head_under_dataparallel_and_missing_attribute():
    import ssg_amd
    m = _model(2)
    old_cls = type(m)
    d = nn.DataParallel(m)
    assert ssg_amd.use_device_head(d) is d
    assert type(d) is nn.DataParallel and issubclass(type(d.module), old_cls) and isinstance(d.module, ssg_amd.DeviceHeadMixin)
    assert d._ssg_linear_skipped == ["module.odd", "module.wide"] and type(d.module.feat) is ssg_amd.Linear
    replica = d.module._replicate_for_data_parallel()       # what DataParallel.replicate makes: the class travels, nothing is bound
    assert type(replica) is type(d.module)
    for attr in ("base", "num_split", "num_features", "num_classes", "cluster"):
        bad = _model(2)
        if attr == "base":
            del bad._modules["base"]
        else:
            delattr(bad, attr)
        for host in (bad, nn.DataParallel(bad)):
            with pytest.raises(ValueError, match=attr):
                ssg_amd.use_device_head(host)
        assert type(bad) is old_cls and (attr == "base" or type(bad.feat) is nn.Linear)     # nothing was changed


def test_use_device_head_composes_with_the_other_swaps():
    """any order of the five swaps ends in the same module classes"""
    import ssg_amd
    steps = [lambda m: ssg_amd.use_device_conv(m, strided=True), ssg_amd.use_device_maxpool, ssg_amd.use_device_batchnorm, ssg_amd.use_device_head]
    seen = []
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 3, 0, 1]):
        m = ref.HeadNet(num_split=2, num_classes=5)
        for i in order:
            steps[i](m)
        assert m._ssg_conv_skipped == [] and m._ssg_maxpool_skipped == [] and m._ssg_bn_skipped == [] and m._ssg_linear_skipped == []
        assert isinstance(m, ssg_amd.DeviceHeadMixin) and isinstance(m.feat_bn, ssg_amd.BatchNorm1d) and isinstance(m.feat, ssg_amd.Linear)
        assert isinstance(m.base.conv1, ssg_amd.StridedConv2d) and isinstance(m.base.maxpool, ssg_amd.MaxPool2d)
        seen.append([(n, type(c).__name__) for n, c in m.named_modules()])
    assert seen[0] == seen[1] == seen[2]
