"""CPU suite of the one module-swap walker behind use_device_conv / use_device_maxpool / use_device_batchnorm / use_device_head
(ssg_amd/_train.py), on a toy model and a toy device class: no GPU, no library."""
import pytest

torch = pytest.importorskip("torch")
from torch import nn  # noqa: E402


class _Dev(nn.Linear):
    """the toy device class"""


class _Odd(nn.Linear):
    """another subclass of the family: never swapped"""


def _toy():
    m = nn.Module()
    m.a = nn.Linear(32, 4)
    m.register_module("gap", None)                              # a None child
    m.block = nn.Sequential(nn.Linear(3, 4), _Odd(32, 4), nn.ReLU(), nn.Sequential(nn.Linear(64, 8)))
    m.z = nn.Linear(5, 5)
    return m


def _swap_all(model, after=None):
    from ssg_amd import _train

    def swap(m):                                                # the toy class takes in_features % 32 == 0
        return _train.adopt(_Dev(m.in_features, m.out_features, device="meta"), m, ("weight", "bias")) if m.in_features % 32 == 0 else None

    return _train.swap_modules(model, "_toy_skipped", nn.Linear, (nn.Linear,), lambda m: isinstance(m, _Dev), swap, after)


def test_swaps_the_exact_type_and_lists_the_rest_depth_first():
    m = _toy().eval()
    before = dict(m.named_parameters())
    assert _swap_all(m) is m
    assert m._toy_skipped == ["block.0", "block.1", "z"]        # depth-first in _modules order; the subclass is listed, not swapped
    assert type(m.a) is _Dev and type(m.block[3][0]) is _Dev and type(m.block[1]) is _Odd and type(m.z) is nn.Linear
    assert m.gap is None and list(m._modules) == ["a", "gap", "block", "z"]
    after = dict(m.named_parameters())
    assert list(after) == list(before) and all(after[k] is before[k] for k in before)      # the same Parameter objects
    assert m.a.training is False and m.a.weight.device.type == "cpu"


def test_dataparallel_prefix():
    d = nn.DataParallel(_toy())
    _swap_all(d)
    assert d._toy_skipped == ["module.block.0", "module.block.1", "module.z"] and type(d.module.a) is _Dev


def test_second_call_is_a_no_op():
    m = _swap_all(_toy())
    mods = dict(m.named_modules())
    _swap_all(m)
    assert m._toy_skipped == ["block.0", "block.1", "z"]        # modules on the device path are neither swapped nor listed
    assert all(v is mods[k] for k, v in m.named_modules()) and len(mods) == len(dict(m.named_modules()))


def test_post_visit_hook_is_called_once_per_container():
    m = _toy()
    relu, inner, block = m.block[2], m.block[3], m.block
    seen = []
    _swap_all(m, seen.append)
    # after its children, on everything the walk goes into and on the model itself; never on a module of the family
    assert len(seen) == 4 and all(a is b for a, b in zip(seen, [relu, inner, block, m]))
    assert type(inner[0]) is _Dev                               # the hook of a container runs after that container's swaps
