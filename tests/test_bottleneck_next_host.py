"""Host side of the next-conv instance of the layer1 fused block (csrc/bottleneck.hip): the shape predicate, the argument validation
of ssg_bottleneck_attach_next / ssg_bottleneck_nhwc_x with null pointers (nothing is launched, no GPU needed) and the SSG_BN_L1_NEXT
switch as the library parses it."""
import ctypes

import pytest

from ssg_amd import _lib


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_next_supported_shapes(L):
    assert L.ssg_bottleneck_next_supported(64, 32, 256, 64, 128) == 1
    assert L.ssg_bottleneck_next_supported(4, 32, 256, 64, 128) == 1
    for bad in ((0, 32, 256, 64, 128), (-4, 32, 256, 64, 128), (6, 32, 256, 64, 128), (64, 16, 256, 64, 128), (64, 32, 512, 64, 128),
                (64, 32, 256, 128, 128), (64, 32, 256, 64, 64), (64, 32, 256, 64, 256), (32, 16, 512, 128, 256)):
        assert L.ssg_bottleneck_next_supported(*bad) == 0, bad


def test_attach_next_validates_its_arguments(L):
    one = ctypes.c_void_p(16)        # any non-null address: a descriptor is only stored, never dereferenced on the host
    assert L.ssg_bottleneck_attach_next(None, None, None, None, None, 128) == -1
    assert b"ssg_bottleneck_attach_next" in L.ssg_last_error()
    assert L.ssg_bottleneck_attach_next(None, one, one, None, None, 128) == -1      # no weights
    assert L.ssg_bottleneck_attach_next(one, None, one, None, None, 128) == -1      # no bias
    assert L.ssg_bottleneck_attach_next(one, one, None, None, None, 128) == -1      # no per-row scale
    assert L.ssg_bottleneck_attach_next(one, one, one, None, None, 64) == -1        # MIDN
    assert L.ssg_bottleneck_attach_next(one, one, one, one, one, 128) == -1         # y1n aliases out_s2
    # a failed attach leaves the slot empty: the block call fails on ITS OWN arguments (B = 0), with its plain message
    assert L.ssg_bottleneck_nhwc_x(None, None, None, None, None, None, None, None, None, None, None, 0, 64, 32, 256, 64, None, None) == -1
    assert b"unsupported block" in L.ssg_last_error()


def test_block_call_consumes_the_descriptor_even_when_it_fails(L):
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(32)
    assert L.ssg_bottleneck_attach_next(one, one, one, two, None, 128) == 0
    # the plain validation comes first (null scales): error, descriptor gone
    assert L.ssg_bottleneck_nhwc_x(one, None, None, None, None, None, None, None, None, None, two, 1, 64, 32, 256, 64, None, None) == -1
    assert b"unsupported block" in L.ssg_last_error()
    # a supported plain shape without a next-conv instance (layer2): an error that names the instance, never a plain launch
    assert L.ssg_bottleneck_attach_next(one, one, one, two, None, 128) == 0
    three = ctypes.c_void_p(48)
    assert L.ssg_bottleneck_nhwc_x(one, one, one, one, one, one, one, one, one, one, three, 1, 8, 16, 512, 128, None, None) == -1
    assert b"next-conv" in L.ssg_last_error()
    # ... and an output that aliases x
    assert L.ssg_bottleneck_attach_next(one, one, one, one, None, 128) == 0
    assert L.ssg_bottleneck_nhwc_x(one, one, one, one, one, one, one, one, one, one, None, 1, 64, 32, 256, 64, None, None) == -1
    assert b"next-conv" in L.ssg_last_error()
    # the slot is empty again: B = 0 fails with the plain message
    assert L.ssg_bottleneck_nhwc_x(one, one, one, one, one, one, one, one, one, one, two, 0, 64, 32, 256, 64, None, None) == -1
    assert b"unsupported block" in L.ssg_last_error()


def test_env_switch_parses(L, monkeypatch):
    monkeypatch.delenv("SSG_BN_L1_NEXT", raising=False)
    default = L.ssg_bottleneck_next_enabled()
    assert default in (0, 1)
    monkeypatch.setenv("SSG_BN_L1_NEXT", "")
    assert L.ssg_bottleneck_next_enabled() == default
    monkeypatch.setenv("SSG_BN_L1_NEXT", "0")
    assert L.ssg_bottleneck_next_enabled() == 0
    monkeypatch.setenv("SSG_BN_L1_NEXT", "1")
    assert L.ssg_bottleneck_next_enabled() == 1
    for bad in ("2", "yes", "01", "-1", " 1"):
        monkeypatch.setenv("SSG_BN_L1_NEXT", bad)
        assert L.ssg_bottleneck_next_enabled() == -1, bad
        assert b"SSG_BN_L1_NEXT" in L.ssg_last_error()
