"""The fetch order of conv_dma_kernel's pixel operand (csrc/conv.hip, template parameter LINE, knob SSG_CONV_LINE): with the two 64-byte
halves of a 128-byte line requested back to back (1) every launch must give the bits and the range flag of the k-tile order (0) -- on
every LDS-DMA instance (the "wide" and "tall" routing of test_conv_tiled_weights.py) -- and of the register-staged kernel; the embedder
must not depend on the knob either, before and after refresh().  The knobs are cached per process: one child per configuration."""
import json
import os
import subprocess
import sys

import pytest
import torch

from ssg_amd import _lib
from ssg_amd._lib import ptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_line_child as child  # noqa: E402

_WIDE = {"SSG_SPLIT_WIDE_MINTILES": "1", "SSG_SPLIT_BN64_MAXTILES": "0", "SSG_CONV_TALL_MINTILES": "0"}
_TALL = {"SSG_SPLIT_WIDE_MINTILES": "1", "SSG_SPLIT_BN64_MAXTILES": "0", "SSG_CONV_TALL_MINTILES": "1", "SSG_CONV_TALL_RES": "1", "SSG_CONV_TALL_DUAL": "1"}
ORDERS = ("1",)                                       # every line order the build has (SSG_CONV_LINE values besides 0)
_RESULTS = {}


def _child(mode, routing, line, dma=None):
    key = (mode, routing, line, dma)
    if key not in _RESULTS:
        env = dict(os.environ, **{"wide": _WIDE, "tall": _TALL, "default": {}}[routing])
        for k in ("SSG_CONV_DMA", "SSG_CONV_LINE"):
            env.pop(k, None)
        if line is not None:
            env["SSG_CONV_LINE"] = line
        if dma is not None:
            env["SSG_CONV_DMA"] = dma
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "conv_line_child.py"), mode], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        _RESULTS[key] = json.loads(r.stdout.strip().splitlines()[-1])
    return _RESULTS[key]


@pytest.mark.parametrize("case", sorted(child.CASES))
@pytest.mark.parametrize("line", ORDERS)
@pytest.mark.parametrize("routing", ["wide", "tall"])
def test_line_order_equals_the_ktile_order(routing, line, case):
    ref, got = _child("kernels", routing, "0")[case], _child("kernels", routing, line)[case]
    print(routing, line, case, ref, got)
    assert ref["nonzero"] and got["nonzero"], "the launch wrote nothing"
    assert got["sha"] == ref["sha"], "output bits differ between SSG_CONV_LINE=%s and 0" % line
    assert got["flag"] == ref["flag"] == (1 if case.endswith("out_of_range") else 0)


@pytest.mark.parametrize("case", sorted(child.CASES))
def test_line_order_equals_the_register_staged_kernel(case):
    ref, got = _child("kernels", "wide", None, dma="0")[case], _child("kernels", "wide", ORDERS[0])[case]
    print(case, ref, got)
    assert got["sha"] == ref["sha"] and got["flag"] == ref["flag"]


def test_odd_ktile_count_is_refused_by_the_entry_points():
    """Kpad / 16 odd needs Cin % 32 == 16: neither convolution entry point accepts such a shape (nothing is launched), so the line order
    never meets an odd k-tile count there; conv_route checks the parity all the same."""
    L = _lib.lib()
    w = torch.ones((256, 48), dtype=torch.int32, device="cuda")
    assert L.ssg_conv2d_nhwc_xt(None, ptr(w), None, None, None, None, 3, 16, 8, 48, 256, 1, 1, 1, 0, 1, 3, 1.0, None, None, None) == -1
    assert b"unsupported shape" in L.ssg_last_error()
    assert L.ssg_conv1x1_dual_nhwc_xt(None, None, ptr(w), None, None, None, 3, 16, 8, 32, 32, 16, 16, 2, 256, 1, 3, 1.0, None, None, None) == -1
    assert b"unsupported shape" in L.ssg_last_error()


@pytest.mark.parametrize("when", ["before", "after"])
@pytest.mark.parametrize("line", ORDERS)
def test_embedder_does_not_depend_on_the_order(line, when):
    ref, got = _child("embed", "default", "0")[when], _child("embed", "default", line)[when]
    assert ref["finite"] and got["finite"]
    assert got["sha"] == ref["sha"], "features differ between SSG_CONV_LINE=%s and 0 (%s refresh)" % (line, when)
    assert _child("embed", "default", "0")["before"]["sha"] != _child("embed", "default", "0")["after"]["sha"]
