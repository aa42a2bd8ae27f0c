"""The tiled weight copies of the LDS-DMA convolution launches (ssg_conv_weights_tile, ssg_conv2d_nhwc_xt, ssg_conv1x1_dual_nhwc_xt):
the layout against a numpy restatement, every kernel instance with the copy against the same call without it (same bits, same range
flag), and the embedder with `tiled_weights` on and off."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ssg_amd
from ssg_amd import _lib
from ssg_amd._lib import ptr, stream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_tiled_child as child  # noqa: E402


def tile_ref(w):
    """[Cout][Kpad] 4-byte containers -> [Cout/128][Kpad/16][128 rows][4 slots][4]: granules of 128 rows x one 16-container k-tile, slot pc
    of row r holding the row's 16-byte chunk pc ^ ((r >> 2) & 3) of that k-tile"""
    cout, kp = w.shape
    t = w.reshape(cout // 128, 128, kp // 16, 4, 4).transpose(0, 2, 1, 3, 4)
    out = np.empty_like(t)
    for r in range(128):
        for pc in range(4):
            out[:, :, r, pc] = t[:, :, r, pc ^ ((r >> 2) & 3)]
    return out.reshape(cout, kp)


@pytest.mark.parametrize("cout,kp", [(256, 144), (128, 2304)])
def test_tile_layout_matches_the_restatement(cout, kp):
    L = _lib.lib()
    w = np.random.default_rng(cout + kp).integers(0, 2 ** 32, (cout, kp), dtype=np.uint32)
    wd = torch.from_numpy(w.view(np.int32)).cuda()
    wt = torch.zeros_like(wd)
    assert L.ssg_conv_weights_tile_supported(cout, kp) == 1
    assert L.ssg_conv_weights_tile(ptr(wd), cout, kp, ptr(wt), stream()) == 1
    assert np.array_equal(wt.cpu().numpy().view(np.uint32), tile_ref(w))


def test_shapes_without_a_tiled_form_are_left_alone():
    L = _lib.lib()
    wd = torch.ones((64, 256), dtype=torch.int32, device="cuda")
    wt = torch.full_like(wd, 7)
    assert L.ssg_conv_weights_tile_supported(64, 256) == 0 and L.ssg_conv_weights_tile_supported(128, 40) == 0
    assert L.ssg_conv_weights_tile(ptr(wd), 64, 256, ptr(wt), stream()) == 0
    assert bool((wt == 7).all())
    # a launch that is handed a copy for such a shape is refused, not quietly run on the row-major weights
    assert L.ssg_conv2d_nhwc_xt(None, ptr(wd), ptr(wt), None, None, None, 2, 8, 8, 256, 64, 1, 1, 1, 0, 1, 3, 1.0, None, None, None) == -1
    assert b"tiled weights" in L.ssg_last_error()
    assert L.ssg_conv1x1_dual_nhwc_xt(None, None, ptr(wd), ptr(wt), None, None, 2, 4, 4, 128, 8, 8, 128, 2, 64, 1, 3, 1.0, None, None, None) == -1


# routing knobs of csrc/conv.hip (cached per process, hence the child): every launch on the LDS-DMA kernel whatever its tile count --
# "wide": 128 x 256 tiles where Cout % 256 == 0 and K >= 128 (with and without residual, DUAL), 128 x 128 tiles otherwise;
# "tall": the 256 x 256 four-stage instance for the same launches (residual and DUAL included), 128 x 128 for the others
_ENV = {"wide": {"SSG_SPLIT_WIDE_MINTILES": "1", "SSG_SPLIT_BN64_MAXTILES": "0", "SSG_CONV_TALL_MINTILES": "0"},
        "tall": {"SSG_SPLIT_WIDE_MINTILES": "1", "SSG_SPLIT_BN64_MAXTILES": "0", "SSG_CONV_TALL_MINTILES": "1", "SSG_CONV_TALL_RES": "1",
                 "SSG_CONV_TALL_DUAL": "1"}}
_RESULTS = {}


def _child(config):
    if config not in _RESULTS:
        env = dict(os.environ, **_ENV[config])
        env.pop("SSG_CONV_DMA", None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "conv_tiled_child.py")], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        _RESULTS[config] = json.loads(r.stdout.strip().splitlines()[-1])
    return _RESULTS[config]


@pytest.mark.parametrize("case", sorted(child.CASES))
@pytest.mark.parametrize("config", sorted(_ENV))
def test_tiled_launch_equals_the_row_major_launch(config, case):
    got = _child(config)[case]
    print(config, case, got)
    assert got["nonzero"], "the launch wrote nothing"
    assert got["out"], "output bits differ between wt and wt = NULL"
    assert got["flag"], "range flag differs between wt and wt = NULL"
    assert got["flag_value"] == (1 if case.endswith("out_of_range") else 0)


def test_embedder_with_and_without_tiled_weights():
    model = ssg_amd.create("resnet50", num_classes=0, num_split=1, cluster=False, seed=1, pretrained=False).cuda().eval()
    imgs = torch.randn(8, 3, 256, 128, generator=torch.Generator().manual_seed(5))
    assert model.tiled_weights is (os.environ.get("SSG_CONV_WT", "1") != "0")

    def both():
        model.tiled_weights = True
        on = model.embed_with_flip(imgs)
        model.tiled_weights = False
        off = model.embed_with_flip(imgs)
        assert torch.equal(on.view(torch.int32), off.view(torch.int32))
        return on

    first = both()
    blocks = model._prepare()["blocks"]
    l3 = blocks[3 + 4 + 1]                                          # an identity block of layer3
    for f in (l3["c1"], l3["c2"], l3["c3"], blocks[3 + 4]["ds"]):
        assert f.wt is not None and f.wt.data_ptr() == f.w.data_ptr() + 4 * f.w.numel()
    assert model._prepare()["stem"].wt is None
    model.refresh(ssg_amd.synthetic_state_dict(seed=2))
    second = both()
    assert not torch.equal(first, second)
    assert model._prepare()["blocks"][3 + 4 + 1]["c2"].wt is not None
