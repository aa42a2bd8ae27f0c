"""GPU suite (-m gpu): the raw output bytes of every kernel with a split-half epilogue, on seeded inputs at batch 3, against SHA-256
digests recorded with the library as it was before the epilogues moved to the shared codec of csrc/ssg_common.h
(tests/golden/epilogue_digests.json).  The kernel-against-kernel equality tests of the suite cannot see a change that all kernels
make together; this one can.  Covered:

  stem           ssg_stem_pool_nchw_x, plain and flipped
  r50_blocks     every fused launch of the resnet50 forward in order: layer1 with downsample, layer1 plain, layer1 next-conv
                 (y1n and out_s2), the layer2 channel-halves blocks
  r18_blocks     every fused BasicBlock launch of the resnet18 forward
  *_fmap/pooled  the layer4 map (h8l8 containers, through the unfused convolutions of layers 2-4) and the un-normalised pooled
                 features of both orientations, i.e. all embed_with_flip computes before its final normalisation

`python tests/test_gpu_epilogue_digests.py --record` rewrites the file from the library in use (SSG_LIB_PATH selects another build).
"""
import hashlib
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epilogue_digests.json")
B, H, W = 3, 256, 128


def _sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _forward(name, imgs, flip, out, tag):
    """one forward with every fused-block launch's result hashed in order"""
    import ssg_amd
    from ssg_amd.resnet import ResNet
    model = ssg_amd.create(name, num_classes=0, num_split=1, cluster=False, seed=1).cuda().eval()
    seen = []
    real_bn, real_bb = ResNet._bottleneck, ResNet._basicblock

    def spy(real):
        def f(*a, **kw):
            r = real(*a, **kw)
            if r is not None:
                seen.extend(_sha(t) for t in (r if isinstance(r, tuple) else (r,)))
            return r
        return staticmethod(f)
    ResNet._bottleneck, ResNet._basicblock = spy(real_bn), spy(real_bb)
    try:
        y, sp = model._fmap(imgs, flip=flip)
    finally:
        ResNet._bottleneck, ResNet._basicblock = staticmethod(real_bn), staticmethod(real_bb)
    assert sp and not model._overflowed()
    out[tag + "_blocks"] = seen
    out[tag + "_fmap"] = _sha(y)
    out[tag + "_pooled"] = _sha(model.pooled(y, sp))
    return model


def compute():
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr, stream
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    L = _lib.lib()
    imgs = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(17)).cuda()
    d = {}
    model = _forward("resnet50", imgs, False, d, "r50")
    _forward("resnet50", imgs, True, d, "r50_flip")
    _forward("resnet18", imgs, False, d, "r18")
    st = model._prepare()["stem"]
    flag = torch.zeros(1, dtype=torch.int32, device=imgs.device)
    for flip in (0, 1):
        y = torch.empty((B, H // 4, W // 4, 64), dtype=torch.float32, device=imgs.device)
        check(L.ssg_stem_pool_nchw_x(ptr(imgs), flip, ptr(st.w), ptr(st.bias), ptr(st.cscale), ptr(y), B, H, W, ptr(flag), stream()), "stem")
        d["stem_flip" if flip else "stem"] = _sha(y)
    assert int(flag.item()) == 0
    return d


@pytest.fixture(scope="module")
def got():
    return compute()


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


def test_launch_counts(got):
    """the forward took the fused routes this test is about: 3 layer1 launches (the last one hands over y1n and out_s2: 4 tensors)
    and 3 layer2 launches for resnet50, and fused BasicBlocks for resnet18"""
    assert len(got["r50_blocks"]) == 7 and len(got["r50_flip_blocks"]) == 7, got["r50_blocks"]
    assert len(got["r18_blocks"]) >= 1


@pytest.mark.parametrize("key", ["stem", "stem_flip", "r50_blocks", "r50_flip_blocks", "r18_blocks", "r50_fmap", "r50_flip_fmap", "r18_fmap",
                                 "r50_pooled", "r50_flip_pooled", "r18_pooled"])
def test_digest(key, got, want):
    assert got[key] == want[key]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = compute()
    if "--record" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))
