"""GPU suite (-m gpu): the whole embedder at the batch sizes it is used at -- 250 (tests/test_gpu_chain.py), 1000 (bench.py) and 1023,
the largest batch of 256 x 128 images the library admits (layer1's output, 2 MiB per image, has to stay inside the 2 GiB
buffer-resource range of the convolution that reads it) -- next to the handful of images the reference goldens vouch for.

A forward at batch 1000 takes other kernels for most layers than one at batch 16 (256 x 256 and 128 x 256 tiles, other
workgroup-to-tile assignments, byte offsets up to 2^31); every one of those choices claims to be bit-invariant, so
  1. the layer4 map of a batch equals the maps of the same images four at a time, on the int32 view, every image, both orientations;
  2. the features of the images tests/embed_batch_ref.sample_union picks agree with the float64 restatement (oracle/embed_oracle.py,
     pinned against the reference model's goldens by tests/test_embed_oracle.py) inside the 5e-6 every golden test uses;
  3. two streams give the one-stream features at batch 1000, and no activation leaves the half range;
  4. an extraction of 2 300 images in batches of 1000, 1000 and 300 returns the bits of the four-at-a-time features, row for row.
Every case prints one `embed-batch-error` line (pytest -s); profiles/fused_block_errors.txt holds such a log.
"""
import warnings

import pytest

import embed_batch_ref as ebr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_ALL = 2300
_REF = {}            # image index -> float64 features [3, 2048] (shared by every batch size and both precisions)
_MODELS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    from ssg_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def sd():
    from synth import checkpoint_like_state_dict
    return checkpoint_like_state_dict(7)


@pytest.fixture(scope="module")
def images(dev):
    """2 300 images that carry identities (a random 3 x 16 x 8 pattern per identity, upsampled x 16, plus pixel noise), generated on
    the device: nothing large crosses PCIe.  Batch B is the first B of them."""
    g = torch.Generator(device=dev).manual_seed(29)
    pat = torch.randn(97, 3, 16, 8, generator=g, device=dev)
    base = pat[torch.arange(N_ALL, device=dev) % 97].repeat_interleave(16, dim=2).repeat_interleave(16, dim=3)
    return base + 0.35 * torch.randn(N_ALL, 3, 256, 128, generator=g, device=dev)


def _model(precision, sd):
    import ssg_amd
    if precision not in _MODELS:
        m = ssg_amd.create("resnet50", num_split=2, pretrained=False, precision=precision).cuda().eval()
        m.load_state_dict(sd, strict=False)
        _MODELS[precision] = m
    return _MODELS[precision]


def _reference_rows(sd, images, idx):
    """float64 features [3, len(idx), 2048] of the images `idx`"""
    from oracle import embed_oracle
    todo = [i for i in idx if i not in _REF]
    for lo in range(0, len(todo), 8):
        part = todo[lo:lo + 8]
        f = torch.stack(embed_oracle.embed_with_flip(sd, images[torch.tensor(part, device=images.device)].cpu(), 2, dtype=torch.float64))
        for k, i in enumerate(part):
            _REF[i] = f[:, k].clone()
    return torch.stack([_REF[i] for i in idx], dim=1)


def _check_batch(m, sd, images, B):
    imgs = images[:B]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # no overflow fallback may be needed here
        # 1. layer4 map: the batch against the same images four at a time
        for flip in (False, True):
            big, sp = m._fmap(imgs, flip=flip)
            assert sp == (m.precision == "split") and big.shape == (B, 8, 4, 2048)
            small = torch.cat([m._fmap(imgs[lo:lo + 4], flip=flip)[0] for lo in range(0, B, 4)], 0)
            same = (big.view(torch.int32) == small.view(torch.int32)).flatten(1).all(dim=1)
            bad = (~same).nonzero().flatten().tolist()
            assert not bad, "B=%d %s flip=%s: %d images differ from the four-at-a-time maps, first %r" % (B, m.precision, flip, len(bad), bad[:8])
            del big, small
        assert not m._overflowed()
        # 2. features of the sampled images against float64
        idx = ebr.sample_union(B, ebr.EMBED_TILES, ebr.EMBED_IMAGE_BYTES)
        got = m.embed_with_flip(imgs)
        assert got.shape == (3, B, 2048) and bool(torch.isfinite(got).all())
        ref = _reference_rows(sd, images, idx)
        err = float((got[:, torch.tensor(idx, device=got.device)].cpu().double() - ref).abs().max())
    print("embed-batch-error: B=%4d precision=%-5s images %2d  max|features - float64| %.3e  (bound 5e-6)" % (B, m.precision, len(idx), err))
    assert err < 5e-6, (B, m.precision, err)
    return got


@pytest.mark.parametrize("B", ebr.EMBED_BATCHES)
def test_split_embedder_at_batch(B, sd, images):
    _check_batch(_model("split", sd), sd, images, B)


@pytest.mark.parametrize("B", [250, 1000])
def test_f32_embedder_at_batch(B, sd, images):
    _check_batch(_model("f32", sd), sd, images, B)


def test_two_streams_equal_one_stream_at_batch_1000(sd, images):
    m = _model("split", sd)
    imgs = images[:1000]
    keep = m.flip_streams
    try:
        m.flip_streams = False
        one = m.embed_with_flip(imgs)
        m.flip_streams = True
        two = m.embed_with_flip(imgs)
    finally:
        m.flip_streams = keep
    assert torch.equal(one.view(torch.int32), two.view(torch.int32))
    assert not m._overflowed()


def test_extraction_in_batches_of_1000_returns_the_small_batch_bits(sd, images):
    import ssg_amd
    m = _model("split", sd)
    small = torch.cat([m.embed_with_flip(images[lo:lo + 4]) for lo in range(0, N_ALL, 4)], dim=1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        feats, names, _ = ssg_amd.extract_embeddings(m, ssg_amd.TensorBatchLoader(images, 1000), for_eval=False)
    assert feats.shape == small.shape == (3, N_ALL, 2048) and len(names) == N_ALL
    same = (feats.view(torch.int32) == small.view(torch.int32)).all(dim=2).all(dim=0)
    bad = (~same).nonzero().flatten().tolist()
    assert not bad, "%d rows differ from the four-at-a-time features, first %r" % (len(bad), bad[:8])
    assert not m._overflowed()
