"""CPU suite: the image sampler of the large-batch embedder tests (tests/embed_batch_ref.py) returns every image class the GPU
tests promise to compare with float64, for every case they run, and the restated XCD tile assignment is a permutation."""
import pytest

import embed_batch_ref as ebr


@pytest.mark.parametrize("ntiles", sorted({B * t for B, t, _ in ebr.sampler_cases()} | set(range(1, 40))))
def test_restated_tile_assignment_is_a_permutation_of_contiguous_runs(ntiles):
    tiles = [ebr.xcd_tile(b, ntiles) for b in range(ntiles)]
    assert sorted(tiles) == list(range(ntiles))
    runs = ebr.xcd_runs(ntiles)
    q, r = divmod(ntiles, 8)
    assert len(runs) == min(ntiles, 8) and runs[0][0] == 0 and runs[-1][1] == ntiles - 1
    assert all(b[0] == a[1] + 1 for a, b in zip(runs, runs[1:]))
    assert [hi - lo + 1 for lo, hi in runs] == [q + 1] * r + [q] * (8 - r if q else 0)
    for x, (lo, hi) in enumerate(runs):          # XCD x walks its run in order: workgroups x, x + 8, x + 16, ...
        assert [ebr.xcd_tile(x + 8 * s, ntiles) for s in range(hi - lo + 1)] == list(range(lo, hi + 1))


def test_cases_cover_what_the_small_batches_never_reach():
    """the remainders r = ntiles % 8 and the q = 0 launches the fused-block cases were chosen for"""
    r256 = {(B * ebr.bneck_tiles_img(C, H)) % 8 for C, _, _, H, _, B in ebr.BNECK_CASES if C == 256}
    r512 = {(B * ebr.bneck_tiles_img(C, H)) % 8 for C, _, _, H, _, B in ebr.BNECK_CASES if C == 512}
    assert r256 == set(range(8)) and r512 == {0, 1, 3, 4, 5, 7}      # (layer2: one tile per 8-row image gives the odd ones)
    q0 = {B * ebr.bneck_tiles_img(C, H) for C, _, _, H, _, B in ebr.BNECK_CASES if B * ebr.bneck_tiles_img(C, H) < 8}
    assert {1, 3, 5, 7} <= q0 and {3, 6} <= q0
    assert {ebr.stem_strips(H) for H, _ in ebr.STEM_CASES} == {1, 2, 4, 5}
    assert (1000, 16, ebr.EMBED_IMAGE_BYTES) in ebr.sampler_cases() and (1023, 4, ebr.EMBED_IMAGE_BYTES) in ebr.sampler_cases()


@pytest.mark.parametrize("B,tiles_img,image_bytes", ebr.sampler_cases())
def test_sampler_returns_every_promised_image(B, tiles_img, image_bytes):
    got = ebr.sample_images(B, tiles_img, image_bytes)
    assert got == sorted(set(got)) and all(0 <= i < B for i in got) and len(got) <= 48
    assert got == ebr.sample_images(B, tiles_img, image_bytes)          # pure
    if B <= 48:
        assert got == list(range(B))
        return
    have = set(got)
    assert {0, 1, B - 2, B - 1} <= have
    # first and last tile of every non-empty XCD run, from the workgroup enumeration itself (not from xcd_runs)
    ntiles = B * tiles_img
    for x in range(min(8, ntiles)):
        mine = [ebr.xcd_tile(b, ntiles) for b in range(x, ntiles, 8)]
        assert mine[0] // tiles_img in have and mine[-1] // tiles_img in have, (x, mine[0], mine[-1])
    # byte-offset neighbours: image i covers bytes [i * image_bytes, (i + 1) * image_bytes)
    for bound in (1 << 30, 1 << 31):
        for i in range(B):
            below_last = (i + 1) * image_bytes <= bound < (i + 2) * image_bytes      # the last image wholly below the bound
            holds = i * image_bytes <= bound < (i + 1) * image_bytes                 # the image the byte `bound` belongs to
            if below_last or holds:
                assert i in have, (bound, i)
    assert len(have) >= 12          # the seeded draw and the run ends are really there (8 distinct draws alone)


def test_offset_neighbours_at_the_benchmark_shape():
    """2 MiB per image (layer1's output at 256 x 128): 2^30 falls between images 511 and 512, 2^31 behind image 1023"""
    assert ebr.offset_neighbours(1000, ebr.EMBED_IMAGE_BYTES) == [511, 512]
    assert ebr.offset_neighbours(512, ebr.EMBED_IMAGE_BYTES) == [511]
    assert ebr.offset_neighbours(1023, ebr.EMBED_IMAGE_BYTES) == [511, 512] and ebr.offset_neighbours(250, ebr.EMBED_IMAGE_BYTES) == []
    assert {511, 512} <= set(ebr.sample_images(1000, 16, ebr.EMBED_IMAGE_BYTES))
    assert 1023 * ebr.EMBED_IMAGE_BYTES <= 0x7fffffff < 1024 * ebr.EMBED_IMAGE_BYTES      # 1023: the largest batch the library admits
    u = ebr.sample_union(1000, ebr.EMBED_TILES, ebr.EMBED_IMAGE_BYTES)
    assert set(ebr.sample_images(1000, 16, ebr.EMBED_IMAGE_BYTES)) | set(ebr.sample_images(1000, 4, ebr.EMBED_IMAGE_BYTES)) == set(u)


def test_batch_1024_is_refused_by_the_argument_checks():
    """256 x 128 images: layer1's output is 2 MiB per image and the first convolution of layer2 reads it through a 2 GiB buffer
    resource, so 1023 images is the largest batch; 1024 is refused by the entry points' argument checks, which return before any
    launch (no pointer is touched: this runs without a GPU, like tests/test_abi.py)."""
    from ssg_amd import _lib
    L = _lib.lib()
    # layer2.0 conv1 (1x1, 256 -> 128) on [1024, 64, 32, 256]
    assert L.ssg_conv2d_nhwc_x(None, None, None, None, None, 1024, 64, 32, 256, 128, 1, 1, 1, 0, 1, 3, 1.0, None, None, None) == -1
    assert b"2 GiB" in L.ssg_last_error() and b"smaller batch" in L.ssg_last_error()
    with pytest.raises(ValueError, match="2 GiB buffer-resource range"):
        _lib.check(-1, "ssg_conv2d_nhwc_x")
    # layer2.0 conv3 | downsample: the second input is the same tensor
    assert L.ssg_conv1x1_dual_nhwc_x(None, None, None, None, None, 1024, 32, 16, 128, 64, 32, 256, 2, 512, 1, 3, 1.0, None, None, None) == -1
