"""Which images of a large embedding batch the GPU tests compare with the float64 reference (TEST INFRASTRUCTURE ONLY).

A fused kernel that is wrong only for some workgroup index, image index or byte offset is wrong for SOME images of a large batch;
a float64 reference of every image of a 1 000-image batch costs minutes of CPU time.  `sample_images` is the pure function that
picks the images where such a mistake would show, and tests/test_embed_batch_host.py proves on the CPU that it returns them.

`xcd_tile` restates (it does not import) the tile assignment of csrc/bottleneck.hip: workgroups are dealt round-robin to the 8
XCDs, and workgroup b = 8 s + x takes tile s of the contiguous run of XCD x; with ntiles = 8 q + r the first r runs hold q + 1
tiles and the others q.
"""
import random

XCDS = 8
CAP = 48                 # most images any case compares with float64; B <= CAP: every image
RANDOM_DRAWS = 8


def xcd_tile(block, ntiles):
    """tile that workgroup `block` of an `ntiles`-workgroup launch computes"""
    q, r = divmod(ntiles, XCDS)
    x, s = block % XCDS, block // XCDS
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + s


def xcd_runs(ntiles):
    """[(first tile, last tile)] of every non-empty XCD run, in XCD order"""
    q, r = divmod(ntiles, XCDS)
    runs, t = [], 0
    for x in range(XCDS):
        n = q + 1 if x < r else q
        if n:
            runs.append((t, t + n - 1))
        t += n
    return runs


def offset_neighbours(B, image_bytes):
    """images on both sides of the points where the byte offset into a [B, ...] tensor of `image_bytes` per image crosses 2^30 and
    2^31: the last image that lies wholly below the bound and the image that holds (or starts at) that byte"""
    out = []
    if image_bytes > 0:
        for bound in (1 << 30, 1 << 31):
            k = bound // image_bytes
            out += [i for i in (k - 1, k) if 0 <= i < B]
    return out


def sample_images(B, tiles_img, image_bytes=0):
    """sorted image indices of a B-image launch with `tiles_img` tiles (workgroups) per image, `image_bytes` bytes per image in the
    launch's largest tensor: every image when B <= 48, else the batch ends (0, 1, B-2, B-1), the images of the first and the last
    tile of each XCD run, the 2^30 / 2^31 byte-offset neighbours and 8 images drawn from a generator seeded by (B, tiles_img)."""
    if B <= CAP:
        return list(range(B))
    pick = {0, 1, B - 2, B - 1}
    for first, last in xcd_runs(B * tiles_img):
        pick.add(first // tiles_img); pick.add(last // tiles_img)
    pick.update(offset_neighbours(B, image_bytes))
    pick.update(random.Random(1000003 * B + tiles_img).sample(range(B), RANDOM_DRAWS))
    out = sorted(pick)
    assert len(out) <= CAP and all(0 <= i < B for i in out)
    return out


def sample_union(B, tiles_list, image_bytes=0):
    """union of the samples for several kernels that run on the same batch (layer1: 16 tiles per image, layer2: 4)"""
    if B <= CAP:
        return list(range(B))
    return sorted(set().union(*[sample_images(B, t, image_bytes) for t in tiles_list]))


# ---- the cases of tests/test_gpu_fused_blocks.py and tests/test_gpu_embed_batch.py (shared with the host test of the sampler)
STEM_STRIP = 16          # pooled rows per workgroup of csrc/stem_pool.hip (its default)
# (H, B): one strip (8, 12, 64) / ragged last strip (100, 104) / four strips (256) / more than four, the last one a single row (260)
STEM_CASES = [(H, B) for H in (8, 12, 64, 100, 104, 256, 260) for B in (1, 3, 250)] + [(256, 1000)]
# (C, MID, CIN, H, W, B): layer1 identity (CIN 256) and downsample (CIN 64) blocks, 4-row tiles; layer2 identity blocks, 8-row tiles
BNECK_CASES = ([(256, 64, cin, 12, 32, B) for cin in (256, 64) for B in (1, 3, 5, 7)]          # ntiles 3, 9, 15, 21: r = 3, 1, 7, 5 at q = 0..2
               + [(256, 64, cin, 24, 32, B) for cin in (256, 64) for B in (1, 2, 3)]           # ntiles 6, 12, 18: r = 6, 4, 2
               + [(256, 64, cin, 64, 32, B) for cin in (256, 64) for B in (1, 250, 1000)]      # r = 0: the benchmark's shape and batch
               + [(512, 128, 512, H, 16, B) for H in (8, 32) for B in (1, 3, 5, 7, 251, 1000)])  # ntiles = B: r = 1, 3, 5, 7 at q = 0; 4 B: r = 4; odd B at size
EMBED_BATCHES = (1, 2, 5, 13, 64, 250, 1000, 1023)
EMBED_TILES = (16, 4)                                   # layer1 / layer2 tiles per 256 x 128 image
EMBED_IMAGE_BYTES = 64 * 32 * 256 * 4                   # the forward's largest tensor: layer1's output, 2 MiB per image


def stem_strips(H):
    return (H // 4 + STEM_STRIP - 1) // STEM_STRIP


def bneck_tiles_img(C, H):
    return H // (4 if C == 256 else 8)


def sampler_cases():
    """every (B, tiles_img, image_bytes) the GPU tests call sample_images with"""
    out = [(B, stem_strips(H), (H // 4) * 32 * 64 * 4) for H, B in STEM_CASES]
    out += [(B, bneck_tiles_img(C, H), H * W * C * 4) for C, MID, CIN, H, W, B in BNECK_CASES]
    out += [(B, t, EMBED_IMAGE_BYTES) for B in EMBED_BATCHES for t in EMBED_TILES]
    return sorted(set(out))
