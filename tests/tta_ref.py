"""Yardstick of the test-time extraction tests (tests/test_tta_host.py, tests/test_gpu_tta.py) and of tools/make_golden_tta.py: seeded
cases and plain numpy / Pillow restatements of what reid/extract_feature.py computes around the model.

TenCrop.  torchvision is not a dependency; its transform is restated from its documented formulas (torchvision.transforms.functional):
    center_crop(img, (ch, cw)):  crop_top  = int(round((image_height - crop_height) / 2.0))
                                 crop_left = int(round((image_width  - crop_width)  / 2.0))
    five_crop(img, size)      :  tl = crop(img, 0, 0, ch, cw); tr = crop(img, 0, w - cw, ch, cw); bl = crop(img, h - ch, 0, ch, cw);
                                 br = crop(img, h - ch, w - cw, ch, cw); center = center_crop(img, (ch, cw))   -> (tl, tr, bl, br, center)
    ten_crop(img, size)       :  five_crop(img, size) + five_crop(hflip(img), size)
`round` is Python's: halves go to the even neighbour (4.5 -> 4, 3.5 -> 4).  Crop 5 + k is therefore the window k of the MIRRORED
image, which is the mirror of the window (top_k, W - cw - left_k) of the image itself.  For the four corners that is the mirror of
crop (1, 0, 3, 2)[k]; for the centre it is the mirror of the centre crop only when W - cw is even (with an odd margin the two windows
lie one pixel apart).

Mean over the crops.  torch's CPU `x.view(bs, n, -1).mean(1)` on a float32 tensor = the ascending sequential float32 sum over the n
rows, divided by n in float32 (`sequential_mean`) -- in the columns its sum kernel takes a block of SIMD vectors at a time.  The
columns behind the last whole block (D % 32 of them in the build that wrote the fixture: `mean_tail`) go through its scalar loop, which
keeps four interleaved partial sums (`torch_mean`; ATen/native/cpu/SumKernel.cpp, row_sum with ilp_factor 4).
tests/golden/tta_multiquery_cases.npz pins torch's own result.

Multi-query pooling.  `normalize64` is the float64 value t of sklearn.preprocessing.normalize (the sum of squares exactly rounded with
math.fsum, so that every machine gets the same t); the fixture keeps sklearn's float32 result and numpy's max / mean of it as small
integer distances, in float32 steps, from float32(t) -- `unpack_steps` rebuilds the recorded arrays exactly.  The recorded arrays
are sklearn's and numpy's results on float32 2-D arrays.  (The script hands `normalize` a Python list of float32 rows, which
scikit-learn 1.7.2 converts to float64: there the three results are float64 and equal t to a few units of 2^-53.)
"""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tta_multiquery_cases.npz")
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
FLIP_OF = (1, 0, 3, 2, 4)

# name -> (B, source h, w, resize (RH, RW), crop (CH, CW), seed); "full": the fixture stores every crop as float32 (small geometries),
# else Pillow's resized uint8 image
GEOMETRIES = {
    "market": (3, 128, 64, (288, 144), (256, 128), 901),        # Market-1501's own size: an up-scale
    "down": (2, 400, 180, (288, 144), (256, 128), 902),         # a down-scale: filter windows longer than 3
    "odd9": (2, 37, 23, (41, 25), (32, 16), 903),               # margins (9, 9): centre 4.5 -> 4
    "odd7": (2, 19, 11, (23, 15), (16, 8), 904),                # margins (7, 7): centre 3.5 -> 4
    "same": (2, 29, 17, (24, 16), (24, 16), 905),               # resize == crop: the ten windows coincide, five are mirrored
}
FULL = ("odd9", "odd7", "same")

MEAN_CASES = {"d2048": (3, 10, 2048, 911), "d70": (3, 10, 70, 912)}           # name -> (B, n, D, seed)

# name -> (M, D, seed); the membership below is shared: groups of 1, 2, 7 and 13 rows, interleaved
POOL_CASES = {"d2048": (23, 2048, 921), "d70": (23, 70, 922)}
POOL_ZERO_ROW = 11


def centre_offset(full, crop):
    return int(round((full - crop) / 2.0))


def crop_boxes(RH, RW, CH, CW):
    """(top, left) of tl, tr, bl, br, centre"""
    return [(0, 0), (0, RW - CW), (RH - CH, 0), (RH - CH, RW - CW), (centre_offset(RH, CH), centre_offset(RW, CW))]


def source_images(name):
    """uint8 [B, h, w, 3]: random 8 x 8 blocks, one pixel in sixteen lifted by a random amount (flat enough for the fixture's resized
    images to compress, with edges and single pixels for the filters to smear)"""
    B, h, w, _, _, seed = GEOMETRIES[name]
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 200, size=(B, (h + 7) // 8, (w + 7) // 8, 3))
    img = np.repeat(np.repeat(blocks, 8, axis=1), 8, axis=2)[:, :h, :w]
    noise = rng.integers(0, 56, size=(B, h, w, 3)) * (rng.integers(0, 16, size=(B, h, w, 1)) == 0)
    return (img + noise).astype(np.uint8)


def pil_resize(img_u8, size):
    """Resize((RH, RW)) of one image -> uint8 [RH, RW, 3]"""
    from PIL import Image
    RH, RW = size
    return np.asarray(Image.fromarray(img_u8).resize((RW, RH), Image.BILINEAR))


def ten_crop_pil(img_u8, size):
    """the ten crops of one (resized) image with Pillow's own crop and transpose -> uint8 [10, CH, CW, 3]"""
    from PIL import Image
    CH, CW = size
    out = []
    img = Image.fromarray(img_u8)
    for im in (img, img.transpose(Image.FLIP_LEFT_RIGHT)):
        W, H = im.size
        for top, left in crop_boxes(H, W, CH, CW):
            out.append(np.asarray(im.crop((left, top, left + CW, top + CH))))
    return np.stack(out)


def ten_crop_u8(img_u8, size):
    """the same with numpy slices -> uint8 [10, CH, CW, 3]"""
    CH, CW = size
    H, W = img_u8.shape[:2]
    out = []
    for im in (img_u8, img_u8[:, ::-1]):
        for top, left in crop_boxes(H, W, CH, CW):
            out.append(im[top:top + CH, left:left + CW])
    return np.stack(out)


def to_tensor_normalize(crops_u8, mean=MEAN, std=STD):
    """ToTensor + Normalize of uint8 [..., H, W, 3] -> float32 [..., 3, H, W]: (v / 255 - m) / s, every step in float32"""
    x = np.moveaxis(crops_u8.astype(np.float32) / np.float32(255.0), -1, -3)
    m = np.asarray(mean, np.float32).reshape(3, 1, 1); s = np.asarray(std, np.float32).reshape(3, 1, 1)
    return ((x - m) / s).astype(np.float32)


def ten_crop_reference(resized_u8, size):
    """uint8 [B, RH, RW, 3] resized images -> float32 [B, 10, 3, CH, CW]"""
    return np.stack([to_tensor_normalize(ten_crop_u8(im, size)) for im in resized_u8])


def mean_inputs(name):
    B, n, D, seed = MEAN_CASES[name]
    return np.random.default_rng(seed).standard_normal((B, n, D)).astype(np.float32)


def sequential_mean(x):
    """float32 [B, n, D] -> [B, D]: ((x0 + x1) + x2) + ... in float32, then / float32(n)"""
    acc = x[:, 0].astype(np.float32).copy()
    for t in range(1, x.shape[1]):
        acc = (acc + x[:, t]).astype(np.float32)
    return (acc / np.float32(x.shape[1])).astype(np.float32)


def mean_tail(D):
    """the number of trailing columns torch's CPU sum kernel leaves to its scalar loop"""
    return D % 32


def torch_mean(x, tail):
    """sequential_mean, with the last `tail` columns in the scalar loop's order: p[k] = x[k] + x[4 + k] + ... over the whole fours of
    rows, the remaining rows onto p[0], then ((p[0] + p[1]) + p[2]) + p[3]"""
    out = sequential_mean(x)
    if tail:
        n = x.shape[1]
        xs = x[:, :, x.shape[2] - tail:]
        p = [np.zeros_like(xs[:, 0]) for _ in range(4)]
        for t in range(n):
            k = t % 4 if t < (n // 4) * 4 else 0
            p[k] = (p[k] + xs[:, t]).astype(np.float32)
        acc = p[0]
        for k in (1, 2, 3):
            acc = (acc + p[k]).astype(np.float32)
        out[:, x.shape[2] - tail:] = acc / np.float32(n)
    return out


def pool_case(name):
    """-> (x [M, D] float32, row names, query names): keys are name[:7]; rows of the groups a (1), b (2), c (7), d (13) interleaved,
    row POOL_ZERO_ROW all zero; five queries, the key of group c twice, in an order that is not the groups'"""
    M, D, seed = POOL_CASES[name]
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((M, D)) * rng.uniform(0.1, 30.0, size=(M, 1))).astype(np.float32)
    x[POOL_ZERO_ROW] = 0.0
    keys = ["0004_c1"] * 13 + ["0003_c2"] * 7 + ["0002_c5"] * 2 + ["0001_c3"]
    perm = np.random.default_rng(seed + 1).permutation(M)
    keys = [keys[i] for i in perm]
    names = ["%s_s1_%06d_00.jpg" % (k, i) for i, k in enumerate(keys)]
    queries = ["0003_c2s1_000151_00.jpg", "0001_c3s1_000551_00.jpg", "0004_c1s2_000001_00.jpg", "0003_c2s3_000301_00.jpg", "0002_c5s1_000451_00.jpg"]
    return x, names, queries


def group_rows(names, queries, key=lambda f: f[:7]):
    """per query the row indices that share its key, in the order the rows come (a dict of lists, filled row by row)"""
    d = {}
    for i, f in enumerate(names):
        d.setdefault(key(f), []).append(i)
    return [d[key(q)] for q in queries]


def normalize64(x):
    """t = x / ||x|| in float64, the sum of squares exactly rounded; an all-zero row stays zero"""
    x64 = x.astype(np.float64)
    norms = np.array([math.sqrt(math.fsum((x64[i] * x64[i]).tolist())) for i in range(x.shape[0])])
    norms[norms == 0.0] = 1.0
    return x64 / norms[:, None]


def pool64(t, groups):
    """float64 max and mean of the rows of every query's group"""
    return (np.stack([t[g].max(axis=0) for g in groups]), np.stack([np.array([math.fsum(col) for col in t[g].T.tolist()]) / len(g) for g in groups]))


def _ordered(a):
    """float32 -> int64 that counts float32 steps monotonically (negative values mirrored)"""
    b = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7fffffff), b)


def pack_steps(recorded_f32, t64):
    """recorded float32 array -> its distance from float32(t64) in float32 steps (int16)"""
    d = _ordered(recorded_f32) - _ordered(t64.astype(np.float32))
    assert np.abs(d).max() < 30000
    return d.astype(np.int16)


def unpack_steps(steps, t64):
    o = _ordered(t64.astype(np.float32)) + steps.astype(np.int64)
    b = np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32)
    return b.view(np.float32)
