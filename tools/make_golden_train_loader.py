#!/usr/bin/env python3
"""Generate tests/golden/train_loader_ref.npz: what the reference's training loader hands out (run where the reference is).

The reference's own RandomIdentitySampler (reid/utils/data/sampler.py), RandomSizedRectCrop and RandomErasing
(reid/utils/data/transforms.py) and Preprocessor (reid/utils/data/preprocessor.py) are imported under make_golden.import_reid()'s stub
modules and run inside a REAL torch.utils.data.DataLoader(..., sampler=RandomIdentitySampler(dataset, K), drop_last=True), as
selftraining.py:325-331 and reid/eug.py:81-86 build it, with num_workers 0 and 4, two epochs per run.

torchvision is not installed here, so Compose / Resize / RandomHorizontalFlip / ToTensor / Normalize are stand-ins written to their
published behaviour (torchvision >= 0.8 for PIL images): Resize((h, w)) = img.resize((w, h), BILINEAR); the flip draws
`torch.rand(1) < p` -- one run uses the older torchvision flip that drew `random.random() < p` instead; ToTensor = uint8 HWC -> float32
CHW / 255; Normalize = (x - mean) / std with float32 mean / std tensors.

Inputs: JPEG files written with Pillow -- ragged sizes (Market's 128 x 64, taller Duke-like crops), one grayscale, one progressive --
with list labels (selftraining's [label of split 0, label of split 1]) and scalar labels (EUG), identities with fewer than K images
(the replace=True branch).  Recorded: the file bytes and dataset lists, the seeds, the fnames of every batch, the sha256 of every item's
float32 tensor, the full first batch of two runs, and hashes of the global torch / numpy / python generator states after each epoch.
"""
import hashlib
import io
import os
import random
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "train_loader_ref.npz")

H, W, BATCH, K = 64, 32, 8, 4
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
# source sizes (h, w); the progressive and the grayscale file are marked
SIZES = [(128, 64), (128, 64), (128, 64), (256, 128), (214, 86), (301, 97), (180, 70), (263, 109), (96, 48), (150, 61), (128, 64), (330, 120),
         (240, 94), (77, 40), (128, 64), (199, 83), (275, 101), (128, 64), (142, 58), (222, 90), (310, 115), (128, 64), (163, 66), (251, 99),
         (188, 77), (128, 64), (207, 81), (290, 108), (134, 55), (128, 64), (170, 72), (233, 95), (128, 64), (119, 50)]
PROGRESSIVE, GRAY = 7, 12
# identity of each file (first-appearance order is not sorted order: the sampler keys by first appearance); ids 5 and 9 have < K images
IDS = [3, 3, 3, 3, 7, 7, 7, 1, 1, 1, 1, 5, 5, 8, 8, 8, 8, 8, 2, 2, 2, 2, 9, 0, 0, 0, 0, 4, 4, 4, 6, 6, 6, 6]
# runs: (pipeline, label form, num_workers, flip generator, seed)
RUNS = [("resize", "list", 0, "torch", 11), ("resize", "list", 4, "torch", 12), ("random_rect", "scalar", 0, "torch", 13),
        ("random_rect", "scalar", 4, "torch", 14), ("resize", "scalar", 4, "python", 15), ("random_rect", "list", 4, "python", 16)]
FULL_RUNS = (0, 3)          # runs whose first batch is stored in full


def sha(b):
    return hashlib.sha256(b).hexdigest()


def rng_hashes():
    import torch
    st = np.random.get_state()
    return (sha(torch.get_rng_state().numpy().tobytes()), sha(st[1].tobytes() + repr(st[2:]).encode()), sha(repr(random.getstate()).encode()))


def stand_ins(flip_rng):
    import torch
    from PIL import Image

    class Compose(object):
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, img):
            for t in self.transforms:
                img = t(img)
            return img

    class Resize(object):
        def __init__(self, size, interpolation=Image.BILINEAR):
            self.size, self.interpolation = size, interpolation

        def __call__(self, img):
            return img.resize((self.size[1], self.size[0]), self.interpolation)

    class RandomHorizontalFlip(object):
        def __init__(self, p=0.5):
            self.p = p

        def __call__(self, img):
            hit = (torch.rand(1) < self.p) if flip_rng == "torch" else (random.random() < self.p)
            return img.transpose(Image.FLIP_LEFT_RIGHT) if hit else img

    class ToTensor(object):
        def __call__(self, pic):
            a = torch.from_numpy(np.array(pic, np.uint8, copy=True)).view(pic.size[1], pic.size[0], len(pic.getbands()))
            return a.permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    class Normalize(object):
        def __init__(self, mean, std):
            self.mean, self.std = mean, std

        def __call__(self, t):
            m = torch.as_tensor(self.mean, dtype=t.dtype); s = torch.as_tensor(self.std, dtype=t.dtype)
            return t.sub_(m[:, None, None]).div_(s[:, None, None])
    return Compose, Resize, RandomHorizontalFlip, ToTensor, Normalize


def pipeline(reid, kind, flip_rng):
    from reid.utils.data import transforms as RT
    Compose, Resize, RandomHorizontalFlip, ToTensor, Normalize = stand_ins(flip_rng)
    first = Resize((H, W)) if kind == "resize" else RT.RandomSizedRectCrop(H, W)
    return Compose([first, RandomHorizontalFlip(), ToTensor(), Normalize(mean=MEAN, std=STD), RT.RandomErasing(probability=0.5, sh=0.2, r1=0.3)])


def host_item(blob, draw, tf):
    """one item rebuilt from its ItemDraw (ssg_amd.trainloader) with Pillow + numpy float32, the published formulas: crop + bilinear
    resize (Pillow), flip, ToTensor (/ 255), Normalize ((x - m) / s), erase (float32 fill) -> float32 [3, H, W]"""
    from PIL import Image
    img = Image.open(io.BytesIO(bytes(blob))).convert("RGB")
    x0, y0, cw, ch = draw.box
    a = np.asarray(img.crop((x0, y0, x0 + cw, y0 + ch)).resize((tf.width, tf.height), Image.BILINEAR))
    if draw.flip:
        a = a[:, ::-1]
    t = np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
    t = (t - np.asarray(tf.mean, np.float32)[:, None, None]) / np.asarray(tf.std, np.float32)[:, None, None]
    if draw.erase is not None:
        r, c, eh, ew = draw.erase
        t[:, r:r + eh, c:c + ew] = np.asarray(tf.erase_fill, np.float32)[:, None, None]
    return t


def make_files(d):
    from PIL import Image
    rng = np.random.default_rng(5)
    names, blobs = [], []
    for i, (h, w) in enumerate(SIZES):
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([xx * 255.0 / (w - 1), yy * 255.0 / (h - 1), ((xx * 3 + yy * 5) % 256)], -1) + rng.normal(0, 18, (h, w, 3))
        a = np.clip(a, 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        if i == GRAY:
            Image.fromarray(a[:, :, 0]).save(buf, "JPEG", quality=85)
        else:
            Image.fromarray(a).save(buf, "JPEG", quality=80 + i % 15, subsampling=[0, 1, 2][i % 3], progressive=(i == PROGRESSIVE))
        name = "%04d_c%ds1_%06d.jpg" % (IDS[i], 1 + i % 6, i)
        with open(os.path.join(d, name), "wb") as f:
            f.write(buf.getvalue())
        names.append(name); blobs.append(buf.getvalue())
    return names, blobs


def datasets(names):
    lab = np.asarray(IDS, np.int64)
    lab2 = (lab * 7 + 3) % 11                       # the second split's labels (any labelling: the sampler keys by split 0)
    lst = [(n, [np.int64(lab[i]), np.int64(lab2[i])], 0) for i, n in enumerate(names)]
    sca = [(n, int(lab[i]), 1 + i % 6) for i, n in enumerate(names)]
    return {"list": lst, "scalar": sca}, lab2


def main():
    import torch
    from torch.utils.data import DataLoader
    from make_golden import import_reid
    reid = import_reid()
    from reid.utils.data.preprocessor import Preprocessor
    from reid.utils.data.sampler import RandomIdentitySampler
    rec = {}
    with tempfile.TemporaryDirectory() as d:
        names, blobs = make_files(d)
        dsets, lab2 = datasets(names)
        for i, b in enumerate(blobs):
            rec["file_%02d" % i] = np.frombuffer(b, np.uint8)
        rec["names"] = np.asarray(names); rec["ids"] = np.asarray(IDS, np.int64); rec["ids2"] = lab2
        rec["camids"] = np.asarray([1 + i % 6 for i in range(len(names))], np.int64)
        rec["out_hw"] = np.asarray([H, W]); rec["batch_k"] = np.asarray([BATCH, K])
        rec["runs"] = np.asarray(["%s,%s,%d,%s,%d" % r for r in RUNS])
        for r, (kind, form, nw, flip_rng, seed) in enumerate(RUNS):
            ds = dsets[form]
            loader = DataLoader(Preprocessor(ds, root=d, transform=pipeline(reid, kind, flip_rng)), batch_size=BATCH, num_workers=nw,
                                sampler=RandomIdentitySampler(ds, K), pin_memory=False, drop_last=True)
            torch.manual_seed(seed); np.random.seed(seed); random.seed(seed)
            for e in range(2):
                fn, hs = [], []
                for bi, (imgs, fnames, pids, camids) in enumerate(loader):
                    assert imgs.shape == (BATCH, 3, H, W) and imgs.dtype == torch.float32
                    fn.append(list(fnames))
                    hs.append([sha(imgs[j].contiguous().numpy().tobytes()) for j in range(BATCH)])
                    if r in FULL_RUNS and e == 0 and bi == 0:
                        rec["first_%d" % r] = imgs.numpy().copy()
                    if form == "list":
                        assert isinstance(pids, list) and len(pids) == 2 and pids[0].dtype == torch.int64
                    else:
                        assert pids.dtype == torch.int64
                rec["fnames_%d_%d" % (r, e)] = np.asarray(fn)
                rec["sha_%d_%d" % (r, e)] = np.asarray(hs)
                rec["rng_%d_%d" % (r, e)] = np.asarray(rng_hashes())
                print("run %d (%s, %s labels, %d workers, %s flip) epoch %d: %d batches" % (r, kind, form, nw, flip_rng, e, len(fn)))
        rec["seeds"] = np.asarray([r[4] for r in RUNS], np.int64)
    np.savez_compressed(OUT, **rec)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
