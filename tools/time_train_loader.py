#!/usr/bin/env python3
"""Throughput of the fine-tune training loader: `GpuTrainLoader` (GPU decode + one ssg_train_transform_u8 call per batch) next to the
reference's way, a CPU `torch.utils.data.DataLoader` whose workers decode with Pillow and run the transforms per item (stand-ins of
Resize / RandomSizedRectCrop / RandomHorizontalFlip / ToTensor / Normalize / the reid RandomErasing written to their published
behaviour), measured in the same call, batch 128, K = 4, 256 x 128 output:
  market   128 x 64 files (Market-1501's size), selftraining's pipeline (Resize)
  duke     ragged Duke-like files (h 150..400, w 50..160), selftraining's pipeline (Resize)
  duke_rc  the same files, SSG++'s pipeline (RandomSizedRectCrop)
Device-synchronised clocks, one warm-up epoch before the timed one.  Prints one JSON line.
--kernel-only: only transform_batch on one decoded batch per set, `--reps` times (run under `rocprofv3 --kernel-trace --stats`), and the
bytes each launch moves (computed from the shapes) for the bytes-over-HBM-peak figure."""
import argparse
import io
import json
import math
import os
import random
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK = 8.0e12           # MI355X HBM3E, bytes/s


def make_files(root, n, sizes, seed):
    from PIL import Image
    from time_loader import picture
    rng = np.random.default_rng(seed)
    names, cache = [], {}
    for i in range(n):
        h, w = sizes(rng)
        key = (h, w, i % 64)
        if key not in cache:
            buf = io.BytesIO()
            Image.fromarray(picture(rng, h, w)).save(buf, "JPEG", quality=90)
            cache[key] = buf.getvalue()
        name = "%06d.jpg" % i
        with open(os.path.join(root, name), "wb") as f:
            f.write(cache[key])
        names.append(name)
    return [(nm, i // 4, 0) for i, nm in enumerate(names)]           # identities of 4 images


def market(rng):
    return 128, 64


def duke(rng):
    return int(rng.integers(150, 401)), int(rng.integers(50, 161))


class _Erase(object):
    def __init__(self, tf):
        self.tf = tf

    def __call__(self, img):
        tf = self.tf
        if random.uniform(0, 1) > tf.erase_p:
            return img
        for _ in range(100):
            area = img.size()[1] * img.size()[2]
            target = random.uniform(tf.sl, tf.sh) * area
            ar = random.uniform(tf.r1, 1 / tf.r1)
            h, w = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
            if w < img.size()[2] and h < img.size()[1]:
                x1, y1 = random.randint(0, img.size()[1] - h), random.randint(0, img.size()[2] - w)
                for c in range(3):
                    img[c, x1:x1 + h, y1:y1 + w] = tf.erase_fill[c]
                return img
        return img


class _RectCrop(object):
    def __init__(self, H, W):
        self.H, self.W = H, W

    def __call__(self, img):
        from PIL import Image
        for _ in range(10):
            area = img.size[0] * img.size[1]
            t, ar = random.uniform(0.64, 1.0) * area, random.uniform(2, 3)
            h, w = int(round(math.sqrt(t * ar))), int(round(math.sqrt(t / ar)))
            if w <= img.size[0] and h <= img.size[1]:
                x1, y1 = random.randint(0, img.size[0] - w), random.randint(0, img.size[1] - h)
                return img.crop((x1, y1, x1 + w, y1 + h)).resize((self.W, self.H), Image.BILINEAR)
        return img.resize((self.W, self.H), Image.BILINEAR)


class _CpuItems(object):
    """reid Preprocessor + Compose on the CPU (what the reference's DataLoader workers run per item)"""

    def __init__(self, ds, root, tf):
        from make_golden_train_loader import stand_ins
        Compose, Resize, Flip, ToTensor, Normalize = stand_ins("torch")
        first = Resize((tf.height, tf.width)) if tf.crop == "resize" else _RectCrop(tf.height, tf.width)
        self.ds, self.root = ds, root
        self.t = Compose([first, Flip(tf.flip_p), ToTensor(), Normalize(tf.mean, tf.std), _Erase(tf)])

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        from PIL import Image
        fname, pid, camid = self.ds[i]
        return self.t(Image.open(os.path.join(self.root, fname)).convert("RGB")), fname, pid, camid


def time_gpu(ds, root, tf, dev):
    import torch
    import ssg_amd
    ld = ssg_amd.GpuTrainLoader(ds, root=root, transform=tf, batch_size=128, num_instances=4, num_workers=4)
    for _ in ld:                       # warm-up epoch (coefficient tables cached, allocator warm)
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter(); n = 0
    for imgs, _, _, _ in ld:
        n += imgs.shape[0]
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def time_cpu(ds, root, tf, workers):
    from torch.utils.data import DataLoader
    from ssg_amd.trainloader import TrainSchedule
    order = [i for b in TrainSchedule(ds, tf, 128, 4, 0).begin().batches() for i in b]
    ld = DataLoader(_CpuItems(ds, root, tf), batch_size=128, num_workers=workers, sampler=order, pin_memory=True, drop_last=True)
    it = iter(ld)
    next(it); next(it)                 # worker start-up and the first batches are not timed
    t0 = time.perf_counter(); n = 0
    for imgs, _, _, _ in it:
        imgs = imgs.cuda(non_blocking=True)
        n += imgs.shape[0]
    import torch
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def kernel_only(sets, dev, reps):
    import torch
    from ssg_amd import jpeg
    from ssg_amd import trainloader as tl
    out = {}
    for name, (ds, root, tf) in sets.items():
        files = []
        for fname, _, _ in ds[:128]:
            with open(os.path.join(root, fname), "rb") as f:
                files.append(f.read())
        pix = jpeg.decode_batch(files, dev)
        random.seed(0); torch.manual_seed(0)
        ep = tl.TrainSchedule(ds, tf, 128, 4, 4).begin()
        draws = ep.items(0, [(int(p.shape[0]), int(p.shape[1])) for p in pix])
        res = torch.empty((128, 3, tf.height, tf.width), dtype=torch.float32, device=dev)
        for _ in range(reps):
            tl.transform_batch(pix, draws, tf, dev, out=res)
        torch.cuda.synchronize()
        # bytes: the float32 output once + the source rows the crops cover (each read once from HBM; LDS holds the band's rows)
        src = sum(d.box[2] * d.box[3] * 3 for d in draws)
        out[name] = {"bytes_out": 128 * 3 * tf.height * tf.width * 4, "bytes_src": int(src), "reps": reps}
    return out


def parse_trace(path, reps):
    """kernel-trace csv of a --kernel-only run -> {set: mean microseconds of train_transform_kernel} (launches in set order, reps each)"""
    import csv
    durs = []
    for row in csv.DictReader(open(path)):
        if "train_transform_kernel" in row["Kernel_Name"]:
            durs.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    durs = [d for _, d in sorted(durs)]
    return {name: round(float(np.mean(durs[i * reps:(i + 1) * reps])), 2) for i, name in enumerate(("market", "duke", "duke_rc"))}


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--parse-trace":
        print(json.dumps(parse_trace(sys.argv[2], int(sys.argv[3]))))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--kernel-us", type=str, default=None, help="json {set: mean kernel microseconds} from the rocprofv3 run, to fold in")
    a = ap.parse_args()
    import torch
    from ssg_amd.trainloader import TrainTransform
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    tmp = tempfile.mkdtemp(prefix="ttl_")
    rm, rd = os.path.join(tmp, "m"), os.path.join(tmp, "d")
    os.makedirs(rm); os.makedirs(rd)
    dm = make_files(rm, a.n, market, 1)
    dd = make_files(rd, a.n, duke, 2)
    sets = {"market": (dm, rm, TrainTransform(256, 128)), "duke": (dd, rd, TrainTransform(256, 128)),
            "duke_rc": (dd, rd, TrainTransform(256, 128, crop="random_rect"))}
    if a.kernel_only:
        print(json.dumps({"kernel_only": kernel_only(sets, dev, a.reps)}))
        return
    res = {"n": a.n, "batch": 128, "K": 4, "out": [256, 128]}
    for name, (ds, root, tf) in sets.items():
        r = {"gpu_loader_img_s": round(time_gpu(ds, root, tf, dev))}
        for w in (4, 16):
            r["cpu_dataloader_%dw_img_s" % w] = round(time_cpu(ds, root, tf, w))
        r["speedup_vs_cpu_16w"] = round(r["gpu_loader_img_s"] / r["cpu_dataloader_16w_img_s"], 2)
        res[name] = r
    if a.kernel_us:
        ko = kernel_only(sets, dev, 1)
        for name, us in json.loads(a.kernel_us).items():
            b = ko[name]["bytes_out"] + ko[name]["bytes_src"]
            res[name]["kernel_us"] = us
            res[name]["kernel_bytes"] = b
            res[name]["kernel_hbm_fraction"] = round(b / (us * 1e-6) / HBM_PEAK, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
