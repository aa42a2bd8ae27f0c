"""Training-batch loader of the fine-tune phase on the GPU -- the replacement for the reference's
`DataLoader(Preprocessor(new_dataset, root, transform=train_transformer), batch_size, num_workers=4,
sampler=RandomIdentitySampler(new_dataset, num_instances), pin_memory=True, drop_last=True)` (selftraining.py:315-331) and for
SSG++'s `get_dataloader(training=True)` (reid/eug.py:62-96 with num_classes == 0).

Three layers:
  * `TrainTransform`: the supported transform pipelines (Resize or RandomSizedRectCrop, RandomHorizontalFlip, ToTensor, Normalize,
    the reid RandomErasing), read from a reference `Compose` by `TrainTransform.from_compose`;
  * `TrainSchedule`: every random choice the reference's DataLoader makes, re-derived on the host from the same generators in the same
    order -- the iterator's base seed, the identity sampler (torch.randperm + np.random.choice on the global generators), and per item
    the crop window, the flip bit and the erase rectangle, drawn from the generators the reference's worker k % num_workers would use
    (seeded base_seed + worker_id, private objects here) or, with num_workers=0, from the global ones.  Device-free;
  * `GpuTrainLoader`: reads the files, decodes them on the GPU (ssg_amd.jpeg, Pillow for what it does not take), and applies the drawn
    transforms to a whole batch of ragged images in ONE call of `ssg_train_transform_u8` (csrc/train_transform.hip), bit-exact with
    Pillow + the published float32 formulas.  Items are collated like `default_collate` makes `(img, fname, pid, camid)`.
"""
import math
import os.path as osp
import random

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from .preprocessor import MEAN, STD, _PRECISION_BITS

ERASE_FILL = (0.4914, 0.4822, 0.4465)      # reid/utils/data/transforms.py:64 RandomErasing(mean=...)
TT_WORDS = 20                               # int32 words per image of ssg_train_transform_u8's descriptor table (include/ssg_hip.h)
LDS_BUDGET = 32768                          # bytes of LDS per workgroup the band height is sized to (>= 4 workgroups per CU)
calls = {"ssg_train_transform_u8": 0}       # launches of the transform (tests count them)
_coeff_cache = {}


# ---------------------------------------------------------------------------------------------------------------- coefficient tables
def bilinear_coeffs_np(in_size, out_size):
    """`preprocessor.bilinear_coeffs` vectorised over the output pixels (the same float64 operations in the same order, the window sum
    accumulated tap by tap like Resample.c's loop) -> (first [out], count [out], k [out, ksize]) int32; cached by (in, out)."""
    key = (int(in_size), int(out_size))
    hit = _coeff_cache.get(key)
    if hit is not None:
        return hit
    in_size, out_size = key
    if in_size <= 0 or out_size <= 0:
        raise ValueError("resize %d -> %d" % key)
    scale = float(in_size) / float(out_size)
    support = max(scale, 1.0)
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / support
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    lo = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)
    hi = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    count = hi - lo
    w = np.zeros((out_size, ksize), np.float64)
    total = np.zeros(out_size, np.float64)
    for t in range(ksize):
        a = np.abs(((lo + t) - center + 0.5) * inv)
        v = np.where(a < 1.0, 1.0 - a, 0.0)
        v = np.where(t < count, v, 0.0)
        w[:, t] = v
        total = total + v
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    s = w * (1 << _PRECISION_BITS)
    k = np.where(w < 0, np.trunc(-0.5 + s), np.trunc(0.5 + s)).astype(np.int32)
    k[np.arange(ksize)[None, :] >= count[:, None]] = 0
    res = (lo.astype(np.int32), count.astype(np.int32), k)
    _coeff_cache[key] = res
    return res


# ----------------------------------------------------------------------------------------------------------------------- transforms
def _is_bilinear(interp):
    if interp is None:
        return True
    if isinstance(interp, int) and not isinstance(interp, bool):
        return interp == 2                                  # PIL.Image.BILINEAR
    v = getattr(interp, "value", interp)                     # torchvision InterpolationMode.BILINEAR (value 'bilinear') or PIL's enum
    return v == 2 or str(v).lower() == "bilinear"


class TrainTransform(object):
    """The training pipeline the loader applies:  crop ('resize': Resize((height, width)) of the whole image; 'random_rect':
    RandomSizedRectCrop(height, width), reid/utils/data/transforms.py:22-48) -> RandomHorizontalFlip(flip_p) -> ToTensor ->
    Normalize(mean, std) -> the reid RandomErasing(erase_p, sl, sh, r1, erase_fill).  flip_p=None / erase_p=None: the transform is
    absent (it draws nothing); flip_rng: 'torch' = torchvision >= 0.8 (`torch.rand(1) < p`), 'python' = older (`random.random() < p`)."""

    def __init__(self, height, width, crop="resize", flip_p=0.5, flip_rng="torch", mean=MEAN, std=STD, erase_p=0.5, sl=0.02, sh=0.2, r1=0.3,
                 erase_fill=ERASE_FILL):
        if crop not in ("resize", "random_rect"):
            raise ValueError("crop must be 'resize' or 'random_rect', got %r" % (crop,))
        if flip_rng not in ("torch", "python"):
            raise ValueError("flip_rng must be 'torch' or 'python', got %r" % (flip_rng,))
        if int(height) <= 0 or int(width) <= 0:
            raise ValueError("output size %r x %r" % (height, width))
        self.height, self.width, self.crop, self.flip_p, self.flip_rng = int(height), int(width), crop, flip_p, flip_rng
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.erase_p, self.sl, self.sh, self.r1 = erase_p, float(sl), float(sh), float(r1)
        self.erase_fill = tuple(float(v) for v in erase_fill)
        if len(self.mean) != 3 or len(self.std) != 3 or len(self.erase_fill) != 3:
            raise ValueError("mean / std / erase_fill need 3 values (RGB)")

    @classmethod
    def from_compose(cls, compose, flip_rng="torch"):
        """a reference `Compose` (torchvision.transforms.Compose or anything with `.transforms`), read by class name and attributes:
        Resize(size=(h, w), bilinear) | RandomSizedRectCrop(height, width), [RandomHorizontalFlip(p)], ToTensor, [Normalize(mean, std)],
        [RandomErasing(probability, sl, sh, r1, mean) -- the reid one].  Anything else raises ValueError naming the transform."""
        ts = list(getattr(compose, "transforms", compose))
        kw, stage = {"flip_p": None, "erase_p": None, "mean": (0.0, 0.0, 0.0), "std": (1.0, 1.0, 1.0), "flip_rng": flip_rng}, 0
        order = {"crop": 1, "flip": 2, "totensor": 3, "normalize": 4, "erase": 5}

        def step(kind, t):
            nonlocal stage
            if order[kind] <= stage:
                raise ValueError("transform %s out of place in %r (supported order: Resize | RandomSizedRectCrop, RandomHorizontalFlip, ToTensor, "
                                 "Normalize, RandomErasing)" % (type(t).__name__, [type(x).__name__ for x in ts]))
            stage = order[kind]
        for t in ts:
            name = type(t).__name__
            if name == "Resize":
                size = getattr(t, "size", None)
                if not isinstance(size, (tuple, list)) or len(size) != 2:
                    raise ValueError("Resize(size=%r): only Resize((height, width)) is supported" % (size,))
                if not _is_bilinear(getattr(t, "interpolation", None)) or getattr(t, "max_size", None) is not None:
                    raise ValueError("Resize with interpolation %r: only bilinear is supported" % (getattr(t, "interpolation", None),))
                step("crop", t)
                kw.update(height=int(size[0]), width=int(size[1]), crop="resize")
            elif name == "RandomSizedRectCrop":
                if not _is_bilinear(getattr(t, "interpolation", None)):
                    raise ValueError("RandomSizedRectCrop with interpolation %r: only bilinear is supported" % (t.interpolation,))
                step("crop", t)
                kw.update(height=int(t.height), width=int(t.width), crop="random_rect")
            elif name == "RandomHorizontalFlip":
                step("flip", t)
                kw["flip_p"] = float(getattr(t, "p", 0.5))
            elif name == "ToTensor":
                step("totensor", t)
            elif name == "Normalize":
                step("normalize", t)
                kw["mean"], kw["std"] = tuple(t.mean), tuple(t.std)
            elif name == "RandomErasing" and all(hasattr(t, a) for a in ("probability", "sl", "sh", "r1", "mean")):
                step("erase", t)
                kw.update(erase_p=float(t.probability), sl=t.sl, sh=t.sh, r1=t.r1, erase_fill=tuple(t.mean))
            elif name == "RandomErasing":
                raise ValueError("unsupported transform RandomErasing(p, scale, ratio, value) (torchvision's): only the reid "
                                 "RandomErasing(probability, sl, sh, r1, mean) is supported")
            else:
                raise ValueError("unsupported transform %s in the training pipeline" % name)
        if "crop" not in kw or stage < order["totensor"]:
            raise ValueError("the training pipeline needs Resize((h, w)) or RandomSizedRectCrop(h, w) followed by ToTensor, got %r"
                             % [type(x).__name__ for x in ts])
        return cls(**kw)


def as_transform(transform):
    if isinstance(transform, TrainTransform):
        return transform
    return TrainTransform.from_compose(transform)


# ------------------------------------------------------------------------------------------------------------------------- schedule
class ItemDraw(object):
    """the random choices of one item: crop box (x0, y0, cw, ch) in the source, flip bit, erase rectangle (row, col, eh, ew) in the
    output tensor or None"""
    __slots__ = ("box", "flip", "erase")

    def __init__(self, box, flip, erase):
        self.box, self.flip, self.erase = box, flip, erase

    def __repr__(self):
        return "ItemDraw(box=%r, flip=%r, erase=%r)" % (self.box, self.flip, self.erase)


class _Rngs(object):
    """the python `random` and torch generators one worker (or, with pyrng=random / trng=None, the main process) draws from"""
    __slots__ = ("py", "torch")

    def __init__(self, py, trng):
        self.py, self.torch = py, trng


def draw_item(tf, rng, size):
    """the draws of reid Preprocessor + Compose for one image of size (h, w), in the order the transforms make them"""
    h, w = size
    py = rng.py
    box = (0, 0, w, h)
    if tf.crop == "random_rect":                               # reid/utils/data/transforms.py:28-48
        area = w * h
        for _ in range(10):
            target_area = py.uniform(0.64, 1.0) * area
            aspect_ratio = py.uniform(2, 3)
            ch = int(round(math.sqrt(target_area * aspect_ratio)))
            cw = int(round(math.sqrt(target_area / aspect_ratio)))
            if cw <= w and ch <= h:
                x1 = py.randint(0, w - cw)
                y1 = py.randint(0, h - ch)
                box = (x1, y1, cw, ch)
                break
    flip = False
    if tf.flip_p is not None:
        if tf.flip_rng == "torch":
            flip = bool(torch.rand(1, generator=rng.torch) < tf.flip_p)
        else:
            flip = py.random() < tf.flip_p
    erase = None
    if tf.erase_p is not None and not (py.uniform(0, 1) > tf.erase_p):     # reid/utils/data/transforms.py:70-94
        H, W = tf.height, tf.width
        for _ in range(100):
            target_area = py.uniform(tf.sl, tf.sh) * (H * W)
            aspect_ratio = py.uniform(tf.r1, 1 / tf.r1)
            eh = int(round(math.sqrt(target_area * aspect_ratio)))
            ew = int(round(math.sqrt(target_area / aspect_ratio)))
            if ew < W and eh < H:
                x1 = py.randint(0, H - eh)
                y1 = py.randint(0, W - ew)
                erase = (x1, y1, eh, ew)
                break
    if box[2] <= 0 or box[3] <= 0:
        raise ValueError("empty crop window %r of a %dx%d image" % (box, h, w))
    return ItemDraw(box, flip, erase)


def identity_index(dataset):
    """reid RandomIdentitySampler.__init__: {identity: [dataset indices]} in first-appearance order; the key is pid[0] for list labels"""
    idx = {}
    try:
        for i, (_, pid, _) in enumerate(dataset):
            idx.setdefault(pid[0], []).append(i)
    except (TypeError, IndexError, KeyError):
        idx = {}
        for i, (_, pid, _) in enumerate(dataset):
            idx.setdefault(pid, []).append(i)
    return idx


class EpochSchedule(object):
    """one epoch of a TrainSchedule (one `for ... in loader`): created after the base-seed draw; `batches()` draws the sampler on first
    use; `items(k, sizes)` draws the transforms of batch k (called in batch order)"""

    def __init__(self, sched, base_seed):
        self.sched, self.base_seed = sched, base_seed
        self._batches = None
        self._workers = {}

    def batches(self):
        if self._batches is None:
            s = self.sched
            perm = torch.randperm(len(s.pids))
            order = []
            for i in perm.tolist():
                t = s.index[s.pids[i]]
                order.extend(np.random.choice(t, size=s.num_instances, replace=len(t) < s.num_instances).tolist())
            bs = s.batch_size
            self._batches = [order[k * bs:(k + 1) * bs] for k in range(len(order) // bs)]
        return self._batches

    def rngs(self, k):
        """the generators batch k's transforms draw from: worker k % num_workers's (seeded base_seed + worker_id, as
        torch/utils/data/_utils/worker.py does), or the process's own with num_workers=0"""
        nw = self.sched.num_workers
        if nw == 0:
            return _Rngs(random, None)
        wid = k % nw
        r = self._workers.get(wid)
        if r is None:
            seed = self.base_seed + wid
            r = self._workers[wid] = _Rngs(random.Random(seed), torch.Generator().manual_seed(seed))
        return r

    def items(self, k, sizes):
        rng = self.rngs(k)
        return [draw_item(self.sched.transform, rng, sz) for sz in sizes]


class TrainSchedule(object):
    """The random streams of `DataLoader(Preprocessor(dataset, transform), batch_size, num_workers, sampler=RandomIdentitySampler(dataset,
    num_instances), drop_last=True)`, device-free.  `epoch(sizes)` yields (indices, [ItemDraw]) per batch; sizes: sequence or callable
    dataset index -> (h, w)."""

    def __init__(self, dataset, transform, batch_size=128, num_instances=4, num_workers=4):
        if int(batch_size) <= 0 or int(num_instances) <= 0 or int(num_workers) < 0:
            raise ValueError("batch_size / num_instances must be > 0 and num_workers >= 0")
        self.dataset = dataset
        self.transform = as_transform(transform)
        self.batch_size, self.num_instances, self.num_workers = int(batch_size), int(num_instances), int(num_workers)
        self.index = identity_index(dataset)
        self.pids = list(self.index.keys())

    def __len__(self):
        return len(self.pids) * self.num_instances // self.batch_size

    def begin(self):
        """the iterator's first draw (torch/utils/data/dataloader.py _BaseDataLoaderIter.__init__), also with num_workers=0"""
        base_seed = int(torch.empty((), dtype=torch.int64).random_().item())
        return EpochSchedule(self, base_seed)

    def epoch(self, sizes):
        ep = self.begin()
        size_of = sizes if callable(sizes) else sizes.__getitem__
        return self._run(ep, size_of)

    def _run(self, ep, size_of):
        for k, idx in enumerate(ep.batches()):
            yield idx, ep.items(k, [size_of(i) for i in idx])


# --------------------------------------------------------------------------------------------------------------------------- kernel
def _pack_coeffs(keys):
    """{(in, out): offset} and the packed int32 buffer of first / count / k blocks for the given keys"""
    offs, parts, o = {}, [], 0
    for key in keys:
        if key in offs:
            continue
        f, c, k = bilinear_coeffs_np(*key)
        offs[key] = (o, k.shape[1])
        parts += [f, c, k.ravel()]
        o += f.size + c.size + k.size
    return offs, (np.concatenate(parts) if parts else np.zeros(1, np.int32))


def _band(tf, ykeys, B):
    """(band rows, LDS rows): the tallest band (<= 32 rows, at least 1024 workgroups while bands stay >= 4 rows) whose crop rows fit
    LDS_BUDGET for every vertical window table of the batch"""
    H, W = tf.height, tf.width
    tabs = [bilinear_coeffs_np(*key) for key in set(ykeys)]

    def need(R):
        y0 = np.arange(0, H, R)
        y1 = np.minimum(y0 + R, H) - 1
        return max(int(((f[y1] + c[y1]) - f[y0]).max()) for f, c, _ in tabs)
    R = min(32, H)
    while R > 1 and (need(R) * W * 3 > LDS_BUDGET or (B * ((H + R - 1) // R) < 1024 and R > 4)):
        R //= 2
    rows = need(R)
    if rows * W * 3 > 65536:
        raise ValueError("output width %d with a vertical reduction to %d source rows per output row does not fit the transform's LDS" % (W, rows))
    return R, rows


def transform_batch(sources, draws, tf, device=None, out=None):
    """decoded images (uint8 CUDA tensors [h, w, 3], any mix of sizes) + their ItemDraws -> float32 CUDA [B, 3, H, W], ONE kernel call"""
    import ctypes
    L = _lib.lib()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    B = len(sources)
    if B == 0 or len(draws) != B:
        raise ValueError("transform_batch: %d sources, %d draws" % (B, len(draws)))
    H, W = tf.height, tf.width
    xkeys, ykeys = [], []
    for s, d in zip(sources, draws):
        if not (torch.is_tensor(s) and s.dtype == torch.uint8 and s.dim() == 3 and s.shape[2] == 3 and s.is_cuda and s.is_contiguous()):
            raise ValueError("transform_batch: sources must be contiguous uint8 CUDA tensors [h, w, 3]")
        h, w = int(s.shape[0]), int(s.shape[1])
        x0, y0, cw, ch = d.box
        if not (0 <= x0 and 0 <= y0 and cw > 0 and ch > 0 and x0 + cw <= w and y0 + ch <= h):
            raise ValueError("crop window %r outside a %dx%d image" % (d.box, h, w))
        if d.erase is not None:
            er, ec, eh, ew = d.erase
            if not (0 <= er and 0 <= ec and eh >= 0 and ew >= 0 and er + eh <= H and ec + ew <= W):
                raise ValueError("erase rectangle %r outside %dx%d" % (d.erase, H, W))
        xkeys.append((cw, W)); ykeys.append((ch, H))
    offs, packed = _pack_coeffs(xkeys + ykeys)
    R, rows = _band(tf, ykeys, B)
    desc = np.zeros((B, TT_WORDS), np.uint32)
    for b, (s, d) in enumerate(zip(sources, draws)):
        a = s.data_ptr()
        xo, xks = offs[xkeys[b]]; yo, yks = offs[ykeys[b]]
        desc[b, :13] = (a & 0xFFFFFFFF, a >> 32, s.shape[0], s.shape[1]) + tuple(d.box) + (xo, xks, yo, yks, int(bool(d.flip)))
        if d.erase is not None:
            desc[b, 13:17] = d.erase
    desc_d = torch.from_numpy(desc.view(np.int32)).pin_memory().to(device, non_blocking=True)
    coef_d = torch.from_numpy(packed).pin_memory().to(device, non_blocking=True)
    if out is None:
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=device)
    f3 = lambda v: (ctypes.c_float * 3)(*v)      # noqa: E731
    check(L.ssg_train_transform_u8(ptr(desc_d), B, ptr(coef_d), H, W, R, rows, f3(tf.mean), f3(tf.std), f3(tf.erase_fill), ptr(out), stream()),
          "ssg_train_transform_u8")
    calls["ssg_train_transform_u8"] += 1
    return out


# --------------------------------------------------------------------------------------------------------------------------- loader
def _collate(values):
    from torch.utils.data import default_collate
    return default_collate(values)


class GpuTrainLoader(object):
    """`DataLoader(Preprocessor(dataset, root, transform), batch_size, num_workers, sampler=RandomIdentitySampler(dataset, num_instances),
    pin_memory=True, drop_last=True)` on the GPU.  Each `for ... in loader` is one epoch and yields (imgs float32 CUDA [B, 3, H, W], fnames,
    pids, camids) as default_collate makes them of (img, fname, pid, camid) items, with the reference's random streams (TrainSchedule).
    decode='gpu': files are decoded on the device (ssg_amd.jpeg; what it does not take goes to Pillow per file); 'pillow': all on the host."""

    def __init__(self, dataset, root=None, transform=None, batch_size=128, num_instances=4, num_workers=4, decode="gpu", device=None):
        if decode not in ("gpu", "pillow"):
            raise ValueError("decode must be 'gpu' or 'pillow'")
        if transform is None:
            raise ValueError("GpuTrainLoader needs the training transform (a TrainTransform or the reference's Compose)")
        self.dataset, self.root, self.decode, self.device = dataset, root, decode, device
        self.schedule = TrainSchedule(dataset, transform, batch_size, num_instances, num_workers)
        self.transform = self.schedule.transform
        self.batch_size = self.schedule.batch_size

    def __len__(self):
        return len(self.schedule)

    def _read(self, i):
        fname = self.dataset[i][0]
        with open(fname if self.root is None else osp.join(self.root, fname), "rb") as f:
            return f.read()

    def __iter__(self):
        ep = self.schedule.begin()          # the base-seed draw happens when the iterator is made, like DataLoader's
        return self._epoch(ep)

    def _epoch(self, ep):
        dev = torch.device("cuda", torch.cuda.current_device()) if self.device is None else torch.device(self.device)
        ahead = None           # (batch number, indices, pending decode) whose status words are not read yet
        for k, idx in enumerate(ep.batches()):
            files = [self._read(i) for i in idx]
            if self.decode == "gpu":
                # one batch of lookahead, as GpuBatchLoader: batch k + 1's decode is queued before batch k's status words are read
                from .jpeg import decode_batch_async
                nxt = (k, idx, decode_batch_async(files, dev))
                if ahead is not None:
                    yield self._finish(ep, ahead[0], ahead[1], ahead[2].result(), dev)
                ahead = nxt
            else:
                from .jpeg import _pillow_rgb
                pix = [torch.from_numpy(np.array(_pillow_rgb(f))).to(dev) for f in files]
                yield self._finish(ep, k, idx, pix, dev)
        if ahead is not None:
            yield self._finish(ep, ahead[0], ahead[1], ahead[2].result(), dev)

    def _finish(self, ep, k, idx, pix, dev):
        # the transforms of batch k are drawn here, just before it is handed out (with num_workers=0 the process's generators are then
        # consumed in the order the reference's in-process loading consumes them)
        draws = ep.items(k, [(int(p.shape[0]), int(p.shape[1])) for p in pix])
        imgs = transform_batch(pix, draws, self.transform, dev)
        recs = [self.dataset[i] for i in idx]
        return imgs, _collate([r[0] for r in recs]), _collate([r[1] for r in recs]), _collate([r[2] for r in recs])


def generate_dataloader(tgt_dataset, labels_list, train_transformer, iter_n, args):
    """selftraining.py:315-331 with the reference's signature: generate_dataset + GpuTrainLoader(..., num_workers=4)"""
    from .selftraining import generate_dataset
    new_dataset = generate_dataset(tgt_dataset.trainval, labels_list, iter_n)
    return GpuTrainLoader(new_dataset, root=tgt_dataset.images_dir, transform=train_transformer, batch_size=args.batch_size,
                          num_instances=args.num_instances, num_workers=4)
