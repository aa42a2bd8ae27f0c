"""Test-time extraction and multi-query pooling -- host-side mirror of reid/extract_feature.py and reid/test_dataset.py.

The script embeds four Market-1501 folders (bounding_box_train, query, gt_bbox, bounding_box_test), builds the multi-query
descriptors (per query file the L2-normalised gt_bbox features that share its `fname[:7]`, their column-wise max and mean), parses
ids and cameras from the file names and writes eleven .mat files.  Its commented-out test-time augmentation (:47-52, :93-96) resizes
to 288 x 144, takes TenCrop((256, 128)) and averages the ten crops' features.

Here the files are decoded on the GPU (ssg_amd.jpeg through `GpuBatchLoader`'s machinery), the transform is one kernel pair
(`preprocess_batch`, or `ten_crop_batch` = ssg_tencrop_u8 with test-time augmentation), the crops' mean is ssg_crop_mean_f32 and
the pooling is ssg_group_pool_f32 (csrc/tta.hip).  torchvision's crops 5..9 are windows of the mirrored image; when the horizontal
margin RW - CW is even they are the mirrors of crops (1, 0, 3, 2, 4), so on the ResNet family, whose stem kernel reads its input
mirrored on request (`ResNet._fmap(x, flip)`), only five crops exist in memory: `TestBatchLoader(tta=True)` yields a `FiveCrops`
block and `extract_feature_matrix` runs it twice.  InceptionNet, an odd margin, or tta='literal' take the ten materialised crops.
"""
import ctypes
import os
import os.path as osp
import time

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from .preprocessor import MEAN, STD, GpuBatchLoader, bilinear_coeffs, preprocess_batch

IMG_EXTENSIONS = ['.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm']       # test_dataset.py:7
FLIP_OF = (1, 0, 3, 2, 4)          # crop 5 + k of TenCrop = the mirror of crop FLIP_OF[k] (even horizontal margin)
MAT_FILES = (("trainID", "trainID"), ("queryID", "queryID"), ("trainCAM", "trainCAM"), ("queryCAM", "queryCAM"), ("testID", "testID"),
             ("testCAM", "testCAM"), ("Hist_train", "Hist_train"), ("Hist_query", "Hist_query"), ("Hist_test", "Hist_test"),
             ("Hist_query_max", "Hist_max"), ("Hist_query_avg", "Hist_avg"))        # (file stem, variable) of extract_feature.py:162-172


def is_image_file(filename):
    lower = filename.lower()
    return any(lower.endswith(ext) for ext in IMG_EXTENSIONS)


class TestDataset(object):
    """reid/test_dataset.py:64-92 with the decode left to the loader: the files of `root` sorted by name and filtered by the
    reference's extension list; items are `(the file's bytes, basename)` (raw=True: decoded on the GPU by `TestBatchLoader`) or
    `(uint8 HWC RGB array, basename)` (raw=False: Pillow, like the reference's pil_loader)."""
    __test__ = False        # not a pytest class, whatever its name says

    def __init__(self, root, raw=True):
        root = osp.expanduser(root)
        imgs = [osp.join(root, f) for f in sorted(os.listdir(root)) if is_image_file(f)]
        if len(imgs) == 0:
            raise RuntimeError("Found 0 images in subfolders of: " + root + "\n" "Supported image extensions are: " + ",".join(IMG_EXTENSIONS))
        self.root, self.imgs, self.raw = root, imgs, bool(raw)

    def __len__(self):
        return len(self.imgs)

    def __getitem__(self, index):
        path = self.imgs[index]
        if self.raw:
            with open(path, "rb") as f:
                return f.read(), osp.basename(path)
        from PIL import Image
        with open(path, "rb") as f:
            return np.asarray(Image.open(f).convert("RGB")), osp.basename(path)


def parse_market_name(fname):
    """(id, cam) of a Market-1501 file name, extract_feature.py:98-103: '-1_c3s1_...' -> (-1, 3), '0001_c1s1_...' -> (1, 1)"""
    if fname[0] == '-':
        return -1, int(fname[4])
    return int(fname[:4]), int(fname[6])


def crop_table(resize, crop):
    """(top, left) of torchvision's five_crop windows tl, tr, bl, br, centre in an image of `resize` = (RH, RW); the centre is
    int(round(margin / 2.0)) with Python's round-half-to-even (center_crop)"""
    (RH, RW), (CH, CW) = resize, crop
    return [(0, 0), (0, RW - CW), (RH - CH, 0), (RH - CH, RW - CW), (int(round((RH - CH) / 2.0)), int(round((RW - CW) / 2.0)))]


def ten_crop_batch(images_u8, resize=(288, 144), crop=(256, 128), mean=MEAN, std=STD, ncrops=10, device=None):
    """uint8 [B, h, w, 3] (decoded RGB images of one size) -> float32 CUDA [B, ncrops, 3, CH, CW] ==
    torch.stack([torch.stack([Normalize(mean, std)(ToTensor()(c)) for c in TenCrop(crop)(Resize(resize)(img))]) for img in images]);
    ncrops=5 stops after the five unmirrored crops.  Viewed as (-1, 3, CH, CW) it is the script's `imgs.view(-1, c, h, w)`."""
    L = _lib.lib()
    x = torch.as_tensor(images_u8)
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
        raise ValueError("expected uint8 images [B, h, w, 3] (RGB), got %r %r" % (x.dtype, tuple(x.shape)))
    (RH, RW), (CH, CW) = (int(v) for v in resize), (int(v) for v in crop)
    B, h, w, _ = x.shape
    if min(RH, RW, CH, CW, B, h, w) <= 0 or CH > RH or CW > RW or ncrops not in (5, 10):
        check(L.ssg_tencrop_u8(None, B, h, w, RH, RW, CH, CW, int(ncrops), (ctypes.c_int32 * 10)(), None, None, None, 1, None, None, None, 1,
                               (ctypes.c_float * 3)(), (ctypes.c_float * 3)(), None, None, None), "ssg_tencrop_u8")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    x = x.to(device).contiguous()
    tabs = []
    for n_in, n_out in ((w, RW), (h, RH)):
        first, count, kk = bilinear_coeffs(n_in, n_out)
        tabs.append((torch.from_numpy(first).to(device), torch.from_numpy(count).to(device), torch.from_numpy(kk).to(device).contiguous(), kk.shape[1]))
    tmp = torch.empty((B, h, RW, 3), dtype=torch.uint8, device=device)
    out = torch.empty((B, int(ncrops), 3, CH, CW), dtype=torch.float32, device=device)
    m3 = (ctypes.c_float * 3)(*[float(v) for v in mean]); s3 = (ctypes.c_float * 3)(*[float(v) for v in std])
    boxes = (ctypes.c_int32 * 10)(*[v for tl in crop_table((RH, RW), (CH, CW)) for v in tl])
    (xf, xc, xk, xks), (yf, yc, yk, yks) = tabs
    check(L.ssg_tencrop_u8(ptr(x), B, h, w, RH, RW, CH, CW, int(ncrops), boxes, ptr(xf), ptr(xc), ptr(xk), xks, ptr(yf), ptr(yc), ptr(yk), yks, m3, s3,
                           ptr(tmp), ptr(out), stream()), "ssg_tencrop_u8")
    return out


def crop_mean(block0, block1=None, table=None, tail=None):
    """the script's `outputs.view(bs, ncrops, -1).mean(1)` (:96) on the device: block0 [B, 5 | 10, D] and optionally block1 hold the
    crops' features, `table` lists (block, crop) in summation order (default: block0's crops in order).  -> [B, D], bit for bit what
    torch computes on the CPU for the rows in that order: a sequential float32 sum, with the last `tail` columns in the order of its
    scalar loop (default D % 32, the x86 builds of torch 2.x; see include/ssg_hip.h)."""
    L = _lib.lib()
    block0 = block0.contiguous()
    B, nc0, D = block0.shape
    nc1 = 0
    if block1 is not None:
        block1 = block1.contiguous()
        if block1.shape[0] != B or block1.shape[2] != D or block1.device != block0.device:
            raise ValueError("crop_mean: the two blocks differ in B, D or device: %r vs %r" % (tuple(block0.shape), tuple(block1.shape)))
        nc1 = block1.shape[1]
    if block0.dtype != torch.float32 or (block1 is not None and block1.dtype != torch.float32) or not block0.is_cuda:
        raise ValueError("crop_mean takes float32 CUDA feature blocks")
    table = [(0, c) for c in range(nc0)] if table is None else [(int(b), int(c)) for b, c in table]
    flat = (ctypes.c_int32 * (2 * len(table)))(*[v for bc in table for v in bc])
    out = torch.empty((B, D), dtype=torch.float32, device=block0.device)
    check(L.ssg_crop_mean_f32(ptr(block0), nc0, ptr(block1), nc1, B, D, flat, len(table), D % 32 if tail is None else int(tail), ptr(out), stream()),
          "ssg_crop_mean_f32")
    return out


class FiveCrops(object):
    """what `TestBatchLoader(tta=True)` yields in place of an image batch: `crops` [B, 5, 3, CH, CW], the unmirrored half of TenCrop.
    The marker `flip_of` obliges the consumer: crop 5 + k of the ten is the horizontal mirror of crops[:, flip_of[k]]."""
    flip_of = FLIP_OF

    def __init__(self, crops):
        self.crops = crops

    def ten(self):
        """the ten materialised crops [B, 10, 3, CH, CW] (a copy; the extraction never makes it)"""
        return torch.cat([self.crops, self.crops[:, list(self.flip_of)].flip(-1)], dim=1)


class _Items(object):
    """a TestDataset in the item layout GpuBatchLoader walks: (data, fname, pid, camid)"""

    def __init__(self, ds):
        self.ds, self.raw = ds, ds.raw
        self.dataset = [(osp.basename(p), 0, 0) for p in ds.imgs]

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        data, name = self.ds[i]
        return data, name, 0, 0


class TestBatchLoader(GpuBatchLoader):
    """Iterable replacement for the script's `DataLoader(TestDataset(root, transform), batch_size=64, shuffle=False)` (:59-76): yields
    `(imgs, fnames)` in name order, with GpuBatchLoader's GPU JPEG decode, one batch of lookahead and size bucketing.
      tta=False      imgs [B, 3, height, width]: Resize((height, width)) + ToTensor + Normalize (:41-45)
      tta=True       a `FiveCrops` block: Resize(resize) + the five unmirrored crops of TenCrop((height, width)); needs an even
                     horizontal margin (resize[1] - width), else crop 9 is no mirror of crop 4 -- ValueError
      tta='literal'  imgs [B, 10, 3, height, width]: the ten crops of :47-52
    resize defaults to the script's 9/8 of the crop, (288, 144) for (256, 128)."""
    __test__ = False

    def __init__(self, dataset_or_dir, height=256, width=128, batch_size=64, tta=False, resize=None, mean=MEAN, std=STD, device=None, decode="gpu"):
        if decode not in ("gpu", "pillow"):
            raise ValueError("decode must be 'gpu' or 'pillow'")
        if tta not in (False, True, "literal"):
            raise ValueError("tta must be False, True or 'literal'")
        ds = dataset_or_dir if isinstance(dataset_or_dir, TestDataset) else TestDataset(dataset_or_dir, raw=(decode == "gpu"))
        self.items = _Items(ds)
        self.decode = "gpu" if ds.raw else "pillow"
        self.height, self.width, self.batch_size, self.mean, self.std, self.device = int(height), int(width), int(batch_size), mean, std, device
        self.first, self.count = 0, len(self.items)
        self.tta = tta
        self.resize = (self.height * 9 // 8, self.width * 9 // 8) if resize is None else (int(resize[0]), int(resize[1]))
        if tta is True and (self.resize[1] - self.width) % 2:
            raise ValueError("tta=True keeps five crops and mirrors them in the stem; with the odd horizontal margin %d - %d TenCrop's crop 9 is "
                             "not the mirror of crop 4: use tta='literal'" % (self.resize[1], self.width))

    def _transform(self, pix, dev):
        if not self.tta:
            return preprocess_batch(pix, self.height, self.width, self.mean, self.std, dev)
        return ten_crop_batch(pix, self.resize, (self.height, self.width), self.mean, self.std, 5 if self.tta is True else 10, dev)

    def _finish(self, recs, pix, dev):
        names = [r[1] for r in recs]
        if torch.is_tensor(pix):                               # a batch of equally sized baseline files: one launch pair
            out = self._transform(pix, dev)
        else:
            lead = () if not self.tta else ((5,) if self.tta is True else (10,))
            out = torch.empty((len(recs),) + lead + (3, self.height, self.width), dtype=torch.float32, device=dev)
            by_size = {}
            for j, a in enumerate(pix):
                by_size.setdefault(tuple(a.shape[:2]), []).append(j)
            for js in by_size.values():
                batch = torch.stack([torch.as_tensor(pix[j]) for j in js]) if self.decode == "gpu" else np.stack([pix[j] for j in js])
                out[torch.as_tensor(js, device=dev)] = self._transform(batch, dev)
        return (FiveCrops(out) if self.tta is True else out), names


def _unwrap(model):
    from .evaluators import _check_model
    return _check_model(model)


def _features(m, x, flip=False):
    """what the script's extract_cnn_feature keeps of model(x): x1, the pooled map (ResNet) or the model's one tensor (InceptionNet);
    flip: of the mirrored images, through the flag of the input kernel"""
    from .inception import InceptionNet
    if isinstance(m, InceptionNet):
        if m.cut_at_pooling:
            raise ValueError("feature extraction needs a vector per image: cut_at_pooling=True returns the map")
        return m._features(x, flip)
    sets = m.pooled(*m._fmap(x, flip))
    return sets[0] if sets.shape[0] == 1 else sets.permute(1, 0, 2).reshape(sets.shape[1], -1)     # num_split > 1: for_eval's concatenation


def _two_streams(m, x, fn):
    """(fn(x, False), fn(x, True)) on the model's two side streams, as embed_with_flip runs its two orientations"""
    if not (m.flip_streams and m.precision == "split" and os.environ.get("SSG_FLIP_STREAMS", "1") != "0"):
        return fn(x, False), fn(x, True)
    cur = torch.cuda.current_stream(m.device)
    ready = torch.cuda.Event(); ready.record(cur)
    ab = []
    for st, flip in zip(m._side_streams(), (False, True)):
        st.wait_event(ready)
        with torch.cuda.stream(st):
            r = fn(x, flip)
        r.record_stream(cur)
        ab.append(r)
    for st in m._side_streams():
        cur.wait_stream(st)
    return ab


def _batch_features(m, imgs):
    """one loader item -> [B, D] CUDA features"""
    from .inception import InceptionNet
    if isinstance(imgs, FiveCrops):
        if isinstance(m, InceptionNet):      # no fused flip worth a second kind of launch there: the literal ten crops
            imgs = imgs.ten()
        else:
            x = imgs.crops.to(m.device, torch.float32)
            B, n = x.shape[:2]
            x = x.reshape((B * n,) + tuple(x.shape[2:]))
            a, b = _two_streams(m, x, lambda t, flip: _features(m, t, flip))
            table = [(0, c) for c in range(n)] + [(1, c) for c in imgs.flip_of]       # the script's order: crops 0..9
            return crop_mean(a.view(B, n, -1), b.view(B, n, -1), table)
    imgs = torch.as_tensor(imgs).to(m.device, torch.float32)
    if imgs.dim() == 5:                      # [B, 10, 3, h, w]: imgs.view(-1, c, h, w) -> model -> view(bs, ncrops, -1).mean(1)
        B, n = imgs.shape[:2]
        return crop_mean(_features(m, imgs.reshape((B * n,) + tuple(imgs.shape[2:]))).view(B, n, -1))
    return _features(m, imgs)


def extract_feature_matrix(model, data_loader, print_freq=1, tta=False):
    """extract_features without the per-row host copies: -> (features [N, D] CUDA float32, ids, cams, files).  `tta` states what the
    loader must yield (FiveCrops or ten-crop batches when true, plain batches when false); a mismatch is an error, not a guess.
    The split-half range flag is read once after the last batch (loaders that can be walked again; else per batch) and the whole
    set is recomputed on the fp32 twin if it is set, as extract_embeddings does."""
    m = _unwrap(model).eval()
    if tta and getattr(m, "num_split", 1) > 1:
        raise ValueError("tta with num_split = %d: the model returns a list of %d feature sets and the reference's "
                         "`outputs.view(bs, ncrops, -1)` (reid/extract_feature.py:96) has no list to view" % (m.num_split, m.num_split + 1))
    again = hasattr(data_loader, "__len__") and hasattr(data_loader, "listing") and hasattr(m, "_overflowed")

    def run(mm, deferred):
        chunks, files = [], []
        t0 = time.time()
        for i, (imgs, fnames) in enumerate(data_loader):
            crops = isinstance(imgs, FiveCrops) or torch.as_tensor(imgs).dim() == 5
            if crops != bool(tta):
                raise ValueError("extract_features(tta=%r) was handed %s" % (tta, "crop blocks" if crops else "plain image batches"))
            f = _batch_features(mm, imgs)
            if not deferred and mm._overflowed():
                f = _batch_features(mm._f32_twin(), imgs)
            chunks.append(f); files.extend(list(fnames))
            if print_freq and (i + 1) % print_freq == 0:
                print('Extract Features: [{}/{}]\tTime {:.3f}'.format(i + 1, len(data_loader) if hasattr(data_loader, "__len__") else -1, time.time() - t0))
        return chunks, files

    chunks, files = run(m, again)
    if again and m._overflowed():
        chunks.clear()
        chunks, files = run(m._f32_twin(), True)
    feats = torch.cat(chunks, dim=0)
    pairs = [parse_market_name(f) for f in files]
    return feats, [p[0] for p in pairs], [p[1] for p in pairs], files


def extract_features(model, data_loader, print_freq=1, tta=False):
    """Drop-in for reid/extract_feature.py:79-117: -> (features, ids, cams, files) with `features` a list of CPU float32 rows (numpy,
    like the script's `output.numpy()`); one device -> host copy for the whole set."""
    feats, ids, cams, files = extract_feature_matrix(model, data_loader, print_freq, tta)
    from . import hostio
    cpu = hostio.to_host(feats).numpy()
    return list(cpu), ids, cams, files


def group_index(fnames, query_files, key=lambda f: f[:7]):
    """host half of multi_query_pool: -> (order [M], offs [G + 1], qgroup [Q]) int32.  Groups are numbered in the order their key is
    first met among `fnames`; `order` lists the rows group by group, each group in the order its rows were met (the script's dict of
    lists, :141-144).  A query whose key has no row raises KeyError like the script's dict lookup (:150)."""
    gid, rows = {}, []
    for i, f in enumerate(fnames):
        k = key(f)
        if k not in gid:
            gid[k] = len(rows); rows.append([])
        rows[gid[k]].append(i)
    qgroup = np.array([gid[key(q)] for q in query_files], np.int32)
    order = np.array([i for r in rows for i in r], np.int32)
    offs = np.zeros(len(rows) + 1, np.int32)
    offs[1:] = np.cumsum([len(r) for r in rows])
    return order, offs, qgroup


def multi_query_pool(feats, fnames, query_files, key=lambda f: f[:7], return_normalized=False):
    """extract_feature.py:146-153 on the device: feats [M, D] (CUDA float32, or anything torch.as_tensor takes) are the gt_bbox
    features, fnames their file names; -> (Hist_max, Hist_avg) CUDA [Q, D], per query file the column-wise max and mean of the
    L2-normalised rows that share its key.  return_normalized adds the normalised rows [M, D]."""
    L = _lib.lib()
    order, offs, qgroup = group_index(fnames, query_files, key)
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.as_tensor(feats)
    x = (x if x.is_cuda else x.to(dev)).to(torch.float32).contiguous()
    M, D = x.shape
    if M != len(fnames):
        raise ValueError("multi_query_pool: %d feature rows, %d file names" % (M, len(fnames)))
    if len(query_files) == 0:
        raise ValueError("multi_query_pool: no query file")
    Q, G = len(qgroup), len(offs) - 1
    o, f, q = (torch.from_numpy(a).to(x.device) for a in (order, offs, qgroup))
    hmax = torch.empty((Q, D), dtype=torch.float32, device=x.device); havg = torch.empty_like(hmax)
    y = torch.empty_like(x) if return_normalized else None
    check(L.ssg_group_pool_f32(ptr(x), M, D, ptr(o), ptr(f), G, ptr(q), Q, ptr(hmax), ptr(havg), ptr(y), stream()), "ssg_group_pool_f32")
    return (hmax, havg, y) if return_normalized else (hmax, havg)


def _scores(title, qf, qid, qcam, gf, gid, gcam):
    from collections import OrderedDict
    from .evaluators import pairwise_distance_device
    from .ranking import evaluate_all
    feats = OrderedDict()
    query = [("q/%d" % i, qid[i], qcam[i]) for i in range(len(qid))]
    gallery = [("g/%d" % i, gid[i], gcam[i]) for i in range(len(gid))]
    for (k, _, _), row in zip(query, qf.unbind(0)):
        feats[k] = row
    for (k, _, _), row in zip(gallery, gf.unbind(0)):
        feats[k] = row
    print(title)
    return evaluate_all(pairwise_distance_device(feats, query, gallery), query=query, gallery=gallery)


def evaluate(model, train_dir, query_dir, multi_query_dir, gallery_dir, out_dir=None, tta=False, print_scores=True, batch_size=64, height=256,
             width=128, resize=None, print_freq=1):
    """reid/extract_feature.py:119-174 with the model already built and loaded: embeds the four folders, pools the multi-query
    descriptors and returns the script's eleven arrays by their .mat variable names (trainID, queryID, trainCAM, queryCAM, testID,
    testCAM, Hist_train, Hist_query, Hist_test, Hist_max, Hist_avg; numpy).  out_dir: also writes the eleven .mat files under the
    script's file names (needs scipy).  print_scores: mean AP / CMC for the single queries and for the max- and mean-pooled
    multi-queries against the gallery (the script leaves that step to MATLAB).  tta: False, True or 'literal' (TestBatchLoader)."""
    if out_dir is not None:
        try:
            import scipy.io as sio
        except ImportError as e:
            raise ImportError("evaluate(out_dir=...) writes .mat files with scipy.io.savemat, and scipy is not installed: %s" % e)
    m = _unwrap(model)
    from .inception import InceptionNet
    mode = tta
    if tta is True and (isinstance(m, InceptionNet) or (((height * 9 // 8, width * 9 // 8) if resize is None else resize)[1] - width) % 2):
        mode = "literal"                 # no fused flip (InceptionNet) or an odd margin: the ten crops, the same reference result

    def loader(d):
        return TestBatchLoader(d, height, width, batch_size, tta=mode, resize=resize)

    print('Extract train&single_query&gallery feature...')
    tr_f, tr_id, tr_cam, _ = extract_feature_matrix(m, loader(train_dir), print_freq, bool(tta))
    q_f, q_id, q_cam, q_files = extract_feature_matrix(m, loader(query_dir), print_freq, bool(tta))
    g_f, g_id, g_cam, _ = extract_feature_matrix(m, loader(gallery_dir), print_freq, bool(tta))
    print('Get multi_query feature...')
    mq_f, _, _, mq_files = extract_feature_matrix(m, loader(multi_query_dir), print_freq, bool(tta))
    hmax, havg = multi_query_pool(mq_f, mq_files, q_files)
    if print_scores:
        _scores("single query", q_f, q_id, q_cam, g_f, g_id, g_cam)
        _scores("multi query, max-pooled", hmax, q_id, q_cam, g_f, g_id, g_cam)
        _scores("multi query, mean-pooled", havg, q_id, q_cam, g_f, g_id, g_cam)
    from . import hostio
    res = dict(trainID=np.array(tr_id), queryID=np.array(q_id), trainCAM=np.array(tr_cam), queryCAM=np.array(q_cam), testID=np.array(g_id),
               testCAM=np.array(g_cam), Hist_train=hostio.to_host(tr_f).numpy(), Hist_query=hostio.to_host(q_f).numpy(),
               Hist_test=hostio.to_host(g_f).numpy(), Hist_max=hostio.to_host(hmax).numpy(), Hist_avg=hostio.to_host(havg).numpy())
    if out_dir is not None:
        print('Write to mat file...')
        os.makedirs(out_dir, exist_ok=True)
        for stem, var in MAT_FILES:
            sio.savemat(osp.join(out_dir, stem + ".mat"), {var: res[var]})
    return res
