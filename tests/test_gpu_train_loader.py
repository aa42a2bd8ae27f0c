"""GPU suite for the fine-tune training loader (ssg_amd.trainloader.GpuTrainLoader + csrc/train_transform.hip): the batches are the
reference DataLoader's bit for bit (tests/golden/train_loader_ref.npz), a ragged batch costs one transform call, a full 128-image
batch at 256 x 128 equals Pillow item by item, and with no flip / no erasing the kernel equals the extraction transform."""
import hashlib
import io
import random

import numpy as np
import pytest
import torch

import ssg_amd
from ssg_amd import jpeg
from ssg_amd import trainloader as tl
from ssg_amd.preprocessor import preprocess_batch
from make_golden_train_loader import host_item   # noqa: E402  (tools/ is on sys.path: tests/conftest.py)

pytestmark = pytest.mark.gpu


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _rng_hashes():
    st = np.random.get_state()
    return (_sha(torch.get_rng_state().numpy()), hashlib.sha256(st[1].tobytes() + repr(st[2:]).encode()).hexdigest(),
            hashlib.sha256(repr(random.getstate()).encode()).hexdigest())


def _seed(s):
    torch.manual_seed(s); np.random.seed(s); random.seed(s)


@pytest.fixture(scope="module")
def fx(golden, tmp_path_factory):
    g = golden("train_loader_ref.npz")
    d = tmp_path_factory.mktemp("train_loader")
    names = [str(n) for n in g["names"]]
    for i, n in enumerate(names):
        (d / n).write_bytes(g["file_%02d" % i].tobytes())
    ids, ids2, cams = g["ids"], g["ids2"], g["camids"]
    ds = {"list": [(n, [np.int64(ids[i]), np.int64(ids2[i])], 0) for i, n in enumerate(names)],
          "scalar": [(n, int(ids[i]), int(cams[i])) for i, n in enumerate(names)]}
    runs = [tuple(int(v) if v.isdigit() else v for v in str(r).split(",")) for r in g["runs"]]
    return g, str(d), ds, runs


@pytest.mark.parametrize("run,decode", [(0, "gpu"), (1, "gpu"), (2, "gpu"), (3, "gpu"), (4, "gpu"), (5, "gpu"), (3, "pillow")])
def test_batches_equal_reference_loader(fx, run, decode):
    """every batch of two epochs == the reference DataLoader's: fnames, each item's float32 bytes (sha256; the first batch in full),
    the collated labels, and the global generator states after each epoch; the golden's progressive file is decoded by Pillow and goes
    through the same kernel call as the GPU-decoded files of its batch"""
    g, root, dss, runs = fx
    kind, form, nw, flip_rng, seed = runs[run]
    H, W = (int(v) for v in g["out_hw"]); B, K = (int(v) for v in g["batch_k"])
    ds = dss[form]
    loader = ssg_amd.GpuTrainLoader(ds, root=root, transform=tl.TrainTransform(H, W, crop=kind, flip_rng=flip_rng), batch_size=B,
                                    num_instances=K, num_workers=nw, decode=decode)
    by_name = {r[0]: r for r in ds}
    _seed(seed)
    pillow0 = jpeg.stats["pillow"]
    for e in range(2):
        names, shas = g["fnames_%d_%d" % (run, e)], g["sha_%d_%d" % (run, e)]
        n = 0
        for k, (imgs, fnames, pids, camids) in enumerate(loader):
            assert imgs.is_cuda and imgs.dtype == torch.float32 and tuple(imgs.shape) == (B, 3, H, W)
            assert list(fnames) == [str(s) for s in names[k]]
            host = imgs.cpu().numpy()
            got = [_sha(host[j]) for j in range(B)]
            assert got == [str(s) for s in shas[k]], (run, e, k, [j for j in range(B) if got[j] != str(shas[k][j])])
            if e == 0 and k == 0 and ("first_%d" % run) in g.files:
                assert torch.equal(imgs.cpu(), torch.from_numpy(g["first_%d" % run]))
            recs = [by_name[f] for f in fnames]
            if form == "list":                   # FinedTrainer2._parse_data (reid/trainers.py:247-252) works on it unchanged
                assert isinstance(pids, list) and len(pids) == 2
                targets = [p.cuda() for p in pids]
                w = camids.float().cuda()
                assert targets[0].dtype == torch.int64 and w.shape == (B,)
                assert pids[0].tolist() == [int(r[1][0]) for r in recs] and pids[1].tolist() == [int(r[1][1]) for r in recs]
            else:
                assert pids.dtype == torch.int64 and pids.tolist() == [r[1] for r in recs]
            assert camids.dtype == torch.int64 and camids.tolist() == [r[2] for r in recs]
            n += 1
        assert n == len(names) == len(loader)
        assert _rng_hashes() == tuple(str(s) for s in g["rng_%d_%d" % (run, e)]), (run, e)
    if decode == "gpu":
        assert jpeg.stats["pillow"] > pillow0          # the progressive file went to Pillow, inside mixed batches


def _jpegs(tmp_path, sizes, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    names, blobs = [], []
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.clip(np.stack([xx * 255.0 / max(w - 1, 1), yy * 255.0 / max(h - 1, 1), (xx * 7 + yy * 3) % 256], -1) + rng.normal(0, 20, (h, w, 3)), 0, 255)
        buf = io.BytesIO()
        Image.fromarray(a.astype(np.uint8)).save(buf, "JPEG", quality=85, subsampling=i % 3)
        names.append("%05d.jpg" % i); blobs.append(buf.getvalue())
        (tmp_path / names[-1]).write_bytes(blobs[-1])
    return names, blobs


def _check_against_pillow(loader, ds, blobs, sizes, tf, seed, epochs=1):
    """the loader's batches == host_item (Pillow + numpy) of the draws of a TrainSchedule run from the same seeds"""
    _seed(seed)
    got = [(imgs.cpu().numpy(), fnames) for imgs, fnames, _, _ in loader]
    _seed(seed)
    sched = tl.TrainSchedule(ds, tf, loader.batch_size, loader.schedule.num_instances, loader.schedule.num_workers)
    exp = list(sched.epoch(sizes))
    assert len(got) == len(exp) > 0
    for (imgs, fnames), (idx, draws) in zip(got, exp):
        assert list(fnames) == [ds[i][0] for i in idx]
        for j, (i, d) in enumerate(zip(idx, draws)):
            ref = host_item(blobs[i], d, tf)
            assert np.array_equal(imgs[j], ref), (j, sizes[i], d, int((imgs[j] != ref).sum()))


def test_ragged_batch_is_one_kernel_call(tmp_path):
    """20 distinct source sizes (Market's 128 x 64, tall Duke-like, a very tall and an upscaled one) in ONE batch: one call of
    ssg_train_transform_u8, every item == Pillow"""
    sizes = [(128, 64), (256, 128), (214, 86), (301, 97), (180, 70), (263, 109), (96, 48), (150, 61), (330, 120), (240, 94), (77, 40),
             (199, 83), (275, 101), (142, 58), (222, 90), (310, 115), (900, 60), (40, 30), (163, 66), (251, 99)]
    names, blobs = _jpegs(tmp_path, sizes, 1)
    ds = [(n, i, 0) for i, n in enumerate(names)]           # one image per identity, K = 1: the batch holds every size once
    tf = tl.TrainTransform(256, 128, crop="random_rect")
    loader = ssg_amd.GpuTrainLoader(ds, root=str(tmp_path), transform=tf, batch_size=20, num_instances=1, num_workers=4)
    c0 = tl.calls["ssg_train_transform_u8"]
    _check_against_pillow(loader, ds, blobs, sizes, tf, 21)
    assert tl.calls["ssg_train_transform_u8"] - c0 == 1
    assert len(set(sizes)) >= 16


@pytest.mark.parametrize("crop", ["resize", "random_rect"])
def test_full_batch_256x128_equals_pillow(tmp_path, crop):
    """one 128-image batch (32 identities x K = 4, Duke-like ragged sizes) at the reference's 256 x 128: every item == Pillow + numpy"""
    rng = np.random.default_rng(8)
    sizes = [(int(h), int(w)) for h, w in zip(rng.integers(90, 420, 100), rng.integers(40, 160, 100))]
    names, blobs = _jpegs(tmp_path, sizes, 2)
    ds = [(n, [np.int64(i % 32)], 0) for i, n in enumerate(names)]
    tf = tl.TrainTransform(256, 128, crop=crop)
    loader = ssg_amd.GpuTrainLoader(ds, root=str(tmp_path), transform=tf, batch_size=128, num_instances=4, num_workers=4)
    assert len(loader) == 1
    _check_against_pillow(loader, ds, blobs, sizes, tf, 5)


def test_no_flip_no_erase_equals_preprocess_batch():
    """flip and erasing absent, whole-image windows, one source size: the new kernel == the extraction transform (ssg_preprocess_u8)"""
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(4)
    for (h, w), (H, W) in (((128, 64), (256, 128)), ((210, 77), (256, 128)), ((300, 310), (64, 32))):
        x = torch.randint(0, 256, (8, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
        tf = tl.TrainTransform(H, W, crop="resize", flip_p=None, erase_p=None)
        draws = [tl.ItemDraw((0, 0, w, h), False, None)] * 8
        got = tl.transform_batch([x[i] for i in range(8)], draws, tf, dev)
        ref = preprocess_batch(x, H, W, device=dev)
        assert torch.equal(got, ref), (h, w, H, W)
