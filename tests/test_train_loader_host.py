"""CPU suite for the fine-tune training loader (ssg_amd.trainloader): the host schedule against what the reference's DataLoader handed
out (tests/golden/train_loader_ref.npz, tools/make_golden_train_loader.py), the vectorised Pillow coefficient tables, the transform
spec read from a Compose, and the argument checks of ssg_train_transform_u8 -- no GPU."""
import hashlib
import io
import random

import numpy as np
import pytest
import torch

from ssg_amd import _lib
from ssg_amd import trainloader as tl
from ssg_amd.preprocessor import bilinear_coeffs
from make_golden_train_loader import host_item   # noqa: E402  (tools/ is on sys.path: tests/conftest.py)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _rng_hashes():
    st = np.random.get_state()
    return (_sha(torch.get_rng_state().numpy()), hashlib.sha256(st[1].tobytes() + repr(st[2:]).encode()).hexdigest(),
            hashlib.sha256(repr(random.getstate()).encode()).hexdigest())


class Fixture(object):
    def __init__(self, g):
        from PIL import Image
        self.g = g
        self.names = [str(n) for n in g["names"]]
        self.blobs = [g["file_%02d" % i] for i in range(len(self.names))]
        self.sizes = [Image.open(io.BytesIO(bytes(b))).size[::-1] for b in self.blobs]
        ids, ids2, cams = g["ids"], g["ids2"], g["camids"]
        self.datasets = {"list": [(n, [np.int64(ids[i]), np.int64(ids2[i])], 0) for i, n in enumerate(self.names)],
                         "scalar": [(n, int(ids[i]), int(cams[i])) for i, n in enumerate(self.names)]}
        self.H, self.W = (int(v) for v in g["out_hw"])
        self.batch, self.K = (int(v) for v in g["batch_k"])
        self.runs = []
        for r in g["runs"]:
            kind, form, nw, flip_rng, seed = str(r).split(",")
            self.runs.append((kind, form, int(nw), flip_rng, int(seed)))

    def transform(self, kind, flip_rng):
        return tl.TrainTransform(self.H, self.W, crop=kind, flip_rng=flip_rng)


@pytest.fixture(scope="module")
def fx(golden):
    return Fixture(golden("train_loader_ref.npz"))


@pytest.mark.parametrize("run", range(6))
def test_schedule_reproduces_reference_loader(fx, run):
    """fnames of every batch, every item rebuilt from its draws with Pillow + numpy (sha256 of the float32 tensor) and the global
    torch / numpy / python generator states after each epoch == the reference's DataLoader, both label forms, workers 0 / 4, 2 epochs"""
    kind, form, nw, flip_rng, seed = fx.runs[run]
    ds = fx.datasets[form]
    tf = fx.transform(kind, flip_rng)
    sched = tl.TrainSchedule(ds, tf, batch_size=fx.batch, num_instances=fx.K, num_workers=nw)
    torch.manual_seed(seed); np.random.seed(seed); random.seed(seed)
    for e in range(2):
        names, shas = fx.g["fnames_%d_%d" % (run, e)], fx.g["sha_%d_%d" % (run, e)]
        n = 0
        for k, (idx, draws) in enumerate(sched.epoch(fx.sizes)):
            assert [ds[i][0] for i in idx] == [str(s) for s in names[k]], (run, e, k)
            for j, (i, d) in enumerate(zip(idx, draws)):
                t = host_item(fx.blobs[i], d, tf)
                assert _sha(t) == str(shas[k][j]), (run, e, k, j, d)
                if e == 0 and k == 0 and ("first_%d" % run) in fx.g.files:
                    assert np.array_equal(t, fx.g["first_%d" % run][j])
            n += 1
        assert n == len(names) == len(sched)
        assert _rng_hashes() == tuple(str(s) for s in fx.g["rng_%d_%d" % (run, e)]), (run, e)


def test_schedule_draws_both_crop_branches_and_the_replace_branch(fx):
    """the fixture exercises what it is meant to: random crops that are not the whole image, erased and kept items, flips, identities
    with fewer than K images drawn with replacement (an index repeated inside one identity's K)"""
    torch.manual_seed(14); np.random.seed(14); random.seed(14)
    sched = tl.TrainSchedule(fx.datasets["scalar"], fx.transform("random_rect", "torch"), fx.batch, fx.K, 4)
    draws = [d for _, ds in sched.epoch(fx.sizes) for d in ds]
    assert any(d.box != (0, 0, fx.sizes[0][1], fx.sizes[0][0]) for d in draws)
    assert any(d.erase is not None for d in draws) and any(d.erase is None for d in draws)
    assert any(d.flip for d in draws) and not all(d.flip for d in draws)
    rep = False
    for idx, _ in tl.TrainSchedule(fx.datasets["scalar"], fx.transform("resize", "torch"), fx.batch, fx.K, 0).epoch(fx.sizes):
        for q in range(0, len(idx), fx.K):
            rep = rep or len(set(idx[q:q + fx.K])) < fx.K
    assert rep


def test_worker_emulation_leaves_process_generators_alone(fx):
    """num_workers > 0: the transforms draw from private generators; the process's python generator is not consumed at all"""
    random.seed(3); torch.manual_seed(3); np.random.seed(3)
    before = random.getstate()
    for _ in tl.TrainSchedule(fx.datasets["list"], fx.transform("random_rect", "python"), fx.batch, fx.K, 4).epoch(fx.sizes):
        pass
    assert random.getstate() == before


def test_vectorised_coefficients_equal_bilinear_coeffs():
    rng = np.random.default_rng(3)
    pairs = [(128, 256), (64, 128), (256, 256), (301, 256), (97, 128), (1, 5), (5, 1), (1000, 64), (64, 32), (33, 384)]
    pairs += [(int(a), int(b)) for a, b in zip(rng.integers(1, 700, 300), rng.integers(1, 400, 300))]
    for a, b in pairs:
        tl._coeff_cache.pop((a, b), None)
        f, c, k = tl.bilinear_coeffs_np(a, b)
        rf, rc, rk = bilinear_coeffs(a, b)
        assert np.array_equal(f, rf) and np.array_equal(c, rc) and np.array_equal(k, rk), (a, b)
        assert k.dtype == np.int32 and f.dtype == np.int32 and c.dtype == np.int32


class RandomSizedRectCrop(object):          # attribute-level stand-ins of the reference's classes (reid/utils/data/transforms.py)
    def __init__(self, height, width, interpolation=2):
        self.height, self.width, self.interpolation = height, width, interpolation


class RandomErasing(object):
    def __init__(self, probability=0.5, sl=0.02, sh=0.4, r1=0.3, mean=(0.4914, 0.4822, 0.4465)):
        self.probability, self.sl, self.sh, self.r1, self.mean = probability, sl, sh, r1, list(mean)


def _tv():
    """torchvision-shaped stand-ins (attributes of torchvision.transforms)"""
    ns = {}
    ns["Resize"] = type("Resize", (), {"__init__": lambda s, size, interpolation=2: (setattr(s, "size", size), setattr(s, "interpolation", interpolation))[0]})
    ns["RandomHorizontalFlip"] = type("RandomHorizontalFlip", (), {"__init__": lambda s, p=0.5: setattr(s, "p", p)})
    ns["ToTensor"] = type("ToTensor", (), {})
    ns["Normalize"] = type("Normalize", (), {"__init__": lambda s, mean, std: (setattr(s, "mean", mean), setattr(s, "std", std))[0]})
    ns["Compose"] = type("Compose", (), {"__init__": lambda s, t: setattr(s, "transforms", t)})
    ns["TvRandomErasing"] = type("RandomErasing", (), {"__init__": lambda s, p=0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3), value=0:
                                                       (setattr(s, "p", p), setattr(s, "scale", scale), setattr(s, "ratio", ratio), setattr(s, "value", value))[0]})
    ns["ColorJitter"] = type("ColorJitter", (), {})
    return type("T", (), ns)


def test_from_compose_reads_the_reference_pipelines():
    T = _tv()
    norm = T.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
    st = tl.TrainTransform.from_compose(T.Compose([T.Resize((256, 128)), T.RandomHorizontalFlip(), T.ToTensor(), norm,
                                                   RandomErasing(probability=0.5, sh=0.2, r1=0.3)]))     # selftraining.py:177-183
    assert (st.height, st.width, st.crop, st.flip_p, st.flip_rng, st.erase_p, st.sl, st.sh, st.r1) == (256, 128, "resize", 0.5, "torch", 0.5, 0.02, 0.2, 0.3)
    assert st.mean == (0.485, 0.456, 0.406) and st.std == (0.229, 0.224, 0.225) and st.erase_fill == (0.4914, 0.4822, 0.4465)
    eug = tl.TrainTransform.from_compose(T.Compose([RandomSizedRectCrop(256, 128), T.RandomHorizontalFlip(), T.ToTensor(), norm,
                                                    RandomErasing(probability=0.5, sh=0.2, r1=0.3)]), flip_rng="python")   # reid/eug.py:64-71
    assert (eug.crop, eug.height, eug.width, eug.flip_rng) == ("random_rect", 256, 128, "python")
    bare = tl.TrainTransform.from_compose(T.Compose([T.Resize((64, 32)), T.ToTensor()]))
    assert bare.flip_p is None and bare.erase_p is None and bare.mean == (0.0, 0.0, 0.0) and bare.std == (1.0, 1.0, 1.0)


@pytest.mark.parametrize("bad", ["tv_erasing", "jitter", "int_size", "nearest", "order", "no_totensor"])
def test_from_compose_rejects_unsupported(bad):
    T = _tv()
    norm = T.Normalize(mean=[0.5] * 3, std=[0.5] * 3)
    pipe = {"tv_erasing": [T.Resize((256, 128)), T.ToTensor(), norm, T.TvRandomErasing()],
            "jitter": [T.Resize((256, 128)), T.ColorJitter(), T.ToTensor()],
            "int_size": [T.Resize(256), T.ToTensor()],
            "nearest": [T.Resize((256, 128), interpolation=0), T.ToTensor()],
            "order": [T.Resize((256, 128)), T.ToTensor(), T.RandomHorizontalFlip()],
            "no_totensor": [T.Resize((256, 128)), T.RandomHorizontalFlip()]}[bad]
    with pytest.raises(ValueError) as e:
        tl.TrainTransform.from_compose(T.Compose(pipe))
    if bad in ("tv_erasing", "jitter"):
        assert ("RandomErasing" if bad == "tv_erasing" else "ColorJitter") in str(e.value)


def test_transform_entry_rejects_bad_arguments_without_gpu():
    import ctypes
    L = _lib.lib()
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    d = ctypes.c_void_p(16)
    assert L.ssg_train_transform_u8(None, 4, d, 256, 128, 32, 40, f3, f3, f3, d, None) == -1              # no descriptor table
    assert b"ssg_train_transform_u8" in L.ssg_last_error()
    assert L.ssg_train_transform_u8(d, 0, d, 256, 128, 32, 40, f3, f3, f3, d, None) == -1                 # empty batch
    assert L.ssg_train_transform_u8(d, 4, d, 256, 128, 300, 40, f3, f3, f3, d, None) == -1                # band taller than the output
    assert L.ssg_train_transform_u8(d, 4, d, 256, 128, 32, 0, f3, f3, f3, d, None) == -1                  # no LDS rows
    assert L.ssg_train_transform_u8(d, 4, d, 256, 128, 32, 200, f3, f3, f3, d, None) == -1                # 200 x 128 x 3 > 64 KiB
    assert b"LDS" in L.ssg_last_error()
    assert L.ssg_train_transform_u8(d, 4, d, 256, 128, 32, 40, None, f3, f3, d, None) == -1               # no mean


def test_loader_surface_without_gpu(fx):
    import ssg_amd
    assert ssg_amd.GpuTrainLoader is tl.GpuTrainLoader and ssg_amd.TrainTransform is tl.TrainTransform
    assert ssg_amd.generate_dataloader is tl.generate_dataloader
    ld = ssg_amd.GpuTrainLoader(fx.datasets["list"], root="/nonexistent", transform=fx.transform("resize", "torch"), batch_size=8,
                                num_instances=4)
    assert len(ld) == 5            # 10 identities x K = 4 // 8, drop_last
    with pytest.raises(ValueError):
        ssg_amd.GpuTrainLoader(fx.datasets["list"], transform=None)
    from ssg_amd.eug import EUGTrainLoaderMixin

    class Base(object):
        def get_dataloader(self, dataset, training=False):
            return ("base", training)

    class E(EUGTrainLoaderMixin, Base):
        data_height, data_width, batch_size, num_classes, num_instances, data_workers = 64, 32, 8, 0, 4, 4
    ld = E().get_dataloader(fx.datasets["scalar"], training=True)
    assert isinstance(ld, tl.GpuTrainLoader) and ld.transform.crop == "random_rect" and (ld.transform.height, ld.transform.width) == (64, 32)
    assert ld.schedule.num_workers == 4 and len(ld) == 5
    assert E().get_dataloader(fx.datasets["scalar"], training=False) == ("base", False)
    E.num_classes = 10
    assert E().get_dataloader(fx.datasets["scalar"], training=True) == ("base", True)
