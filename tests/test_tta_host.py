"""CPU suite of the test-time extraction (ssg_amd/extract_feature.py, csrc/tta.hip): the TenCrop restatement of tests/tta_ref.py against
Pillow's own crops in tests/golden/tta_multiquery_cases.npz (tools/make_golden_tta.py), the centre-crop rounding, the file-name rule,
TestDataset, the host index build of multi_query_pool, the classifier head's state dict, the recorded torch mean against its
restatement, and the three entry points' argument checks.  No GPU work."""
import ctypes
import os

import numpy as np
import pytest

import ssg_amd
import tta_ref as ref
from ssg_amd import _lib, extract_feature as xf

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gold():
    return np.load(ref.GOLDEN)


@pytest.mark.parametrize("name", ref.FULL)
def test_crops_are_pillows_crops(gold, name):
    """the numpy-slice restatement == Image.crop / Image.transpose(FLIP_LEFT_RIGHT), and its normalisation == torch's float32 ops"""
    _, _, _, resize, crop, _ = ref.GEOMETRIES[name]
    resized = gold[name + "_resized"]
    assert resized.shape[1:3] == resize
    mine = np.stack([ref.ten_crop_u8(im, crop) for im in resized])
    assert np.array_equal(mine, gold[name + "_crops_u8"])
    assert np.array_equal(ref.ten_crop_reference(resized, crop), gold[name + "_tencrop"])
    # the mirrored half: the four corners mirror crops (1, 0, 3, 2); the centre mirrors the centre only with an even horizontal margin
    for k, p in enumerate(ref.FLIP_OF):
        if k < 4 or (resize[1] - crop[1]) % 2 == 0:
            assert np.array_equal(mine[:, 5 + k], mine[:, p, :, ::-1])
    if (resize[1] - crop[1]) % 2:
        top, left = ref.crop_boxes(*resize, *crop)[4]
        other = resize[1] - crop[1] - left                          # the window of the image whose mirror crop 9 is
        assert abs(other - left) == 1
        assert np.array_equal(mine[:, 9], resized[:, top:top + crop[0], other:other + crop[1]][:, :, ::-1])


def test_fixture_resized_images_are_pillows(gold):
    """the seeded sources still resize to the stored images with the installed Pillow (the large geometries keep nothing else)"""
    for name, (B, h, w, resize, _, _) in ref.GEOMETRIES.items():
        src = ref.source_images(name)
        assert src.shape == (B, h, w, 3) and src.dtype == np.uint8
        assert np.array_equal(np.stack([ref.pil_resize(im, resize) for im in src]), gold[name + "_resized"]), name


@pytest.mark.parametrize("margins,want", [((9, 9), (4, 4)), ((7, 7), (4, 4)), ((32, 16), (16, 8))])
def test_centre_crop_rounding(margins, want):
    """int(round(m / 2.0)) with Python's round: 4.5 -> 4, 3.5 -> 4"""
    CH, CW = 32, 16
    RH, RW = CH + margins[0], CW + margins[1]
    assert (ref.centre_offset(RH, CH), ref.centre_offset(RW, CW)) == want
    table = xf.crop_table((RH, RW), (CH, CW))
    assert table == ref.crop_boxes(RH, RW, CH, CW)
    assert table == [(0, 0), (0, margins[1]), (margins[0], 0), margins, want]


def test_parse_market_name():
    assert xf.parse_market_name("0001_c1s1_001051_00.jpg") == (1, 1)
    assert xf.parse_market_name("-1_c3s1_000401_03.jpg") == (-1, 3)
    assert xf.parse_market_name("1501_c6s4_001902_01.jpg") == (1501, 6)
    assert ssg_amd.parse_market_name is xf.parse_market_name


def test_test_dataset(tmp_path):
    from PIL import Image
    d = tmp_path / "imgs"
    d.mkdir()
    with pytest.raises(RuntimeError, match="Found 0 images"):
        xf.TestDataset(str(d))
    (d / "notes.txt").write_text("x")
    (d / "sub").mkdir()
    with pytest.raises(RuntimeError, match="Found 0 images"):
        xf.TestDataset(str(d))
    rng = np.random.default_rng(0)
    for f in ("0002_c1s1_000001_00.jpg", "0001_c2s1_000001_00.JPG", "-1_c3s1_000401_03.jpg", "0003_c1s1_000001_00.png", "0004_c1s1_000001_00.gif"):
        Image.fromarray(rng.integers(0, 255, (16, 8, 3), dtype=np.uint8)).save(str(d / f))
    ds = xf.TestDataset(str(d))
    names = [os.path.basename(p) for p in ds.imgs]
    assert names == sorted(["0002_c1s1_000001_00.jpg", "0001_c2s1_000001_00.JPG", "-1_c3s1_000401_03.jpg", "0003_c1s1_000001_00.png"])   # no .gif, no .txt
    assert len(ds) == 4 and ssg_amd.TestDataset is xf.TestDataset
    data, name = ds[1]
    assert name == names[1] and isinstance(data, bytes) and data == open(ds.imgs[1], "rb").read()
    arr, name = xf.TestDataset(str(d), raw=False)[3]
    assert name == names[3] and arr.dtype == np.uint8 and arr.shape == (16, 8, 3)
    assert np.array_equal(arr, np.asarray(Image.open(ds.imgs[3]).convert("RGB")))
    # the loader is built without touching a device; an odd horizontal margin cannot keep five crops
    ld = xf.TestBatchLoader(ds, batch_size=3)
    assert len(ld) == 2 and ld.listing()[0] == names and ld.resize == (288, 144)
    with pytest.raises(ValueError, match="odd horizontal margin"):
        xf.TestBatchLoader(ds, height=144, width=56, tta=True)
    assert xf.TestBatchLoader(ds, height=144, width=56, tta="literal").resize == (162, 63)


def test_group_index():
    names = ["0002_c1s1_a", "0001_c1s1_a", "0002_c1s2_b", "0003_c4s1_a", "0001_c1s3_c", "0002_c1s9_z"]         # interleaved groups
    order, offs, qgroup = xf.group_index(names, ["0001_c1s1_q", "0003_c4s2_q", "0001_c1s2_q", "0002_c1s1_q"])     # a repeated key
    assert order.dtype == offs.dtype == qgroup.dtype == np.int32
    assert order.tolist() == [0, 2, 5, 1, 4, 3] and offs.tolist() == [0, 3, 5, 6] and qgroup.tolist() == [1, 2, 1, 0]
    with pytest.raises(KeyError):
        xf.group_index(names, ["0001_c1s1_q", "0009_c1s1_q"])
    o2, f2, q2 = xf.group_index(names, ["0002"], key=lambda f: f[:4])
    assert f2.tolist() == [0, 3, 5, 6] and q2.tolist() == [0]
    # the seeded pool case: the index build gives the groups of the script's dict of lists
    for case in ref.POOL_CASES:
        _, rows, queries = ref.pool_case(case)
        order, offs, qgroup = xf.group_index(rows, queries)
        groups = ref.group_rows(rows, queries)
        assert sorted(len(g) for g in groups) == [1, 2, 7, 7, 13] and len(offs) == 5
        for q, g in enumerate(groups):
            assert order[offs[qgroup[q]]:offs[qgroup[q] + 1]].tolist() == g


def test_classifier_head_state_dict():
    with pytest.warns(UserWarning):
        m = ssg_amd.create("resnet50", dropout=0.0, num_features=2048, num_classes=632)      # the script's model (:124)
    sd = m.state_dict()
    assert tuple(sd["classifier_x2.weight"].shape) == (632, 2048) and tuple(sd["classifier_x2.bias"].shape) == (632,)
    assert list(sd)[-2:] == ["classifier_x2.weight", "classifier_x2.bias"]
    assert float(sd["classifier_x2.bias"].abs().max()) == 0.0 and 0.0008 < float(sd["classifier_x2.weight"].std()) < 0.0012
    base = ssg_amd.create("resnet50", pretrained=False, num_features=2048, num_classes=0).state_dict()
    assert list(base) == list(sd)[:-2] and all(torch.equal(base[k], sd[k]) for k in base)      # every other tensor is the num_classes=0 one
    assert "classifier_x2.weight" not in ssg_amd.synthetic_state_dict(seed=1)
    m.load_state_dict({k: v + 1 if k == "classifier_x2.bias" else v for k, v in sd.items()})
    assert float(m.state_dict()["classifier_x2.bias"].min()) == 1.0
    with pytest.raises(ValueError, match="num_features must be positive"):
        ssg_amd.create("resnet50", pretrained=False, num_features=0, num_classes=632)
    with pytest.raises(NotImplementedError):
        m.train()
    with pytest.raises(NotImplementedError, match="training-only path"):
        ssg_amd.create("inception", num_classes=632)


@pytest.mark.parametrize("case", list(ref.MEAN_CASES))
def test_recorded_torch_mean_is_the_restated_order(gold, case):
    x = ref.mean_inputs(case)
    D = x.shape[2]
    rec = gold["mean_" + case]
    assert np.array_equal(rec, ref.torch_mean(x, ref.mean_tail(D)))
    V = D - ref.mean_tail(D)
    assert np.array_equal(rec[:, :V], ref.sequential_mean(x)[:, :V])          # the vectorised columns: the plain ascending sum
    assert (rec != x.astype(np.float64).mean(1).astype(np.float32)).mean() > 0.3      # and not the rounded float64 mean


def test_recorded_pool_arrays_unpack(gold):
    """the fixture's step counts rebuild float32 arrays near the float64 restatement (sklearn's float32 rows: a few steps off)"""
    for case in ref.POOL_CASES:
        x, rows, queries = ref.pool_case(case)
        t = ref.normalize64(x)
        y = ref.unpack_steps(gold["pool_%s_y" % case], t)
        assert y.dtype == np.float32 and y.shape == x.shape and np.all(y[ref.POOL_ZERO_ROW] == 0)
        assert np.abs(y - t).max() <= 4 * 2.0 ** -24 * np.abs(t).max()
        groups = ref.group_rows(rows, queries)
        assert np.array_equal(ref.unpack_steps(gold["pool_%s_max" % case], ref.pool64(t, groups)[0]), np.stack([y[g].max(axis=0) for g in groups]))
        assert np.array_equal(ref.unpack_steps(gold["pool_%s_avg" % case], ref.pool64(t, groups)[1]), np.stack([y[g].mean(axis=0) for g in groups]))


def test_entry_points_refuse_bad_arguments():
    """SSG_ERR_INVALID with a message, before any device call"""
    L = _lib.lib()
    boxes = (ctypes.c_int32 * 10)(0, 0, 0, 16, 32, 0, 32, 16, 16, 8)
    m3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)

    def tencrop(B=2, h=128, w=64, RH=288, RW=144, CH=256, CW=128, ncrops=10, boxes=boxes):
        return L.ssg_tencrop_u8(None, B, h, w, RH, RW, CH, CW, ncrops, boxes, None, None, None, 3, None, None, None, 3, m3, m3, None, None, None)

    assert tencrop() == -1 and b"NULL" in L.ssg_last_error()                       # the shapes pass, the pointers do not
    assert tencrop(CH=289) == -1 and b"larger than the resized image" in L.ssg_last_error()
    assert tencrop(CW=145) == -1 and b"larger than the resized image" in L.ssg_last_error()
    for n in (0, 4, 6, 9, 11):
        assert tencrop(ncrops=n) == -1 and b"ncrops must be 5 or 10" in L.ssg_last_error()
    for kw in (dict(B=0), dict(h=0), dict(w=-1), dict(RH=0), dict(CW=0), dict(boxes=None)):
        assert tencrop(**kw) == -1 and b"bad shape" in L.ssg_last_error()
    outside = (ctypes.c_int32 * 10)(0, 0, 0, 17, 32, 0, 32, 16, 16, 8)             # tr one column too far right
    assert tencrop(boxes=outside) == -1 and b"leaves the resized image" in L.ssg_last_error()
    with pytest.raises(ValueError, match="ncrops must be 5 or 10"):
        xf.ten_crop_batch(np.zeros((1, 8, 8, 3), np.uint8), (9, 9), (8, 8), ncrops=7)
    with pytest.raises(ValueError, match="larger than the resized image"):
        xf.ten_crop_batch(np.zeros((1, 8, 8, 3), np.uint8), (9, 9), (10, 8))
    with pytest.raises(ValueError, match="uint8 images"):
        xf.ten_crop_batch(np.zeros((1, 8, 8, 3), np.float32))

    table = (ctypes.c_int32 * 20)(*[v for c in range(10) for v in (0, c)])
    assert L.ssg_crop_mean_f32(None, 10, None, 0, 3, 70, table, 10, 6, None, None) == -1 and b"NULL" in L.ssg_last_error()
    for args in ((None, 10, None, 0, 0, 70, table, 10, 0), (None, 10, None, 0, 3, 0, table, 10, 0), (None, 7, None, 0, 3, 70, table, 10, 0),
                 (None, 10, None, 0, 3, 70, table, 0, 0), (None, 10, None, 0, 3, 70, table, 16, 0), (None, 10, None, 0, 3, 70, table, 10, 71),
                 (None, 10, None, 0, 3, 70, None, 10, 0)):
        assert L.ssg_crop_mean_f32(*args, None, None) == -1 and b"bad arguments" in L.ssg_last_error(), args
    assert L.ssg_crop_mean_f32(None, 5, None, 0, 3, 70, table, 10, 0, None, None) == -1 and b"names no source row" in L.ssg_last_error()      # crop 5 of 5
    two = (ctypes.c_int32 * 4)(0, 0, 1, 0)
    assert L.ssg_crop_mean_f32(None, 5, None, 5, 3, 70, two, 2, 0, None, None) == -1 and b"names no source row" in L.ssg_last_error()         # block 1 without src1

    for args in ((0, 64, 1, 1), (4, 0, 1, 1), (4, 64, 0, 1), (4, 64, 1, 0), (4, 64, 5, 1)):
        M, D, G, Q = args
        assert L.ssg_group_pool_f32(None, M, D, None, None, G, None, Q, None, None, None, None) == -1 and b"bad shape" in L.ssg_last_error()
    assert L.ssg_group_pool_f32(None, 4, 64, None, None, 2, None, 3, None, None, None, None) == -1 and b"NULL" in L.ssg_last_error()
