"""GPU suite of the test-time extraction (csrc/tta.hip, ssg_amd/extract_feature.py) against tests/golden/tta_multiquery_cases.npz
(tools/make_golden_tta.py) and the restatements of tests/tta_ref.py.

Ten-crop: bit for bit Pillow's resize + torchvision's TenCrop + ToTensor + Normalize.  The mirrored half is the mirror of crops
(1, 0, 3, 2, 4) for the four corners always and for the centre when the horizontal margin is even; with the odd margins of `odd9` /
`odd7` torchvision's crop 9 is the mirror of the window one pixel beside the centre crop (tests/tta_ref.py), which is asserted instead.

Crop mean: bit for bit torch's CPU `x.view(B, n, -1).mean(1)`.

Group pool.  t = the float64 restatement.  Normalised rows: one rounding of a float64 quotient away from t.  out_max / out_avg: bit for
bit np.max / np.mean(axis=0) of the device's own normalised rows.  Against the recorded sklearn / numpy float32 results: for the max,
element by element, the recorded value's own distance to t plus 2^-23 |t|; for the mean, the recorded row's WORST distance to t plus
2^-23 |t| -- the error of a float32 sum belongs to the group's summation (m additions of values of one magnitude) and is realised
differently in every column: a column in which numpy's sum happens to round to the exact value says nothing about the next one, so
the recorded error is taken over the query's row (it still comes from the fixture alone).  Measured on the MI355X, worst device error
over its bound: see each test's printed figure (pytest -s); the figures are repeated in profiles/tta_times.txt.

Fused route: five crops, each run unmirrored and mirrored by the stem kernel, against ten materialised crops through model(x).
"""
import contextlib
import io
import os

import numpy as np
import pytest

import ssg_amd
import tta_ref as ref
from ssg_amd import extract_feature as xf
from train_common import U, bound

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def gold():
    return np.load(ref.GOLDEN)


@pytest.fixture(scope="module")
def model50(dev):
    """the script's model (extract_feature.py:124) with seeded weights and a non-zero classifier bias"""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = ssg_amd.create("resnet50", dropout=0.0, num_features=2048, num_classes=632, seed=1)
    sd = m.state_dict()
    sd["classifier_x2.bias"] = torch.randn(632, generator=torch.Generator().manual_seed(5)) * 0.01
    m.load_state_dict(sd)
    return m.cuda().eval()


# ---------------------------------------------------------------------------------------------------------------- ssg_tencrop_u8

@pytest.mark.parametrize("name", list(ref.GEOMETRIES))
def test_ten_crop_is_the_reference_chain(dev, gold, name):
    _, _, _, resize, crop, _ = ref.GEOMETRIES[name]
    src = ref.source_images(name)
    want = gold[name + "_tencrop"] if name in ref.FULL else ref.ten_crop_reference(gold[name + "_resized"], crop)
    ten = xf.ten_crop_batch(src, resize, crop, ncrops=10)
    assert ten.is_cuda and ten.dtype == torch.float32 and tuple(ten.shape) == want.shape
    got = ten.cpu().numpy()
    assert np.array_equal(got, want)
    five = xf.ten_crop_batch(torch.from_numpy(src).to(dev), resize, crop, ncrops=5)
    assert tuple(five.shape) == (src.shape[0], 5, 3) + crop and torch.equal(five, ten[:, :5])
    even = (resize[1] - crop[1]) % 2 == 0
    for k, p in enumerate(ref.FLIP_OF):
        if k < 4 or even:
            assert torch.equal(ten[:, 5 + k], ten[:, p].flip(-1)), (name, k)
    if even:
        assert torch.equal(xf.FiveCrops(five).ten(), ten)
    else:       # crop 9 mirrors the window beside the centre crop: rebuild it from the resized image
        top, left = ref.crop_boxes(*resize, *crop)[4]
        other = resize[1] - crop[1] - left
        win = gold[name + "_resized"][:, top:top + crop[0], other:other + crop[1]][:, :, ::-1]
        assert np.array_equal(got[:, 9], ref.to_tensor_normalize(win))
    if name == "same":
        assert all(torch.equal(ten[:, k], ten[:, 0]) for k in range(5)) and all(torch.equal(ten[:, k], ten[:, 5]) for k in range(5, 10))
        assert np.array_equal(got[:, 0], ssg_amd.preprocess_batch(src, *resize).cpu().numpy())        # no crop at all: the extraction transform


# ------------------------------------------------------------------------------------------------------------- ssg_crop_mean_f32

@pytest.mark.parametrize("case", list(ref.MEAN_CASES))
def test_crop_mean_is_torchs_mean(dev, gold, case):
    x = ref.mean_inputs(case)
    B, n, D = x.shape
    xd = torch.from_numpy(x).to(dev)
    one = xf.crop_mean(xd)
    assert np.array_equal(one.cpu().numpy(), gold["mean_" + case])
    assert np.array_equal(xf.crop_mean(xd, tail=0).cpu().numpy(), ref.sequential_mean(x))
    assert np.array_equal(xf.crop_mean(xd, tail=D).cpu().numpy(), ref.torch_mean(x, D))
    # the fused route's form: five unmirrored rows, five mirrored rows stored in the order of the crops they mirror
    block1 = torch.empty((B, 5, D), dtype=torch.float32, device=dev)
    for k, p in enumerate(ref.FLIP_OF):
        block1[:, p] = xd[:, 5 + k]
    table = [(0, c) for c in range(5)] + [(1, p) for p in ref.FLIP_OF]
    assert torch.equal(xf.crop_mean(xd[:, :5].contiguous(), block1, table), one)
    assert torch.equal(xf.crop_mean(xd, table=[(0, c) for c in range(5)]), xf.crop_mean(xd[:, :5].contiguous()))


# ------------------------------------------------------------------------------------------------------------ ssg_group_pool_f32

@pytest.mark.parametrize("case", list(ref.POOL_CASES))
def test_group_pool(dev, gold, case):
    x, rows, queries = ref.pool_case(case)
    groups = ref.group_rows(rows, queries)
    t = ref.normalize64(x)
    tmax, tavg = ref.pool64(t, groups)
    rec_y = ref.unpack_steps(gold["pool_%s_y" % case], t)
    rec_max = ref.unpack_steps(gold["pool_%s_max" % case], tmax)
    rec_avg = ref.unpack_steps(gold["pool_%s_avg" % case], tavg)
    hmax, havg, y = xf.multi_query_pool(torch.from_numpy(x).to(dev), rows, queries, return_normalized=True)
    hmax2, havg2 = xf.multi_query_pool(x, rows, queries)                           # without the optional output, from host rows
    assert torch.equal(hmax, hmax2) and torch.equal(havg, havg2)
    y, hmax, havg = y.cpu().numpy(), hmax.cpu().numpy(), havg.cpu().numpy()
    one = U * np.abs(t) * (1 + 2.0 ** -20)                                          # one rounding of a float64 quotient
    err = np.abs(y.astype(np.float64) - t)
    assert np.all(err <= one) and np.all(y[ref.POOL_ZERO_ROW] == 0)
    assert np.all(err <= np.abs(rec_y.astype(np.float64) - t) + one)                # at least as close to t as sklearn's float32 rows
    # the pools of the device's own rows, bit for bit
    assert np.array_equal(hmax, np.stack([y[g].max(axis=0) for g in groups]))
    assert np.array_equal(havg, np.stack([np.ascontiguousarray(y[g]).mean(axis=0) for g in groups]))
    assert np.array_equal(hmax[0], hmax[3]) and np.array_equal(havg[0], havg[3])   # the repeated key
    # against the recorded reference (the bounds come from the fixture; see the module docstring)
    e_max, e_avg = np.abs(hmax - tmax), np.abs(havg - tavg)
    b_max = np.abs(rec_max - tmax) + 2 * U * np.abs(tmax)
    b_avg = np.abs(rec_avg - tavg).max(axis=1, keepdims=True) + 2 * U * np.abs(tavg)
    def worst(e, b):
        return float(np.divide(e, b, out=np.zeros_like(e), where=b > 0).max())
    print("group pool %s: worst |dev - t| / bound: max %.3f, avg %.3f; rows %.3f of one rounding" % (case, worst(e_max, b_max), worst(e_avg, b_avg), worst(err, one)))
    assert np.all(e_max <= b_max)
    assert np.all(e_avg <= b_avg)
    assert np.all(hmax >= havg)


def test_group_pool_long_group_and_nan(dev):
    """a group longer than one pass of the kernel (256 rows) keeps its running values in the output rows; a NaN row poisons its
    group's max like np.max and leaves the other groups alone; a missing key is a KeyError"""
    rng = np.random.default_rng(7)
    M, D = 300, 70
    x = rng.standard_normal((M, D)).astype(np.float32)
    names = ["0001_c1_%03d" % i for i in range(M - 2)] + ["0002_c1_a", "0002_c1_b"]
    x[M - 1, 3] = np.nan
    hmax, havg, y = xf.multi_query_pool(torch.from_numpy(x).to(dev), names, ["0002_c1", "0001_c1"], return_normalized=True)
    y, hmax, havg = y.cpu().numpy(), hmax.cpu().numpy(), havg.cpu().numpy()
    assert np.array_equal(hmax[1], y[:M - 2].max(axis=0)) and np.array_equal(havg[1], np.ascontiguousarray(y[:M - 2]).mean(axis=0))
    assert np.all(np.isnan(y[M - 1])) and np.all(np.isnan(hmax[0])) and np.all(np.isnan(havg[0])) and np.all(np.isfinite(hmax[1]))
    with pytest.raises(KeyError):
        xf.multi_query_pool(torch.from_numpy(x).to(dev), names, ["0003_c1"])


# ------------------------------------------------------------------------------------------------------------------ fused route

def _names(n):
    return ["%04d_c%ds1_%06d_00.jpg" % (i + 1, i % 6 + 1, 51 * i) for i in range(n)]


@pytest.mark.parametrize("arch", ["resnet50", "resnet18"])
def test_five_crops_and_stem_flip_are_the_ten_crops(dev, model50, arch):
    """extract_feature_matrix(tta=True) on a FiveCrops block == the ten materialised crops through model(x), then the mean.  The
    stem's flip only mirrors an index, so the two routes agree bit for bit."""
    if arch == "resnet50":
        m = model50
    else:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = ssg_amd.create(arch, num_features=0, seed=2).cuda().eval()
    src = ref.source_images("market")[:2]
    names = _names(2)
    five = xf.FiveCrops(xf.ten_crop_batch(src, ncrops=5))
    ten = xf.ten_crop_batch(src, ncrops=10)
    fused, ids, cams, files = xf.extract_feature_matrix(m, [(five, names)], print_freq=0, tta=True)
    assert files == names and ids == [1, 2] and cams == [1, 2] and tuple(fused.shape) == (2, m.out_planes)
    per_crop = m(ten.view(-1, 3, 256, 128))[0]                                     # the script's extract_cnn_feature(model, imgs.view(-1, c, h, w))
    literal = xf.crop_mean(per_crop.view(2, 10, -1))
    assert np.array_equal(literal.cpu().numpy(), ref.torch_mean(per_crop.view(2, 10, -1).cpu().numpy(), 0))
    print("%s: five crops + stem flip vs ten crops: max |diff| %.3g" % (arch, float((fused - literal).abs().max())))
    assert torch.equal(fused, literal)
    lit2 = xf.extract_feature_matrix(m, [(ten, names)], print_freq=0, tta=True)[0]   # the switch: ten-crop batches take the literal route
    assert torch.equal(lit2, literal)
    feats, _, _, _ = xf.extract_features(m, [(five, names)], print_freq=0, tta=True)
    assert len(feats) == 2 and feats[0].dtype == np.float32 and np.array_equal(np.stack(feats), fused.cpu().numpy())
    with pytest.raises(ValueError, match="plain image batches"):
        xf.extract_feature_matrix(m, [(ten[:, 0], names)], print_freq=0, tta=True)
    with pytest.raises(ValueError, match="crop blocks"):
        xf.extract_feature_matrix(m, [(ten, names)], print_freq=0, tta=False)


def test_num_split_with_tta_is_refused(dev):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = ssg_amd.create("resnet50", num_classes=0, num_split=2, seed=1)
    with pytest.raises(ValueError, match=r"outputs\.view\(bs, ncrops, -1\)"):
        xf.extract_feature_matrix(m, [], tta=True)


def test_inception_takes_the_literal_ten_crops(dev):
    """144 x 56 with the crop geometry scaled by the same 9/8: resize (162, 63), an odd horizontal margin"""
    m = ssg_amd.create("inception", seed=1).cuda().eval()
    rng = np.random.default_rng(31)
    src = rng.integers(0, 255, (2, 150, 60, 3), dtype=np.uint8)
    ten = xf.ten_crop_batch(src, (162, 63), (144, 56))
    assert np.array_equal(ten.cpu().numpy(), ref.ten_crop_reference(np.stack([ref.pil_resize(im, (162, 63)) for im in src]), (144, 56)))
    got = xf.extract_feature_matrix(m, [(ten, _names(2))], print_freq=0, tta=True)[0]
    per_crop = m(ten.view(-1, 3, 144, 56)).view(2, 10, -1).cpu().numpy()
    assert np.array_equal(got.cpu().numpy(), ref.torch_mean(per_crop, ref.mean_tail(per_crop.shape[2])))


# ------------------------------------------------------------------------------------------------------------------- end to end

FOLDERS = {
    "bounding_box_train": ["0005_c1s1_000001_00.jpg", "0006_c2s1_000001_00.jpg"],
    "query": ["0001_c1s1_000151_00.jpg", "0002_c2s1_000301_00.jpg"],
    "gt_bbox": ["0001_c1s1_000151_00.jpg", "0001_c1s1_000176_00.jpg", "0001_c1s2_000200_00.jpg", "0002_c2s1_000301_00.jpg"],
    "bounding_box_test": ["-1_c3s1_000401_03.jpg", "0001_c2s1_000201_00.jpg", "0002_c1s1_000401_00.jpg"],
}


@pytest.fixture(scope="module")
def market_dirs(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("market")
    import zlib
    for folder, files in FOLDERS.items():
        os.makedirs(str(root / folder))
        for f in files:                                  # a file's pixels follow from its name: the query files are also in gt_bbox
            blocks = np.random.default_rng(zlib.crc32(f.encode())).integers(0, 255, (16, 8, 3), dtype=np.uint8)
            Image.fromarray(np.repeat(np.repeat(blocks, 8, axis=0), 8, axis=1)).save(str(root / folder / f), quality=90)      # baseline JPEG, 128 x 64
    return {k: str(root / k) for k in FOLDERS}


def _evaluate(model, d, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = xf.evaluate(model, d["bounding_box_train"], d["query"], d["gt_bbox"], d["bounding_box_test"], batch_size=3, **kw)
    return res, buf.getvalue()


def _check_result(res, D=2048):
    for var, folder in (("train", "bounding_box_train"), ("query", "query"), ("test", "bounding_box_test")):
        files = sorted(FOLDERS[folder])
        assert res[var + "ID"].tolist() == [xf.parse_market_name(f)[0] for f in files]
        assert res[var + "CAM"].tolist() == [xf.parse_market_name(f)[1] for f in files]
        assert res["Hist_" + var].shape == (len(files), D) and res["Hist_" + var].dtype == np.float32
    assert res["testID"][0] == -1 and res["testCAM"][0] == 3
    assert res["Hist_max"].shape == res["Hist_avg"].shape == (2, D)
    assert sorted(res) == sorted(v for _, v in xf.MAT_FILES) and len(res) == 11
    assert np.all(np.isfinite(res["Hist_max"])) and np.all(res["Hist_max"] >= res["Hist_avg"])


def test_evaluate_end_to_end_with_tta(dev, model50, market_dirs):
    res, out = _evaluate(model50, market_dirs, tta=True)
    _check_result(res)
    assert out.count("Mean AP") == 3 and "Extract Features: [1/1]" in out
    # query 1's key has one gt_bbox row: its pooled descriptors are that row, normalised; the file is also the query itself
    row = res["Hist_query"][1].astype(np.float64)
    want = row / np.sqrt((row * row).sum())
    assert np.abs(res["Hist_max"][1] - want).max() <= U * np.abs(want).max() * 1.01 and np.array_equal(res["Hist_max"][1], res["Hist_avg"][1])
    # the loader's five-crop block is the transform of the decoded files
    from PIL import Image
    files = sorted(FOLDERS["query"])
    pix = np.stack([np.asarray(Image.open(os.path.join(market_dirs["query"], f)).convert("RGB")) for f in files])
    (block, names), = list(xf.TestBatchLoader(market_dirs["query"], tta=True))
    assert names == files and isinstance(block, xf.FiveCrops) and torch.equal(block.crops, xf.ten_crop_batch(pix, ncrops=5))
    (plain, _), = list(xf.TestBatchLoader(market_dirs["query"], decode="pillow"))
    assert torch.equal(plain, ssg_amd.preprocess_batch(pix, 256, 128))


def test_evaluate_writes_the_mat_files(dev, model50, market_dirs, tmp_path):
    sio = pytest.importorskip("scipy.io")
    out_dir = str(tmp_path / "matdata")
    res, out = _evaluate(model50, market_dirs, out_dir=out_dir, print_scores=False)
    _check_result(res)
    assert "Mean AP" not in out
    assert sorted(os.listdir(out_dir)) == sorted(stem + ".mat" for stem, _ in xf.MAT_FILES)
    for stem, var in xf.MAT_FILES:
        back = sio.loadmat(os.path.join(out_dir, stem + ".mat"))[var]
        assert np.array_equal(back.reshape(res[var].shape), res[var]) and back.dtype == res[var].dtype, stem


# -------------------------------------------------------------------------------------------------------------- classifier head

def test_classifier_head(dev, model50):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m0 = ssg_amd.create("resnet50", dropout=0.0, num_features=2048, num_classes=0, seed=1).cuda().eval()
    x = torch.randn(3, 3, 256, 128, generator=torch.Generator().manual_seed(9))
    x1, x2 = model50(x)
    y1, feat = m0(x)
    assert torch.equal(x1, y1) and tuple(x2.shape) == (3, 632)
    sd = model50.state_dict()
    W, b = sd["classifier_x2.weight"].double(), sd["classifier_x2.bias"].double()
    f64 = feat.cpu().double()
    want = f64 @ W.T + b
    A = f64.abs() @ W.abs().T + b.abs()
    lim = bound(2048 + 1, A)                                                        # tests/head_ref.py: a 2048-term float32 sum plus the bias
    err = (x2.cpu().double() - want).abs()
    print("classifier_x2: worst |err| / bound %.4f (max |err| %.3g)" % (float((err / lim).max()), float(err.max())))
    assert bool((err <= lim).all())
