"""GPU suite of the verification metrics (csrc/verify.hip, ssg_amd/verification.py) against the numpy restatement tests/verify_ref.py.

Counts, minima, maxima, order statistics, threshold counts, num / cnt / GAR and the error rates must equal the restatement bit for
bit.  The averages and deviations come from float64 sums taken in another order than numpy's, so they are held to
    |device - exact| <= |ref32 - exact| + 2^-52 |exact|
(`exact` / `ref32`: the restatement with float64 / with the reference's float32 running sums): the device may not be worse than the
reference's own arithmetic.  Every case prints one `verify-error` line per quantity (pytest -s); profiles/verify_errors.txt is such a log."""
import contextlib
import ctypes
import io
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verify_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@lru_cache(maxsize=None)
def _case(name):
    c = verify_ref.make_case(name)
    d = c["dist"][:, :c["n"]]
    return c, verify_ref.find_metric_threshold(c["ql"], c["rl"], d, mode="exact"), verify_ref.find_metric_threshold(c["ql"], c["rl"], d, mode="ref32")


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


class Abi(object):
    """the three passes through the C ABI on a device block D[m, n] at pitch ld (D: any float32 CUDA tensor view with stride(1) == 1)"""

    def __init__(self, D, ql, rl):
        from ssg_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.D, self.m, self.n, self.ld = D, D.shape[0], D.shape[1], D.stride(0)
        dev = D.device
        self.ql = torch.as_tensor(np.asarray(ql, dtype=np.int32)).to(dev); self.rl = torch.as_tensor(np.asarray(rl, dtype=np.int32)).to(dev)
        self.wb = int(self.L.ssg_verify_workspace_bytes(self.m, self.n))
        self.ws = torch.empty(self.wb // 8 + 1, dtype=torch.int64, device=dev)
        self.head = (D.data_ptr(), self.m, self.n, self.ld, self.ql.data_ptr(), self.rl.data_ptr())

    def stats(self):
        dev = self.D.device
        c = torch.zeros(2, dtype=torch.int64, device=dev); s = torch.zeros(4, dtype=torch.float64, device=dev)
        mm = torch.zeros(4, dtype=torch.float32, device=dev); st = torch.full((2,), -1, dtype=torch.int32, device=dev)
        self.lib.check(self.L.ssg_verify_stats_f32(*self.head, self.ws.data_ptr(), self.wb, c.data_ptr(), s.data_ptr(), mm.data_ptr(), st.data_ptr(),
                                                   self.lib.stream()), "ssg_verify_stats_f32")
        return c.cpu().numpy(), s.cpu().numpy(), mm.cpu().numpy(), st.cpu().numpy()

    def select(self, ranks):
        dev = self.D.device
        host = (ctypes.c_int64 * len(ranks))(*[int(r) for r in ranks])
        v = torch.zeros(len(ranks), dtype=torch.float32, device=dev); st = torch.full((1,), -1, dtype=torch.int32, device=dev)
        self.lib.check(self.L.ssg_verify_select_f32(*self.head, host, len(ranks), self.ws.data_ptr(), self.wb, v.data_ptr(), st.data_ptr(),
                                                    self.lib.stream()), "ssg_verify_select_f32")
        return v.cpu().numpy(), int(st.item())

    def count(self, thr, is_sq=1):
        dev = self.D.device
        host = (ctypes.c_double * len(thr))(*[float(t) for t in thr])
        c = torch.full((3, len(thr)), -1, dtype=torch.int64, device=dev); tot = torch.full((2,), -1, dtype=torch.int64, device=dev)
        self.lib.check(self.L.ssg_verify_count_f32(*self.head, is_sq, host, len(thr), self.ws.data_ptr(), self.wb, c.data_ptr(), tot.data_ptr(),
                                                   self.lib.stream()), "ssg_verify_count_f32")
        return c.cpu().numpy(), tot.cpu().numpy()


# ------------------------------------------------------------------ s = sqrtf(max(d, 0)) equals numpy's, bit for bit
def test_sqrt_equals_numpy_bit_for_bit(dev):
    from ssg_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(5)
    fin = np.finfo(np.float32)
    special = np.array([0.0, -0.0, -1.0, -fin.tiny, fin.smallest_subnormal, 2 * fin.smallest_subnormal, 3 * fin.smallest_subnormal, fin.tiny / 2,
                        fin.tiny * (1 - 2.0 ** -23), fin.tiny, fin.max, fin.max * (1 - 2.0 ** -24), 1.0, 2.0, 3.0, 4.0, 0.25, 1 - 2.0 ** -24, 1 + 2.0 ** -23,
                        np.inf], dtype=np.float32)
    pats = rng.integers(0, 0x7f800000, 40000, dtype=np.uint32).view(np.float32)                    # every exponent, subnormals included
    sub = rng.integers(1, 0x00800000, 4000, dtype=np.uint32).view(np.float32)                      # subnormals only
    sq = (rng.integers(1, 4096, 4000).astype(np.float32) ** 2)                                     # perfect squares and their neighbours
    near = np.concatenate([sq, np.nextafter(sq, np.float32(0)), np.nextafter(sq, np.float32(np.inf))])
    table = np.concatenate([special, pats, sub, near, -pats[:100]]).astype(np.float32)
    want = verify_ref.clamp_sqrt(table)
    d = torch.from_numpy(table).to(dev); s = torch.empty_like(d)
    _lib.check(L.ssg_selftest_verify_sqrt(d.data_ptr(), table.size, s.data_ptr(), _lib.stream()), "ssg_selftest_verify_sqrt")
    got = s.cpu().numpy()
    bad = np.nonzero(_u32(got) != _u32(want))[0]
    assert bad.size == 0, [(table[i], got[i], want[i]) for i in bad[:5]]


# ------------------------------------------------------------------ the cases, through the public function with dist=
def _err_line(case, what, dev_v, exact_v, r32_v):
    e_dev, e_ref = abs(float(dev_v) - float(exact_v)), abs(float(np.float64(r32_v)) - float(exact_v))
    print("verify-error case %s %-9s device %.17g exact %.17g ref32 %.9g |dev-exact| %.3g |ref32-exact| %.3g" % (case, what, dev_v, exact_v, r32_v, e_dev, e_ref))
    return e_dev, e_ref


@pytest.mark.parametrize("name", verify_ref.CASES)
def test_cases_equal_restatement(dev, name):
    from ssg_amd.verification import find_metric_threshold
    c, exact, r32 = _case(name)
    n = c["n"]
    if name == "a":
        dist = c["dist"][:, :n]                                   # numpy view at pitch ld
    elif name == "c":
        dist = torch.from_numpy(c["dist"])[:, :n]                 # CPU tensor
    else:
        dist = torch.from_numpy(c["dist"]).to(dev)[:, :n]         # CUDA tensor at pitch ld > n: used in place
    before = c["dist"].copy()
    buf = io.StringIO(); log = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = find_metric_threshold(c["x"], c["ql"], c["y"], c["rl"], dist=dist, fid=log)
    got_after = dist.cpu().numpy() if isinstance(dist, torch.Tensor) else dist
    assert np.array_equal(_u32(got_after), _u32(before[:, :n])), "dist was modified"
    assert (res.intra_num, res.inter_num) == (exact["intra_num"], exact["inter_num"])
    for k in ("intra_min", "intra_max", "inter_min", "inter_max"):
        assert _u32(getattr(res, k)) == _u32(exact[k]), k
    assert res.num == exact["num"] and res.cnt == exact["cnt"]
    assert np.array_equal(_u32(res.thr), _u32(exact["thr"]))
    assert _u64(res.GAR).tolist() == _u64(exact["GAR"]).tolist()
    assert res.too_bad == exact["too_bad"]
    for k in ("intra_avg", "inter_avg", "intra_std", "inter_std"):
        e_dev, e_ref = _err_line(name, k, getattr(res, k), exact[k], r32[k])
        assert e_dev <= e_ref + 2.0 ** -52 * abs(float(exact[k])), k
    if not exact["too_bad"]:
        # the thresholds are np.linspace of the device's own float64 averages: the counts at THOSE thresholds, and the rates, exactly
        assert np.array_equal(_u64(res.thresholds), _u64(np.linspace(res.intra_avg, res.inter_avg, 10)))
        s = verify_ref.clamp_sqrt(c["dist"][:, :n]); intra, _ = verify_ref.masks(c["ql"], c["rl"])
        ge, lt, _ = verify_ref.threshold_counts(s, intra, res.thresholds)
        assert np.array_equal(_u64(res.pos_err_rate), _u64(ge.astype('float') / exact["intra_num"]))
        assert np.array_equal(_u64(res.neg_err_rate), _u64(lt.astype('float') / exact["inter_num"]))
        # and they are the exact mode's (an element would have to lie between two thresholds one rounding apart for a difference)
        assert np.array_equal(_u64(res.pos_err_rate), _u64(exact["pos_err_rate"])) and np.array_equal(_u64(res.neg_err_rate), _u64(exact["neg_err_rate"]))
    else:
        assert res.thresholds is None and res.pos_err_rate is None
    # the printed lines are the restatement's (= the reference's, tests/test_verify_host.py), and fid received them
    assert buf.getvalue().split("\n")[:-1] == exact["lines"]
    assert res.lines == exact["lines"]
    assert [ln for ln in log.getvalue().split("\n") if ln] == [ln for ln in exact["lines"] if ln]


def test_second_call_gives_identical_bits(dev):
    c, _, _ = _case("d")
    D = torch.from_numpy(c["dist"]).to(dev)[:, :c["n"]]
    a = Abi(D, c["ql"], c["rl"])
    ranks = [int(v) for v in np.linspace(0, 64 * (4099 - 63) - 1, 64)]
    thr = np.linspace(0.5, 9.0, 64)
    first = (a.stats(), a.select(ranks), a.count(thr))
    second = (a.stats(), a.select(ranks), a.count(thr))
    for x, y in zip(first[0] + (first[1][0],) + first[2], second[0] + (second[1][0],) + second[2]):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------ the three passes one by one through the C ABI
@pytest.mark.parametrize("n,ld,off,nan", [(n, ld, off, False) for n in (1, 3, 63, 64, 65, 1029) for ld, off in ((n + 8 - n % 4, 0), (n + 8 - n % 4, 3), (n + 5 - n % 4, 0))]
                         + [(65, 72, 1, True), (1029, 1032, 2, False)])
def test_passes_through_the_abi(dev, n, ld, off, nan):
    """ld > n always; ld % 4 == 0 with an aligned (off = 0) or a misaligned base (the 16-byte loads start inside the row), and
    ld % 4 == 1 (element loads); m = 35: three row groups, the last one short; 64 ranks and 64 thresholds at once"""
    m = 35
    rng = np.random.default_rng(n * 131 + ld * 7 + off)
    vals = (rng.standard_normal((m, n)) * 2 + 1.5).astype(np.float32)
    vals[rng.random((m, n)) < 0.1] = 0.0
    vals[rng.random((m, n)) < 0.2] = np.float32(2.25)              # ties
    if nan:
        vals[17, n // 2] = np.nan
    rl = rng.integers(-1, 3, n); ql = rng.integers(0, 3, m)
    ql[0] = rl[0]; ql[1] = rl[0] + 1                               # at least one intra and one inter element
    buf = torch.full((m * ld + 8,), 7e30, dtype=torch.float32, device=dev)
    D = buf[off: off + m * ld].view(m, ld)[:, :n]
    D.copy_(torch.from_numpy(vals))
    assert D.data_ptr() % 16 == 4 * off and D.stride(0) == ld
    kept = buf.clone()
    a = Abi(D, ql, rl)
    s = verify_ref.clamp_sqrt(vals); intra, inter = verify_ref.masks(ql, rl)
    counts, sums, mm, st = a.stats()
    assert counts.tolist() == [int(intra.sum()), int(inter.sum())]
    assert st[0] == int(bool((intra.sum(1) == 0).any() or (inter.sum(1) == 0).any())) and st[1] == int(nan)
    if not nan:
        for got, want in zip(sums, (s[intra].astype(np.float64).sum(), (s[intra].astype(np.float64) ** 2).sum(),
                                    s[inter].astype(np.float64).sum(), (s[inter].astype(np.float64) ** 2).sum())):
            assert abs(got - want) <= 2.0 ** -45 * abs(want)          # float64 sums of <= 36 015 terms in another order
        assert np.array_equal(_u32(mm), _u32([s[intra].min(), s[intra].max(), s[inter].min(), s[inter].max()]))
        srt = np.sort(s[inter])
        ranks = sorted(int(r) for r in rng.integers(0, srt.size, 62)) + [0, srt.size - 1]
        rng.shuffle(ranks)                                            # any order
        got, bad = a.select(ranks)
        assert bad == 0 and np.array_equal(_u32(got), _u32(srt[ranks]))
        got, bad = a.select([0, srt.size])                            # a rank outside: flagged through the status word
        assert bad == 1 and np.isnan(got).all()
    thr = list(rng.choice(np.unique(s[~np.isnan(s)]).astype(np.float64), 20)) + list(rng.uniform(-0.5, 6.0, 40)) + [0.0, -np.inf, np.inf, 2.25]
    rng.shuffle(thr)
    for is_sq, v in ((1, s), (0, vals)):
        c3, tot = a.count(thr, is_sq)
        ge, lt, below = verify_ref.threshold_counts(v, intra, [np.float64(t) for t in thr])
        assert np.array_equal(c3[0], ge) and np.array_equal(c3[1], lt) and np.array_equal(c3[2], below)
        assert tot.tolist() == [int(intra.sum()), int(inter.sum())]
    assert torch.equal(buf.view(torch.int32), kept.view(torch.int32))                                       # nothing was written into the block


def test_block_beyond_4gib(dev):
    """m * ld * 4 > 2^32 bytes.  The block is table[(i * 7 + j * 13 + (i * j >> 5)) % T] built on the device; expected counts, order
    statistics and threshold counts from torch on the device (per-class histograms of the table index, float64 sums)."""
    m, n, ld, T = 8200, 131073, 131076, 1021
    assert m * ld * 4 > 2 ** 32
    rng = np.random.default_rng(3)
    table = np.sort((rng.random(T) * 9.0).astype(np.float32)); table[:3] = [-1.0, 0.0, 0.0]
    tab = torch.from_numpy(table).to(dev)
    ql = (np.arange(m) * 5 % 97).astype(np.int32); rl = (np.arange(n) * 11 % 97).astype(np.int32)
    qd, rd = torch.from_numpy(ql).to(dev), torch.from_numpy(rl).to(dev)
    D = torch.empty((m, ld), dtype=torch.float32, device=dev)
    D[:, n:] = 5e29
    h = torch.zeros((2, T), dtype=torch.int64, device=dev)
    jj = torch.arange(n, device=dev, dtype=torch.int64)
    for r0 in range(0, m, 1025):
        ii = torch.arange(r0, min(r0 + 1025, m), device=dev, dtype=torch.int64)[:, None]
        idx = (ii * 7 + jj * 13 + ((ii * jj) >> 5)) % T
        D[r0:r0 + idx.shape[0], :n] = tab[idx]
        intra = rd[None, :] == qd[r0:r0 + idx.shape[0], None]
        h[0] += torch.bincount(idx[intra], minlength=T); h[1] += torch.bincount(idx[~intra], minlength=T)
        del idx, intra
    s_tab = torch.sqrt(torch.clamp(tab, min=0)).double()
    a = Abi(D[:, :n], ql, rl)
    counts, sums, mm, st = a.stats()
    assert counts.tolist() == [int(h[0].sum()), int(h[1].sum())] and sum(counts.tolist()) == m * n and st.tolist() == [0, 0]
    want = [float((h[0] * s_tab).sum()), float((h[0] * s_tab * s_tab).sum()), float((h[1] * s_tab).sum()), float((h[1] * s_tab * s_tab).sum())]
    for g, w in zip(sums, want):
        assert abs(g - w) <= 1e-11 * abs(w)
    st32 = s_tab.float().cpu().numpy()
    h_np = h.cpu().numpy()
    assert np.array_equal(_u32(mm), _u32([st32[h_np[0] > 0].min(), st32[h_np[0] > 0].max(), st32[h_np[1] > 0].min(), st32[h_np[1] > 0].max()]))
    cum = np.cumsum(h_np[1])
    ranks = [0, 1, int(cum[2]) - 1, int(cum[2]), int(1e-5 * cum[-1]), int(1e-2 * cum[-1]), int(cum[-1] // 2), int(cum[-1] // 10 * 9),
             int(cum[-1]) - 1]
    got, bad = a.select(ranks)
    assert bad == 0 and np.array_equal(_u32(got), _u32(st32[np.searchsorted(cum, ranks, side="right")]))
    thr = [0.0, 0.5, float(st32[500]), float(np.nextafter(st32[500], np.float32(9))), 2.9, 10.0]
    c3, tot = a.count(thr)
    s64 = st32.astype(np.float64)
    for q, t in enumerate(thr):
        assert c3[0, q] == h_np[0][s64 >= t].sum() and c3[1, q] == h_np[1][s64 < t].sum() and c3[2, q] == h_np[0][s64 < t].sum()
    assert tot.tolist() == counts.tolist()


# ------------------------------------------------------------------ the Python surface
def _fields(res):
    out = []
    for k, v in sorted(res.__dict__.items()):
        out.append((k, None if v is None else np.asarray(v).tobytes() if k != "lines" else "\n".join(v)))
    return out


def test_from_features_equals_dist_path(dev):
    from ssg_amd.evaluators import _sqdist
    from ssg_amd.verification import find_metric_threshold
    c, _, _ = _case("a")
    x, y = torch.from_numpy(c["x"]), torch.from_numpy(c["y"])
    with contextlib.redirect_stdout(io.StringIO()):
        a = find_metric_threshold(c["x"], c["ql"], c["y"], c["rl"])
        block = _sqdist(x, y)
        b = find_metric_threshold(None, c["ql"], None, c["rl"], dist=block)
        b2 = find_metric_threshold(x, list(c["ql"]), y, torch.from_numpy(c["rl"]), dist=block, far=(1e-2, 1e-3, 1e-4, 1e-5))
    assert _fields(a) == _fields(b) == _fields(b2)
    assert a.intra_num == 1073 and a.inter_num == 6438


def test_cal_classification_error_compares_dist_as_given(dev):
    from ssg_amd.verification import CalClassificationError_MPI
    c, _, _ = _case("c")
    n = c["n"]
    d = c["dist"][:, :n]
    thr = list(np.linspace(-30.0, 60.0, 67)) + [0.0, 0.0, float(d.max()), float(d.min())]          # 71 thresholds: two calls inside, unsorted, repeated
    buf = io.StringIO(); log = io.StringIO()
    with contextlib.redirect_stdout(buf):
        pos, neg = CalClassificationError_MPI(c["x"], c["ql"], c["y"], c["rl"], thr, dist=torch.from_numpy(c["dist"]).to(dev)[:, :n], fid=log)
    wp, wn, pos_num, neg_num, wlog = verify_ref.cal_classification_error(c["ql"], c["rl"], thr, d)
    assert np.array_equal(_u64(pos), _u64(wp)) and np.array_equal(_u64(neg), _u64(wn))
    assert buf.getvalue() == wlog + "\n" and log.getvalue() == wlog + "\n"


def test_status_words_raise_value_error(dev):
    from ssg_amd.verification import find_metric_threshold
    d = np.ones((3, 6), dtype=np.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match="no intra"):
            find_metric_threshold(None, [0, 1, 5], None, [0, 1, 0, 1, 2, 2], dist=d)               # query 2 has no match in the gallery
        with pytest.raises(ValueError, match="no intra"):
            find_metric_threshold(None, [0, 0, 0], None, [0] * 6, dist=d)                          # nobody has an inter element
        d[1, 4] = np.nan
        with pytest.raises(ValueError, match="NaN"):
            find_metric_threshold(None, [0, 1, 2], None, [0, 1, 0, 1, 2, 2], dist=d)


def test_evaluator_evaluate_same_cams(dev, golden):
    """reid/evaluators.py:194-207 on a tiny resident set: the verification lines, then mAP / CMC without the camera filter"""
    import ssg_amd
    g = golden("embed_ref.npz")
    imgs = torch.randn(4, 3, 256, 128, generator=torch.Generator().manual_seed(int(g["image_seed"])))
    imgs = torch.cat([imgs, imgs.flip(0) * 0.9], 0)
    names = ["i%d" % i for i in range(8)]; pids = [0, 1, 2, 3, 3, 2, 1, 0]
    model = ssg_amd.create("resnet50", num_classes=0, num_split=1, cluster=False, seed=int(g["weight_seed"])).cuda()
    loader = ssg_amd.TensorBatchLoader(imgs, batch_size=8, fnames=names, pids=pids)
    query = [(names[i], pids[i], 0) for i in range(4)]; gallery = [(names[i], pids[i], 0) for i in range(8)]     # ONE camera: evaluate() would drop every match
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        top1 = ssg_amd.Evaluator(model, print_freq=1).evaluate_same_cams(loader, query, gallery)
    lines = [ln for ln in buf.getvalue().split("\n") if ln and not ln.startswith("Extract Features")]
    with contextlib.redirect_stdout(io.StringIO()):
        feats, _ = ssg_amd.extract_features(model, loader)
        block = ssg_amd.pairwise_distance_device(feats, query, gallery)
    want_buf = io.StringIO()
    with contextlib.redirect_stdout(want_buf):
        ssg_amd.find_metric_threshold(None, pids[:4], None, pids, dist=block)
        want_top1 = ssg_amd.evaluate_all(block, query_ids=pids[:4], gallery_ids=pids, query_cams=[0] * 4, gallery_cams=[1] * 8)
        same = ssg_amd.evaluate_same_cams_all(block, query_ids=pids[:4], gallery_ids=pids)
    assert top1 == want_top1 == same
    want = [ln for ln in want_buf.getvalue().split("\n") if ln]
    assert lines == want[:len(lines)]
    assert lines[0].startswith("Intra Distance: 8, ") and lines[1].startswith("Inter Distance: 24, ")
    assert lines[2] in ("pos pair num 8, neg pair num 24", "The Metric Feature Is Too Bad!") and [ln[:4] for ln in lines[3:7]] == ["thr:"] * 4
    assert lines[7].startswith("Mean AP:") and lines[8].startswith("CMC Scores") and [ln[:4] for ln in lines[9:]] == ["top-"] * 3
