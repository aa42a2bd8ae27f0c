"""CPU half of the silhouette tests: the sequential restatement of tests/silhouette_ref.py against what sklearn 1.7.2 gave
(tests/golden/silhouette_cases.npz; live sklearn where it imports), the product's host stage (ssg_amd/silhouette.py: the encoding, the
member lists, sklearn's finishing lines) fed the restatement's sums, the pure selection function of the eps sweep with a fake scorer,
the argument errors that need no device, and the refusals of the entry points, which are made before any device call."""
import ctypes

import numpy as np
import pytest

import silhouette_ref as ref

NAMES = [c["name"] for c in ref.CASES]


@pytest.fixture(scope="module")
def gold():
    return ref.load_golden()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_golden(gold, name):
    """one running float64 sum per cluster per row in column order, the division, the min and sklearn's four lines give sklearn's
    per-sample result bit for bit (uint64 views), the sub-problem without the noise and the sampled score with its permuted column
    order included; the labels rebuilt from the seed are the stored ones"""
    case = ref.BY_NAME[name]
    lab = ref.labels(case)
    assert lab.dtype == np.int64 and np.array_equal(lab, gold[name + "/labels"])
    if case["kind"] == "neg":
        assert str(gold[name + "/error"]).startswith("Negative values in data passed to `pairwise_distances`.")
        assert (ref.expected_input(case) < 0).any() and np.isfinite(ref.expected(case)).all()
        return
    got = ref.expected(case)
    assert _same_bits(got, gold[name + "/sil"])
    kept = got[~np.isnan(got)]
    assert (len(kept) < len(got)) == ref.ignore_noise(case) and float(np.mean(kept)) == float(gold[name + "/score"])
    if case.get("sample"):
        rs = np.random.RandomState(ref.SAMPLE_SEED)
        assert ref.sampled_score(ref.expected_input(case), lab, case["N"] // 2, rs) == float(gold[name + "/sampled_score"])
        assert rs.random_sample() == float(gold[name + "/next_draw"])


def test_the_cases_cover_what_they_are_for(gold):
    assert {c["N"] for c in ref.CASES} >= {3, 7, 65, 513, 1030}
    assert {c["kind"] for c in ref.CASES} == {"f64", "f32", "f16", "neg", "rerank"}
    assert {c["labeling"] for c in ref.CASES} >= {"halves", "big_single", "pairs", "many", "gapped", "noise"}
    many = ref.labels(ref.BY_NAME["n1030_many"])
    assert len(np.unique(many)) > 256 + 128, "more clusters than a workgroup has threads: the per-thread cluster loop wraps"
    big = ref.labels(ref.BY_NAME["n513_big_single"])
    single = int(np.nonzero(big == 1)[0][0])
    assert np.count_nonzero(big == 1) == 1 and gold["n513_big_single/sil"][single] == 0.0       # nan_to_num: a singleton scores 0
    gapped = ref.labels(ref.BY_NAME["n65_gapped_f32"])
    assert gapped.min() < -1 and (gapped == -1).any() and gapped.max() == 1000
    pairs = np.bincount(ref.labels(ref.BY_NAME["n65_pairs"]))
    assert sorted(pairs.tolist()) == [2] * 31 + [3]
    noise = ref.labels(ref.BY_NAME["n513_noise"])
    assert np.count_nonzero(noise == -1) == 513 // 3 and np.isnan(gold["n513_noise/sil"]).sum() == 513 // 3
    assert ref.matrix(ref.BY_NAME["n65_gapped_f16"]).dtype == np.float16 and ref.matrix(ref.BY_NAME["n513_gapped_f32"]).dtype == np.float32
    D = ref.matrix(ref.BY_NAME["rerank_n256_few"])
    assert (np.abs(np.diag(D)) > 100 * np.finfo(np.float64).eps).any(), "the re-rank matrix has the non-zero diagonal sklearn refuses"


@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_sklearn_where_it_imports(gold, name):
    try:
        from sklearn.metrics import silhouette_samples, silhouette_score
    except ImportError:
        return
    case = ref.BY_NAME[name]
    X, lab = ref.expected_input(case), ref.labels(case)
    if case["kind"] == "neg":
        with pytest.raises(ValueError) as e:
            silhouette_samples(X, lab, metric="precomputed")
        assert str(e.value) == str(gold[name + "/error"])
        return
    if ref.ignore_noise(case):
        keep = lab != -1
        want = np.full(len(lab), np.nan)
        want[keep] = silhouette_samples(X[keep][:, keep], lab[keep], metric="precomputed")
    else:
        want = silhouette_samples(X, lab, metric="precomputed")
    assert _same_bits(ref.expected(case), want)
    if case.get("sample"):
        rs = np.random.RandomState(ref.SAMPLE_SEED)
        assert silhouette_score(X, lab, metric="precomputed", sample_size=case["N"] // 2, random_state=ref.SAMPLE_SEED) == ref.sampled_score(X, lab, case["N"] // 2, rs)


@pytest.mark.parametrize("name", [n for n in NAMES if ref.BY_NAME[n]["N"] <= 513 and ref.BY_NAME[n]["kind"] != "neg"])
def test_host_stage_on_the_restatement_s_sums(gold, name):
    """ssg_amd.silhouette's host stage -- the encoding, the member lists, sklearn's finishing lines -- fed the restatement's two arrays
    gives the golden result; the member lists are the positions of every cluster in ascending order"""
    from ssg_amd import silhouette as sil
    case = ref.BY_NAME[name]
    X, lab = ref.expected_input(case), ref.labels(case)
    enc, C = sil._encode(lab, ref.ignore_noise(case))
    assert enc.dtype == np.int32 and sil._labels_valid(enc, C)
    keep = enc >= 0
    assert np.array_equal(keep, lab != -1) if ref.ignore_noise(case) else keep.all()
    assert np.array_equal(np.unique(lab[keep])[enc[keep]], lab[keep])
    members, start = sil._member_list(enc, C)
    assert members.dtype == start.dtype == np.int32 and start[0] == 0 and start[-1] == keep.sum() and len(start) == C + 1
    for c in range(C):
        assert np.array_equal(members[start[c]:start[c + 1]], np.nonzero(enc == c)[0])
    intra, inter = np.full(len(lab), np.nan), np.full(len(lab), np.nan)
    intra[keep], inter[keep] = ref.reduce_rows(X[keep][:, keep], enc[keep], C)
    assert _same_bits(sil._finish(intra, inter, enc), gold[name + "/sil"])


# ------------------------------------------------------------------ the sweep's selection
def _cut(n, clusters, noise=0):
    """n samples: `noise` of them -1, the rest dealt over `clusters` labels"""
    lab = np.full(n, -1)
    lab[noise:] = np.arange(n - noise) % clusters
    return lab


def test_select_cut_first_maximum_invalid_cuts_fallback_and_noise_as_zero():
    from ssg_amd.silhouette import cut_is_valid, select_cut
    n = 12
    calls = []

    def scorer(values):
        def run(cuts):
            calls.append(len(cuts))
            out = []
            for lab, v in zip(cuts, values):
                s = np.where(np.asarray(lab) == -1, np.nan, v)
                out.append(s)
            return out
        return run

    # validity: between 2 and m - 1 labels among the m clustered samples
    assert cut_is_valid(_cut(n, 3)) and cut_is_valid(_cut(n, 2, noise=9))
    assert not cut_is_valid(_cut(n, 1)) and not cut_is_valid(np.full(n, -1)) and not cut_is_valid(np.arange(n)) and not cut_is_valid(_cut(n, 2, noise=10))
    factors = (0.6, 0.8, 1.0, 1.25, 1.5)
    # the first maximum in list order wins
    cuts = [_cut(n, 3)] * 5
    best, scores = select_cut(factors, cuts, scorer([0.1, 0.5, 0.2, 0.5, 0.3]))
    assert best == 1 and scores == pytest.approx([0.1, 0.5, 0.2, 0.5, 0.3]) and calls == [5]
    # invalid cuts are skipped and never reach the scorer; the scorer is called once, with the valid cuts in order
    del calls[:]
    cuts = [np.full(n, -1), _cut(n, 3), _cut(n, 1), _cut(n, 4), np.arange(n)]
    best, scores = select_cut(factors, cuts, scorer([0.2, 0.4]))
    assert best == 3 and scores[0] is None and scores[2] is None and scores[4] is None and scores[1] == pytest.approx(0.2) and scores[3] == pytest.approx(0.4)
    assert calls == [2]
    # no valid cut: the factor 1.0 wins and the scorer is not called; without a factor 1.0 the nearest one, the first of two equally near
    del calls[:]
    best, scores = select_cut(factors, [np.full(n, -1)] * 5, scorer([]))
    assert best == 2 and scores == [None] * 5 and calls == []
    assert select_cut((0.5, 0.9, 1.1), [np.arange(n)] * 3, scorer([]))[0] == 1
    # noise counts as zero: a cut that keeps three samples at 0.9 loses to one that keeps them all at 0.3
    cuts = [_cut(n, 2, noise=9), _cut(n, 3)]
    best, scores = select_cut((1.0, 1.5), cuts, scorer([0.9, 0.3]))
    assert scores == pytest.approx([0.9 * 3 / n, 0.3]) and best == 1
    # negative scores are compared like any others
    assert select_cut((0.8, 1.0), [_cut(n, 3)] * 2, scorer([-0.5, -0.2]))[0] == 1
    with pytest.raises(ValueError):
        select_cut((1.0,), cuts, scorer([0.1]))


# ------------------------------------------------------------------ errors that need no device
def test_argument_errors_without_a_device():
    import torch
    import ssg_amd
    from ssg_amd import cluster, silhouette
    from ssg_amd import silhouette_many, silhouette_samples, silhouette_score
    assert cluster.silhouette_samples is silhouette.silhouette_samples is silhouette_samples and cluster.silhouette_many is silhouette_many
    assert cluster.silhouette_score is silhouette_score and ssg_amd.generate_selflabel_sweep is ssg_amd.selftraining.generate_selflabel_sweep
    X, lab = np.zeros((4, 4)), np.array([0, 0, 1, 1])
    for fn in (silhouette_samples, silhouette_score):
        with pytest.raises(ValueError, match="implements metric='precomputed' only"):
            fn(X, lab, metric="euclidean")
        with pytest.raises(ValueError, match="diagonal must be 'check'"):
            fn(X, lab, diagonal="fill")
        with pytest.raises(ValueError, match="state must be 0"):
            fn(X, lab, state=3)
    with pytest.raises(ValueError, match="diagonal must be 'check'"):
        silhouette_many(X, [lab], diagonal=None)
    with pytest.raises(ValueError, match="at least one labeling"):
        silhouette_many(X, [])
    for bad in (0, -1, 2.0):
        with pytest.raises(ValueError) as e:
            silhouette_score(X, lab, sample_size=bad)
        assert str(e.value) == "The 'sample_size' parameter of silhouette_score must be an int in the range [1, inf) or None. Got %r instead." % (bad,)
    with pytest.raises(ValueError, match="cannot be used to seed"):
        silhouette_score(X, lab, sample_size=2, random_state="x")

    class Sparse:
        shape = (4, 4)

        def tocsr(self):
            return self
    with pytest.raises(TypeError, match="sparse input is not supported"):
        silhouette_samples(Sparse(), lab)
    with pytest.raises(TypeError, match="unsupported distance matrix type"):
        silhouette_samples([[0.0, 1.0], [1.0, 0.0]], [0, 1])
    with pytest.raises(ValueError, match=r"Precomputed metric requires shape \(n_queries, n_indexed\). Got \(3, 5\) for 3 indexed."):
        silhouette_samples(np.zeros((3, 5)), [0, 1, 1])
    with pytest.raises(ValueError, match="Expected 2D array, got 1D array instead"):
        silhouette_samples(torch.zeros(5), [0, 1, 1, 0, 0])


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """SSG_ERR_INVALID before any device call: null or misaligned pointers, a bad mode, mode 0 without v, m < 3, m > N, m != N without
    sel, a sel entry outside [0, N) in the host copy, K < 1, a bad Cmax, diag or state, state 1 with m too large, the global stage without
    its workspace; every message names its entry point"""
    from ssg_amd import _lib
    L = _lib.lib()
    P = lambda a: ctypes.c_void_p(a)      # noqa: E731  (never dereferenced: every call below is refused)
    M, v, C = P(0x10000), P(0x20000), P(0x80000)
    lim = L.ssg_silhouette_lds_max_m()
    assert lim % 2 == 0 and 16000 <= lim <= 160 * 1024 // 8 and (lim + 8) * 8 <= 160 * 1024
    sel_ok = (ctypes.c_int32 * 4)(3, 0, 2, 1)
    sel_high = (ctypes.c_int32 * 4)(3, 0, 8, 1)
    sel_neg = (ctypes.c_int32 * 4)(3, -1, 2, 1)
    sel_d = P(0x30000)
    good = dict(M=M, v=v, N=8, mode=1, sel=None, sel_host=None, m=8, atol=1e-14, count=C)
    bad_diag = [dict(M=None), dict(M=P(0x10001)), dict(M=P(0x10004), mode=2), dict(mode=3), dict(mode=-1), dict(mode=0, v=None), dict(v=P(0x20001), mode=0),
                dict(N=0, m=0), dict(m=0), dict(m=9), dict(m=4), dict(sel=sel_d, m=9), dict(sel=P(0x30002), m=4), dict(sel_host=sel_ok, m=4),
                dict(sel=sel_d, sel_host=sel_high, m=4), dict(sel=sel_d, sel_host=sel_neg, m=4), dict(count=None), dict(count=P(0x80004)), dict(atol=-1.0),
                dict(atol=float("nan"))]
    for change in bad_diag:
        a = dict(good)
        a.update(change)
        rc = L.ssg_silhouette_diag(a["M"], a["v"], a["N"], a["mode"], 0.3, a["sel"], a["sel_host"], a["m"], a["atol"], a["count"], None)
        assert rc == -1, change
        assert b"ssg_silhouette_diag" in L.ssg_last_error(), change
    lab, mem, st, ncl, ws, o1, o2, neg = P(0x100000), P(0x200000), P(0x300000), P(0x400000), P(0x500000), P(0x600000), P(0x700000), P(0x800000)
    big = lim + 2
    good = dict(M=M, v=v, N=8, mode=1, sel=None, sel_host=None, m=8, K=2, Cmax=3, lab=lab, mem=mem, st=st, ncl=ncl, diag=0, state=0, ws=ws, ws_bytes=64, o1=o1, o2=o2,
                neg=neg)
    bad_sums = [dict(M=None), dict(M=P(0x10001)), dict(M=P(0x10004), mode=2), dict(mode=3), dict(mode=-1), dict(mode=0, v=None), dict(v=P(0x20001), mode=0),
                dict(N=2, m=2), dict(sel=sel_d, m=2), dict(m=9), dict(m=4), dict(sel=sel_d, m=9), dict(sel=P(0x30002), m=4), dict(sel_host=sel_ok, m=4),
                dict(sel=sel_d, sel_host=sel_high, m=4), dict(sel=sel_d, sel_host=sel_neg, m=4), dict(K=0), dict(K=-1), dict(Cmax=0), dict(Cmax=9),
                dict(lab=None), dict(mem=None), dict(st=None), dict(ncl=None), dict(o1=None), dict(o2=None), dict(neg=None), dict(lab=P(0x100002)),
                dict(mem=P(0x200001)), dict(st=P(0x300002)), dict(ncl=P(0x400002)), dict(o1=P(0x600004)), dict(o2=P(0x700004)), dict(neg=P(0x800004)),
                dict(diag=2), dict(diag=-1), dict(state=3), dict(state=-1), dict(N=big, m=big, state=1), dict(N=big, m=big, state=0, ws=None),
                dict(N=big, m=big, state=2, ws_bytes=big * 8 - 8), dict(state=2, ws=None), dict(state=2, ws_bytes=56), dict(state=2, ws=P(0x500008))]
    for change in bad_sums:
        a = dict(good)
        a.update(change)
        rc = L.ssg_silhouette_sums(a["M"], a["v"], a["N"], a["mode"], 0.3, a["sel"], a["sel_host"], a["m"], a["K"], a["Cmax"], a["lab"], a["mem"], a["st"], a["ncl"],
                                   a["diag"], a["state"], a["ws"], a["ws_bytes"], a["o1"], a["o2"], a["neg"], None)
        assert rc == -1, change
        assert b"ssg_silhouette_sums" in L.ssg_last_error(), change
