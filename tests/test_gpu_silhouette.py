"""GPU half of the silhouette tests: `ssg_amd.silhouette` (csrc/silhouette.hip) against what sklearn 1.7.2 gave for every case of
tests/silhouette_ref.py (tests/golden/silhouette_cases.npz), bit for bit.

Sizes 3, 7, 65, 513 and 1 030; two clusters of N / 2, N - 1 plus a singleton, pairs plus a triple, more clusters than a workgroup has
threads, negative and gapped labels; float64, float32 and float16 matrices, a matrix with negative entries (sklearn refuses it: the
public functions raise its message, the entry point's sums are held to the restatement), the mode-0 re-rank handle read in place;
ignore_noise; sample_size with all three kinds of random_state; silhouette_many with one blocking read; both placements of the stage;
the errors; generate_selflabel_sweep."""
import numpy as np
import pytest
import torch

import silhouette_ref as ref

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in ref.CASES]


@pytest.fixture(scope="module")
def gold():
    return ref.load_golden()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def rerank_handle(golden, dev):
    """the mode-0 handle re_ranking_device builds from the features of the re-rank golden whose final_dist the 'rerank' cases use"""
    from ssg_amd import rerank
    g = golden(ref.RERANK_FILE)
    h = rerank.re_ranking_device(torch.from_numpy(g["src"]).to(dev), torch.from_numpy(g["tgt"]).to(dev), k1=int(g["k1"]), k2=int(g["k2"]),
                                 lambda_value=ref.RERANK_LAMBDA)
    assert h.mode == 0 and h.group is None
    assert np.array_equal(h.final_dist().cpu().numpy(), np.asarray(ref.matrix(ref.BY_NAME["rerank_n256_few"])))
    return h


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _input(case, rerank_handle):
    return rerank_handle if case["kind"] == "rerank" else ref.matrix(case)


def _options(case):
    return dict(diagonal="zero" if case["kind"] == "rerank" else "check", ignore_noise=ref.ignore_noise(case))


@pytest.mark.parametrize("name", NAMES)
def test_samples_and_score_are_sklearn_s(gold, dev, rerank_handle, name):
    """silhouette_samples gives sklearn's per-sample result bit for bit and silhouette_score its mean, for every case; a float32 or
    float16 matrix gives the float64 copy's result as float64; the matrix with negative entries raises sklearn's refusal; the input is
    unchanged"""
    from ssg_amd import silhouette_samples, silhouette_score
    case = ref.BY_NAME[name]
    X, lab = _input(case, rerank_handle), gold[name + "/labels"]
    keep = X.M.clone() if case["kind"] == "rerank" else np.array(X)
    if case["kind"] == "neg":
        for fn in (silhouette_samples, silhouette_score):
            with pytest.raises(ValueError) as e:
                fn(X, lab)
            assert str(e.value) == str(gold[name + "/error"])
        return
    got = silhouette_samples(X, lab, **_options(case))
    assert _same_bits(got, gold[name + "/sil"]), name
    score = silhouette_score(X, lab, **_options(case))
    assert type(score) is float and score == float(gold[name + "/score"])
    assert torch.equal(X.M, keep) if case["kind"] == "rerank" else np.array_equal(np.array(X), keep)


def _entry_sums(L, h, enc_list, dev, sel=None, diag=0, state=0):
    """ssg_silhouette_sums called by name -> (intra [K, m], inter [K, m], negatives); the outputs start at a sentinel"""
    from ssg_amd import silhouette as sil
    from ssg_amd._lib import check, ptr
    m = h.N if sel is None else len(sel)
    K = len(enc_list)
    Cs = [int(e.max()) + 1 for e in enc_list]
    Cmax = max(Cs)
    lists = [sil._member_list(e, C) for e, C in zip(enc_list, Cs)]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)      # noqa: E731
    lab_d, mem_d = up(np.stack(enc_list)), up(np.stack([l[0] for l in lists]))
    start_d = up(np.stack([np.concatenate([l[1], np.full(Cmax - C, l[1][-1])]) for l, C in zip(lists, Cs)]))
    ncl_d = up(np.array(Cs))
    sel_h = None if sel is None else np.ascontiguousarray(sel, dtype=np.int32)
    sel_d = None if sel is None else up(sel_h)
    out = torch.full((2, K, m), -7.0, dtype=torch.float64, device=dev)
    neg = torch.full((1,), -7, dtype=torch.int64, device=dev)
    nblk = min(m, 5)                                                  # (fewer slices than rows: every workgroup walks several rows)
    ws = torch.empty(nblk * ((m + 1) & ~1), dtype=torch.float64, device=dev)
    check(L.ssg_silhouette_sums(ptr(h.M), ptr(h.v), h.N, h.mode, h.lambda_value, ptr(sel_d), None if sel_h is None else sel_h.ctypes.data, m, K, Cmax,
                                ptr(lab_d), ptr(mem_d), ptr(start_d), ptr(ncl_d), diag, state, ptr(ws), ws.numel() * 8, ptr(out[0]), ptr(out[1]), ptr(neg), None),
          "ssg_silhouette_sums")
    o = out.cpu().numpy()
    return o[0], o[1], int(neg.cpu()[0])


@pytest.mark.parametrize("state", [1, 2], ids=["lds", "global"])
@pytest.mark.parametrize("name", ["n65_neg", "n513_neg"])
def test_entry_point_sums_negative_entries_like_numpy(gold, dev, name, state):
    """ssg_silhouette_sums by name on the matrices with negative entries, both placements of the stage, two labelings in one call: the
    own cluster's sum and the smallest mean of another cluster are the restatement's bit for bit, and the count of negative entries
    is the matrix's"""
    from ssg_amd import _lib, hdbscan
    from ssg_amd import silhouette as sil
    case = ref.BY_NAME[name]
    X = ref.expected_input(case)
    h = hdbscan._as_handle(ref.matrix(case))
    other = (np.arange(case["N"]) * 7 % 11).astype(np.int64)
    encs = [sil._encode(gold[name + "/labels"], False)[0], sil._encode(other, False)[0]]
    intra, inter, neg = _entry_sums(_lib.lib(), h, encs, dev, state=state)
    for k, enc in enumerate(encs):
        want_intra, want_inter = ref.reduce_rows(X, enc, int(enc.max()) + 1)
        assert _same_bits(intra[k], want_intra) and _same_bits(inter[k], want_inter), (name, k)
    assert neg == int((X < 0).sum()) > 0


@pytest.mark.parametrize("state", [1, 2], ids=["lds", "global"])
def test_entry_points_with_a_selection_and_the_diagonal(gold, dev, rerank_handle, state):
    """ssg_silhouette_sums and ssg_silhouette_diag by name with a permuted selection on the re-rank handle: the sums are those of
    X[sel][:, sel] added in PERMUTED column order; diag = 1 takes the own entry as +0.0, diag = 0 as stored; positions labelled -1 keep
    their sentinels; the diagonal count follows the selection and atol"""
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr
    L = _lib.lib()
    h = rerank_handle
    X = np.array(ref.matrix(ref.BY_NAME["rerank_n256_few"]))
    sel = np.random.RandomState(5).permutation(h.N)[:101]
    sub = X[sel][:, sel]
    enc = (np.arange(101) % 6).astype(np.int32)
    enc[::9] = -1
    keep = enc >= 0
    for diag in (0, 1):
        S = sub.copy()
        if diag:
            np.fill_diagonal(S, 0.0)
        intra, inter, neg = _entry_sums(L, h, [enc], dev, sel=sel, diag=diag, state=state)
        want_intra, want_inter = ref.reduce_rows(S[keep][:, keep], enc[keep], 6)
        assert _same_bits(intra[0][keep], want_intra) and _same_bits(inter[0][keep], want_inter), diag
        assert (intra[0][~keep] == -7.0).all() and (inter[0][~keep] == -7.0).all() and neg == 0
    count = torch.full((1,), -7, dtype=torch.int64, device=dev)
    sel32 = np.ascontiguousarray(sel, dtype=np.int32)
    sel_d = torch.from_numpy(sel32).to(dev)
    d = np.abs(np.diag(X))
    for atol in (0.0, float(np.median(d[sel])), float(d.max())):
        check(L.ssg_silhouette_diag(ptr(h.M), ptr(h.v), h.N, h.mode, h.lambda_value, ptr(sel_d), sel32.ctypes.data, len(sel), atol, ptr(count), None), "ssg_silhouette_diag")
        assert int(count.cpu()[0]) == int((d[sel] > atol).sum()), atol
        check(L.ssg_silhouette_diag(ptr(h.M), ptr(h.v), h.N, h.mode, h.lambda_value, None, None, h.N, atol, ptr(count), None), "ssg_silhouette_diag")
        assert int(count.cpu()[0]) == int((d > atol).sum()), atol


def test_rerank_handle_with_its_diagonal_is_refused_and_left_alone(gold, dev, rerank_handle):
    """the re-rank matrix's diagonal is lambda * half(2 v_i): diagonal='check' raises sklearn's message; the handle is not modified"""
    from ssg_amd import silhouette_samples
    keep = rerank_handle.M.clone()
    with pytest.raises(ValueError) as e:
        silhouette_samples(rerank_handle, gold["rerank_n256_few/labels"], diagonal="check")
    assert str(e.value) == "The precomputed distance matrix contains non-zero elements on the diagonal. Use np.fill_diagonal(X, 0)."
    assert torch.equal(rerank_handle.M, keep)


@pytest.mark.parametrize("name", [c["name"] for c in ref.CASES if c.get("sample")])
def test_sampled_score_and_the_random_stream(gold, dev, name):
    """silhouette_score(sample_size=N // 2) with an int seed, a RandomState and the global stream: sklearn's score (the columns are added
    in the permuted order) and the stream left where sklearn leaves it; a refused X does not advance it"""
    from ssg_amd import silhouette_score
    case = ref.BY_NAME[name]
    X, lab, n = ref.matrix(case), gold[name + "/labels"], case["N"]
    want, nxt = float(gold[name + "/sampled_score"]), float(gold[name + "/next_draw"])
    assert silhouette_score(X, lab, sample_size=n // 2, random_state=ref.SAMPLE_SEED) == want
    rs = np.random.RandomState(ref.SAMPLE_SEED)
    assert silhouette_score(X, lab, sample_size=n // 2, random_state=rs) == want and rs.random_sample() == nxt
    saved = np.random.get_state()
    try:
        np.random.seed(ref.SAMPLE_SEED)
        assert silhouette_score(X, lab, sample_size=n // 2) == want and np.random.random_sample() == nxt
    finally:
        np.random.set_state(saved)
    bad = np.array(X)
    bad[1, 2] = np.nan
    rs = np.random.RandomState(ref.SAMPLE_SEED)
    with pytest.raises(ValueError, match="Input X contains NaN."):
        silhouette_score(bad, lab, sample_size=n // 2, random_state=rs)
    assert rs.random_sample() == np.random.RandomState(ref.SAMPLE_SEED).random_sample()


@pytest.mark.parametrize("K", [1, 3, 9])
def test_many_is_the_single_calls_from_one_read(gold, dev, K, monkeypatch):
    """silhouette_many with K labelings of different cluster counts: each result is the single-labeling call's, bit for bit, with and
    without per-labeling noise sets; one blocking read for the whole call"""
    from ssg_amd import silhouette, silhouette_many, silhouette_samples
    case = ref.BY_NAME["n513_few"]
    X, n = ref.matrix(case), case["N"]
    rs = np.random.RandomState(40 + K)
    labelings = [gold["n513_few/labels"], gold["n513_halves/labels"], gold["n513_big_single/labels"]][:K]
    labelings += [rs.randint(0, 2 + 37 * k, n) for k in range(K - len(labelings))]
    singles = [silhouette_samples(X, l) for l in labelings]
    reads = []
    real = silhouette._read_back
    monkeypatch.setattr(silhouette, "_read_back", lambda *t: reads.append(len(t)) or real(*t))
    got = silhouette_many(X, labelings)
    assert len(reads) == 1 and len(got) == K
    for k in range(K):
        assert _same_bits(got[k], singles[k]), k
    assert _same_bits(got[0], gold["n513_few/sil"])
    # every labeling with its own noise set (the first one without any noise)
    noisy = [np.array(l) for l in labelings]
    for k in range(1, K):
        noisy[k][rs.permutation(n)[:40 * k]] = -1
    if K >= 3:
        noisy[2][labelings[2] == 1] = 1                           # (the singleton stays, or one label would be left)
    if K == 1:
        noisy[0] = np.array(gold["n513_noise/labels"])
    monkeypatch.setattr(silhouette, "_read_back", real)
    singles = [silhouette_samples(X, l, ignore_noise=True) for l in noisy]
    del reads[:]
    monkeypatch.setattr(silhouette, "_read_back", lambda *t: reads.append(len(t)) or real(*t))
    got = silhouette_many(X, noisy, ignore_noise=True)
    assert len(reads) == 1
    for k in range(K):
        assert _same_bits(got[k], singles[k]) and np.array_equal(np.isnan(got[k]), noisy[k] == -1), k
    if K > 1:
        # an invalid labeling is named by its index
        with pytest.raises(ValueError, match=r"^labeling 1: Number of labels is 1\. Valid values are 2 to n_samples - 1 \(inclusive\)$"):
            silhouette_many(X, [labelings[0], np.zeros(n, dtype=int)] + labelings[2:])


def test_state_placement(gold, dev):
    """the stage in global memory gives the bits of the stage in LDS at N = 513 (one past a 512-entry chunk); state=1 beyond
    ssg_silhouette_lds_max_m() is refused"""
    from ssg_amd import _lib, silhouette_many, silhouette_samples
    for name in ("n513_halves", "n513_pairs_f16", "n513_noise"):
        case = ref.BY_NAME[name]
        a = silhouette_samples(ref.matrix(case), gold[name + "/labels"], state=1, ignore_noise=ref.ignore_noise(case))
        b = silhouette_samples(ref.matrix(case), gold[name + "/labels"], state=2, ignore_noise=ref.ignore_noise(case))
        assert _same_bits(a, b) and _same_bits(a, gold[name + "/sil"]), name
    n = _lib.lib().ssg_silhouette_lds_max_m() + 2
    big = torch.zeros((n, n), dtype=torch.float16, device=dev)
    with pytest.raises(ValueError, match=r"ssg_silhouette_sums: state=1 \(LDS\) holds at most m=%d samples, got m=%d" % (n - 2, n)):
        silhouette_many(big, [np.arange(n) % 2], state=1)


@pytest.mark.parametrize("n", [5300, 10400])
def test_wider_workgroups_give_the_same_bits(dev, n):
    """above m = 5 088 a CU's LDS holds fewer than four stages and a workgroup gets 512 threads, above m = 10 208 fewer than two and
    1 024 threads: at one size past each threshold the result equals the 256-thread workgroups of the global placement bit for bit, and
    on a few rows numpy's own `np.bincount(labels, weights=row)` followed by sklearn's lines"""
    from ssg_amd import _lib, silhouette_many
    assert (160 * 1024) // (8 * 5300 + 256) == 3 and (160 * 1024) // (8 * 10400 + 256) == 1 and n <= _lib.lib().ssg_silhouette_lds_max_m()
    g = torch.Generator(device=dev).manual_seed(n)
    X = (torch.rand((n, n), generator=g, device=dev) * 2.0).to(torch.float16)
    X.fill_diagonal_(0.0)
    rs = np.random.RandomState(n)
    labelings = [rs.randint(0, 700, n), (np.arange(n) * 13 % 3)]
    lds = silhouette_many(X, labelings, state=1)
    glob = silhouette_many(X, labelings, state=2)
    for a, b in zip(lds, glob):
        assert _same_bits(a, b)
    for i in (0, 1, n // 2 + 3, n - 1):
        row = X[i].cpu().numpy().astype(np.float64)
        for lab, got in zip(labelings, lds):
            classes, enc = np.unique(lab, return_inverse=True)
            freq = np.bincount(enc)
            s = np.bincount(enc, weights=row, minlength=len(classes))
            intra = s[enc[i]] / max(freq[enc[i]] - 1, 1)
            s[enc[i]] = np.inf
            inter = (s / freq).min()
            assert got[i] == ((inter - intra) / max(intra, inter) if freq[enc[i]] > 1 else 0.0), (n, i)


def test_errors_in_sklearn_s_order(gold, dev):
    """NaN and infinity from the device counts, with sklearn's messages, before the length of the labels, the diagonal and the number of
    labels; a diagonal of 1e-3 raises, one of 1e-15 passes (the float64 atol is 2.2e-14); a row-sharded handle is refused"""
    from ssg_amd import silhouette_many, silhouette_samples, silhouette_score
    from ssg_amd.rerank import DistHandle
    case = ref.BY_NAME["n65_halves"]
    base, lab = np.array(ref.matrix(case)), gold["n65_halves/labels"]
    n = len(lab)
    nlab = "Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)"
    diag = "The precomputed distance matrix contains non-zero elements on the diagonal. Use np.fill_diagonal(X, 0)."

    def raises(text, fn, *a, **kw):
        with pytest.raises(ValueError) as e:
            fn(*a, **kw)
        assert str(e.value) == text, str(e.value)

    for (i, j) in ((3, 40), (64, 0), (7, 7), (64, 64)):
        X = base.copy()
        X[i, j] = np.nan
        X[5, 5] = 1e-3                                            # NaN comes before the diagonal, the length and the number of labels
        raises("Input X contains NaN.", silhouette_samples, X, lab)
        raises("Input X contains NaN.", silhouette_samples, X, lab[:-1])
        raises("Input X contains NaN.", silhouette_score, X, np.zeros(n, dtype=int))
        raises("Input X contains NaN.", silhouette_samples, X, lab, diagonal="zero")
        for bad in (np.inf, -np.inf):
            X[i, j] = bad
            raises("Input X contains infinity or a value too large for dtype('float64').", silhouette_samples, X, lab)
            raises("Input X contains infinity or a value too large for dtype('float32').", silhouette_many, X.astype(np.float32), [lab, lab])
    X = base.copy()
    X[5, 5] = 1e-3
    raises("Found input variables with inconsistent numbers of samples: [65, 64]", silhouette_samples, X, lab[:-1])
    raises(diag, silhouette_samples, X, lab)
    raises(diag, silhouette_samples, X, np.zeros(n, dtype=int))     # the diagonal comes before the number of labels
    raises(diag, silhouette_samples, X.astype(np.float32), lab)
    assert _same_bits(silhouette_samples(X, lab, diagonal="zero"), gold["n65_halves/sil"])
    X[5, 5] = 1e-15
    assert np.isfinite(silhouette_samples(X, lab)).all()
    X[5, 5] = -1e-15                                              # passes the diagonal check; sklearn then refuses it as a negative distance
    raises("Negative values in data passed to `pairwise_distances`. Precomputed distance  need to have non-negative values..", silhouette_samples, X, lab)
    raises(nlab % 1, silhouette_samples, X, np.zeros(n, dtype=int))   # the number of labels comes before the negative entries
    assert _same_bits(silhouette_samples(X, lab, diagonal="zero"), gold["n65_halves/sil"])
    X[5, 5] = 3e-14
    raises(diag, silhouette_samples, X, lab)
    assert np.isfinite(silhouette_samples(X.astype(np.float32), lab)).all()        # (the float32 atol is 1.2e-5)
    raises(nlab % 1, silhouette_samples, base, np.zeros(n, dtype=int))
    raises(nlab % n, silhouette_samples, base, np.arange(n))
    raises(nlab % n, silhouette_score, base, np.arange(n))
    raises(nlab % 2, silhouette_samples, base[:2, :2], [0, 1])
    raises(nlab % 1, silhouette_samples, base, np.where(np.arange(n) % 2, -1, 4), ignore_noise=True)
    raises(nlab % 32, silhouette_score, base, np.arange(n), sample_size=32, random_state=0)
    d = torch.from_numpy(base).to(dev)
    sharded = DistHandle(n, 2, d[:32].contiguous(), row0=0, nrows=32, group=object())
    with pytest.raises(ValueError, match="row-sharded DistHandle is not supported"):
        silhouette_samples(sharded, lab)


def test_generate_selflabel_sweep(dev, rerank_handle, capsys):
    """the eps sweep over two iterations: estimator and eps0 cached at iteration 0 (the rho rule, printed with the reference's line); every
    iteration one fit, the cuts at eps0 * f, one scoring pass; the labels of the chosen cut are cluster_optics_dbscan's at that eps and
    the printed choice is select_cut's on the scores of silhouette_many"""
    from types import SimpleNamespace
    from ssg_amd import OPTICS, cluster, cluster_optics_dbscan, generate_selflabel_sweep, silhouette_many
    from ssg_amd.silhouette import cut_is_valid, select_cut
    h = rerank_handle
    rho = 2e-2
    eps0 = float(cluster.eps_rule(h, rho)[0])
    factors = [0.6, 0.8, 1.0, 1.25, 1.5]
    args = SimpleNamespace(no_rerank=False, rho=rho)
    labels, cl = generate_selflabel_sweep([[]], [h], 0, args, cluster_list=[])
    est = cl[0]
    assert len(cl) == 1 and isinstance(est, OPTICS) and (est.eps, est.min_samples, est.cluster_method, est.metric) == (eps0, 4, "dbscan", "precomputed")
    cuts = [cluster_optics_dbscan(reachability=est.reachability_, core_distances=est.core_distances_, ordering=est.ordering_, eps=eps0 * f) for f in factors]
    best, scores = select_cut(factors, cuts, lambda v: silhouette_many(h, v, diagonal="zero", ignore_noise=True))
    valid = [cut_is_valid(c) for c in cuts]
    assert any(valid) and not all(valid), "the matrix shows both cuts that can be scored and cuts that cannot"
    assert np.array_equal(labels[0], cuts[best]) and est.sweep_factor_ == factors[best] and est.sweep_eps_ == eps0 * factors[best]
    assert est.sweep_scores_ == scores and np.array_equal(est.labels_, labels[0])
    sils = silhouette_many(h, [c for c, ok in zip(cuts, valid) if ok], diagonal="zero", ignore_noise=True)
    want = [float(np.nansum(s)) / h.N for s in sils]
    assert [s for s in scores if s is not None] == pytest.approx(want, rel=1e-12) and max(want) == pytest.approx(scores[best], rel=1e-12)
    assert [s is None for s in scores] == [not ok for ok in valid]
    out = capsys.readouterr().out
    ids = len(set(labels[0][labels[0] >= 0].tolist()))
    assert 'eps in cluster: {:.3f}'.format(eps0) in out and "Clustering and labeling..." in out and "Iteration 1 have %d training ids" % ids in out
    assert "-> factor %s (eps %.3f)" % (factors[best], eps0 * factors[best]) in out and "skipped" in out
    args2 = SimpleNamespace(no_rerank=False, rho=0.5, sweep_factors=(1.0, 1.5), sweep_min_samples=9)   # eps0 and the estimator are frozen
    labels2, cl2 = generate_selflabel_sweep([[]], [h], 1, args2, cluster_list=cl)
    out = capsys.readouterr().out
    assert cl2[0] is est and est.eps == eps0 and est.min_samples == 4 and "eps in cluster" not in out and "Iteration 2 have" in out
    cuts2 = [cuts[2], cuts[4]]
    best2, _ = select_cut((1.0, 1.5), cuts2, lambda v: silhouette_many(h, v, diagonal="zero", ignore_noise=True))
    assert np.array_equal(labels2[0], cuts2[best2]) and est.sweep_factor_ == (1.0, 1.5)[best2]
