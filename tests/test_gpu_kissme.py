"""GPU suite of KISSME (csrc/kissme.hip, ssg_amd/metric_learning.py, ssg_amd/dist_metric.py) on the cases of tests/kissme_ref.py.

    index pairs     ia1, ib1, ia0, ib0 of KISSME.fit equal the reference's (tests/golden/kissme_cases.npz) bit for bit, and the stream is
                    left where the reference's fit leaves it
    C1, C0          every element within (P + 2) 2^-53 A of the float64 restatement, A = sum_p |s_pi| |s_pj| / P: a length-P float64 sum in
                    any order plus the division (tests/train_common.bound with float64's unit); bitwise symmetric; two calls, same bits
    M before validation
                    with E = C_dev - C_64, |E| <= B elementwise and ||C^-1||_2 ||B||_F <= 1/2 (asserted), the Neumann series gives
                    ||(C + E)^-1 - C^-1||_F <= ||C^-1||_2^2 ||E||_F / (1 - ||C^-1||_2 ||E||_2) <= 2 ||C^-1||_2^2 ||B||_F, for C1 and C0
    transform       within (d + 2) 2^-24 A of X64 G64, A = |X| |G|: the rounding of G to float32 and a length-d float32 sum
    distances       pairwise_distance_device(..., metric) against (x - y)^T M (x - y) in float64, bound derived at the test
    Evaluator       a DistanceMetric('kissme') trained through .train prints the scores of the host restatement's distance matrix
    int64 scans     n = 131 072: y_i = i % 2 (exactly 2^32 non-matching pairs) with positions on both sides of 2^31, the last one 2^32 - 1 and
                    2^32 itself refused; y_i = i (8.59e9 pairs) with positions on both sides of 2^32
"""
import contextlib
import io

import numpy as np
import pytest

import kissme_ref as kr
from train_common import U, bound

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    return golden("kissme_cases.npz")


@pytest.fixture(scope="module")
def fits():
    """every case fitted once on the device with a RandomState(FIT_SEED): name -> (learner, stages, the stream's next draw, X, y, ref64)"""
    from ssg_amd.metric_learning import KISSME
    out = {}
    for name in sorted(kr.CASES):
        X, y = kr.make_case(name)
        rs = np.random.RandomState(kr.FIT_SEED[name])
        st = {}
        k = KISSME().fit(torch.from_numpy(X).cuda() if name in "AC" else X, y, rng=rs, stages=st)      # tensors on the device and numpy arrays
        nxt = rs.randint(0, 2 ** 31 - 1, size=4)
        out[name] = (k, st, nxt, X, y, kr.fit64(X, y, st["p"]))
    return out


@pytest.mark.parametrize("name", sorted(kr.CASES))
def test_index_pairs_and_stream_equal_the_references(g, fits, name):
    k, st, nxt, X, y, r = fits[name]
    assert sorted(st) == sorted(["ia1", "ib1", "p", "ia0", "ib0", "C1", "C0", "M_raw"])
    for key in ("ia1", "ib1", "p", "ia0", "ib0"):
        assert st[key].shape == g["%s_%s" % (name, key)].shape and np.array_equal(st[key], g["%s_%s" % (name, key)]), key
    assert np.array_equal(nxt, g[name + "_next"])
    assert k.metric() is k.M_ and k.M_.dtype == np.float64 and k.M_.shape == (X.shape[1],) * 2


def test_global_stream_and_seed(g):
    """rng=np.random consumes the global legacy stream as the reference does; an int seed leaves it alone"""
    from ssg_amd.metric_learning import KISSME
    X, y = kr.make_case("D")
    state = np.random.get_state()
    try:
        np.random.seed(kr.FIT_SEED["D"])
        st = {}
        KISSME().fit(X, y, stages=st)                            # rng defaults to np.random
        nxt = np.random.randint(0, 2 ** 31 - 1, size=4)
        assert np.array_equal(st["p"], g["D_p"]) and np.array_equal(st["ia0"], g["D_ia0"]) and np.array_equal(nxt, g["D_next"])
        before = np.random.get_state()[1].copy()
        st2 = {}
        KISSME().fit(X, y, rng=kr.FIT_SEED["D"], stages=st2)
        assert np.array_equal(st2["p"], g["D_p"]) and np.array_equal(np.random.get_state()[1], before)
    finally:
        np.random.set_state(state)
    with pytest.raises(ValueError):                              # numpy's own: fewer non-matching pairs than matching ones
        KISSME().fit(np.zeros((6, 16), np.float32), np.array([0, 0, 0, 0, 0, 1]), rng=0)
    with pytest.raises(ValueError, match="no matching pair"):
        KISSME().fit(np.zeros((6, 16), np.float32), np.arange(6), rng=0)


@pytest.mark.parametrize("name", sorted(kr.CASES))
def test_covariances_within_the_float64_bound(fits, name):
    from ssg_amd import metric_learning as ml
    k, st, _, X, y, r = fits[name]
    P, d = r["P"], X.shape[1]
    for key, bkey in (("C1", "B1"), ("C0", "B0")):
        err = np.abs(st[key] - r[key])
        worst = float((err / np.maximum(r[bkey], 1e-300)).max())
        print("%s %s: P = %d, max |dev - ref64| = %.3g, worst err / bound = %.3g" % (name, key, P, float(err.max()), worst))
        assert st[key].dtype == np.float64 and st[key].shape == (d, d) and np.isfinite(st[key]).all()
        assert (err <= r[bkey]).all(), "%s %s misses (P + 2) 2^-53 A by a factor of %.3g" % (name, key, worst)
        assert np.array_equal(st[key], st[key].T)                # the same bits on both sides of the diagonal
    # the entry point itself, twice: same bits; the zero columns of the padding give zero rows and columns
    Xd = ml._padded(X, torch.device("cuda"), 16)
    ia = torch.from_numpy(st["ia0"]).cuda(); ib = torch.from_numpy(st["ib0"]).cuda()
    a = ml.pairdiff_cov(Xd, ia, ib, P).cpu().numpy(); b = ml.pairdiff_cov(Xd, ia, ib, P).cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(a, a.T) and np.array_equal(a[:d, :d], st["C0"])
    assert not a[d:].any() and not a[:, d:].any()
    # pairs with an index outside [0, n) contribute nothing
    ia2 = torch.cat([ia[:5], torch.tensor([-1, 0, X.shape[0]], dtype=torch.int32).cuda(), ia[5:]])
    ib2 = torch.cat([ib[:5], torch.tensor([0, X.shape[0], 1], dtype=torch.int32).cuda(), ib[5:]])
    c = ml.pairdiff_cov(Xd, ia2, ib2, P).cpu().numpy()
    ref, A = kr.cov64(X, st["ia0"], st["ib0"], P)
    assert (np.abs(c[:d, :d] - ref) <= kr.cov_bound(P + 3, A)).all()


@pytest.mark.parametrize("name", sorted(kr.CASES))
def test_m_before_validation(fits, name):
    k, st, _, X, y, r = fits[name]
    lim = 0.0
    for ckey, bkey in (("C1", "B1"), ("C0", "B0")):
        inv2 = np.linalg.norm(np.linalg.inv(r[ckey]), 2)
        bf = np.linalg.norm(r[bkey], "fro")
        print("%s %s: cond = %.3g, ||C^-1||_2 ||B||_F = %.3g" % (name, ckey, np.linalg.cond(r[ckey]), inv2 * bf))
        assert inv2 * bf <= 0.5
        lim += 2.0 * inv2 * inv2 * bf
    err = np.linalg.norm(st["M_raw"] - r["M_raw"], "fro")
    print("%s: ||M_dev - M_64||_F = %.3g, bound %.3g (share %.3g)" % (name, err, lim, err / lim))
    assert err <= lim


@pytest.mark.parametrize("name", sorted(kr.CASES))
def test_transform_and_distances(fits, name):
    from ssg_amd import pairwise_distance_device
    k, st, _, X, y, r = fits[name]
    n, d = X.shape
    G = k.transformer()
    assert np.array_equal(G, np.tril(G)) and np.abs(G.dot(G.T) - k.M_).max() <= 1e-9 * np.abs(k.M_).max()
    X64 = X.astype(np.float64)
    Z = X64.dot(G)
    bz = bound(d, np.abs(X64).dot(np.abs(G)))
    for src in (X, torch.from_numpy(X), torch.from_numpy(X).cuda()):
        got = k.transform(src)
        assert type(got) is type(src) and got.dtype == src.dtype and got.shape == X.shape
        if torch.is_tensor(src):
            assert got.device == src.device
            got = got.cpu().numpy()
        err = np.abs(got.astype(np.float64) - Z)
        print("%s transform: max err %.3g, worst err / bound %.3g" % (name, float(err.max()), float((err / bz).max())))
        assert (err <= bz).all()
    assert np.array_equal(k.transform(), k.transform(X)) if not torch.is_tensor(k.X_) else torch.equal(k.transform(), k.transform(k.X_))
    # pairwise_distance_device through a DistanceMetric: the first third of the rows against the rest
    from ssg_amd.dist_metric import DistanceMetric
    dm = DistanceMetric("kissme"); dm.metric = k
    names = ["r%04d" % i for i in range(n)]
    feats = {f: torch.from_numpy(X[i]) for i, f in enumerate(names)}
    nq = n // 3
    query = [(names[i], int(y[i]), 0) for i in range(nq)]; gallery = [(names[i], int(y[i]), 1) for i in range(nq, n)]
    got = pairwise_distance_device(feats, query, gallery, metric=dm)
    assert got.is_cuda and got.shape == (nq, n - nq)
    diff = X64[:nq, None, :] - X64[None, nq:, :]
    ref = np.einsum("qgi,ij,qgj->qg", diff, k.M_, diff)
    # z' = z + e, |e| <= bz (above).  The block is |zx'|^2 + |zy'|^2 - 2 zx'.zy' in float32: the exact squared distance of the perturbed
    # rows differs from ||zx - zy||^2 by at most sum 2 |zx - zy| (ex + ey) + (ex + ey)^2, and the three length-d float32 sums with their
    # combination cost (d + 4) 2^-24 sum (|zx'| + |zy'|)^2 with |z'| <= |z| + e.  (||zx - zy||^2 = (x - y)^T G G^T (x - y), and G G^T = M.)
    zq, zg, eq, eg = Z[:nq, None, :], Z[None, nq:, :], bz[:nq, None, :], bz[None, nq:, :]
    lim = (2 * np.abs(zq - zg) * (eq + eg) + (eq + eg) ** 2).sum(-1) + (d + 4) * U * ((np.abs(zq) + eq + np.abs(zg) + eg) ** 2).sum(-1)
    # the invariant itself, in float64: ||(x - y) G||^2 = (x - y)^T M (x - y) up to the float64 roundings of cholesky and of both sums
    mag = np.einsum("qgi,ij,qgj->qg", np.abs(diff), np.abs(k.M_), np.abs(diff))
    assert (np.abs(((zq - zg) ** 2).sum(-1) - ref) <= 1e-11 * mag).all()
    lim = lim + 1e-11 * mag
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    print("%s distances: max err %.3g, worst err / bound %.3g" % (name, float(err.max()), float((err / lim).max())))
    assert (err <= lim).all()


def test_evaluator_with_a_trained_distance_metric(capsys):
    """DistanceMetric('kissme').train(model, loader) -> Evaluator(model).evaluate(loader, query, gallery, metric=) end to end.  The
    embedder is a stand-in (a ResNet object whose embed_with_flip reads the feature vector out of the first image row), so that the
    features are the float32 rows of a case-A-like set and the float64 restatement can be fitted on exactly the same numbers."""
    import ssg_amd
    from oracle import eval_oracle
    rs = np.random.RandomState(5)
    ids, per, d = 48, 8, 32
    cls = np.repeat(np.arange(ids), per)[rs.permutation(ids * per)]
    X = (2.0 * rs.standard_normal((ids, d))[cls] + rs.standard_normal((ids * per, d))).astype(np.float32)
    n = X.shape[0]
    imgs = torch.zeros(n, 3, 2, d); imgs[:, 0, 0, :] = torch.from_numpy(X)
    names = ["i%04d" % i for i in range(n)]; pids = [int(c) + 100 for c in cls]; cams = [int(i % 2) for i in range(n)]
    loader = [(imgs[b:b + 100], names[b:b + 100], pids[b:b + 100], cams[b:b + 100]) for b in range(0, n, 100)]
    model = ssg_amd.create("resnet18", num_classes=0, num_split=1, pretrained=False).cuda()
    model.embed_with_flip = lambda x, for_eval=False, check_overflow=True: x[:, 0, 0, :].to("cuda", torch.float32).contiguous()
    dm = ssg_amd.DistanceMetric("kissme")
    dm.train(model, loader, rng=21)
    assert dm.metric.M_.shape == (d, d) and torch.is_tensor(dm.metric.X_) and dm.metric.X_.is_cuda          # the features stayed on the device
    query = [(names[i], pids[i], cams[i]) for i in range(0, n, 4)]; gallery = [(names[i], pids[i], cams[i]) for i in range(n)]
    capsys.readouterr()
    top1 = ssg_amd.Evaluator(model, print_freq=0).evaluate(loader, query, gallery, metric=dm)
    printed = capsys.readouterr().out
    # host restatement: fit in float64 on the same rows, labels as the loader hands them (float32), the same draw
    y = np.asarray(pids, dtype=np.float32)
    _, _, m = kr.pair_order(y)
    p = np.random.RandomState(21).choice(int((~m).sum()), int(m.sum()), replace=False)
    M = ssg_amd.validate_cov_matrix(kr.fit64(X, y, p)["M_raw"])
    X64 = X.astype(np.float64)
    qi = np.arange(0, n, 4)
    diff = X64[qi, None, :] - X64[None, :, :]
    dist = np.einsum("qgi,ij,qgj->qg", diff, M, diff)
    with contextlib.redirect_stdout(io.StringIO()):
        mAP, scores, t1 = eval_oracle.evaluate_all(dist, [pids[i] for i in qi], pids, [cams[i] for i in qi], cams)
    expect = "Mean AP: {:4.1%}\n".format(mAP) + "CMC Scores{:>12}\n".format("market1501") + "".join(
        "top-{:<4}{:12.1%}\n".format(kk, scores[kk - 1]) for kk in (1, 5, 10))
    assert printed.endswith(expect), (printed, expect)
    assert top1 == t1 and 0.0 < mAP < 1.0 + 1e-12
    # the euclidean metric is the identity all the way through
    eu = ssg_amd.DistanceMetric()
    assert eu.train(model, loader) is None
    with contextlib.redirect_stdout(io.StringIO()):
        a = ssg_amd.Evaluator(model, print_freq=0).evaluate(loader, query, gallery, metric=eu)
        b = ssg_amd.Evaluator(model, print_freq=0).evaluate(loader, query, gallery)
    assert a == b


def test_int64_scans_beyond_2_to_the_32():
    """ssg_kissme_index + ssg_kissme_unrank alone at n = 131 072, no X and no match enumeration.
    y_i = i % 2 has 65 536^2 non-matching pairs, which is exactly 2^32: 1 000 positions, among them 0, the last (2^32 - 1), its
    neighbour and both sides of 2^31, against the numpy int64 restatement of the same rule; 2^32 and 2^32 + 1 lie outside this order and
    come back as (-1, -1).  Positions on both sides of 2^32 that are inside an order need more pairs than that: y_i = i (every pair
    non-matching, 8.59e9 of them) at the same n supplies them."""
    from ssg_amd import metric_learning as ml
    n = 131072
    y = np.arange(n) % 2
    ix = ml.pair_index(y)
    totals = ix["scans"][:, n].cpu().numpy()
    total = int(totals[1])
    assert total == 65536 * 65536 == 2 ** 32 and int(totals[0]) == n * (n - 1) // 2 - total
    rs = np.random.RandomState(3)
    special = [0, 1, total - 1, total - 2, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1]
    pos = np.concatenate([np.array(special, dtype=np.int64), rs.randint(0, total, size=1000 - len(special), dtype=np.int64)])
    a, b, tot = kr.unrank_rule(y, pos)
    assert tot == total and (a < b).all() and (y[a] != y[b]).all()
    ia, ib = ml.unrank(ix, pos)
    assert np.array_equal(ia.cpu().numpy(), a) and np.array_equal(ib.cpu().numpy(), b)
    # the sort itself: members ascending inside each class, rank = position in the class
    mem = ix["members"].cpu().numpy(); ptr = ix["cls_ptr"].cpu().numpy(); rank = ix["rank"].cpu().numpy()
    assert list(ptr) == [0, 65536, n] and np.array_equal(mem[:65536], np.arange(0, n, 2)) and np.array_equal(mem[65536:], np.arange(1, n, 2))
    assert np.array_equal(rank, np.arange(n) // 2)
    # positions outside the order come back as (-1, -1)
    ia, ib = ml.unrank(ix, np.array([-1, 2 ** 32, 2 ** 32 + 1, 5], dtype=np.int64))
    assert ia.cpu().tolist()[:3] == [-1, -1, -1] and ib.cpu().tolist()[:3] == [-1, -1, -1] and ia.cpu().tolist()[3] >= 0
    # every row a class of its own: the scan passes 2^32 inside the order
    y2 = np.arange(n)
    ix2 = ml.pair_index(y2)
    t2 = ix2["scans"][:, n].cpu().numpy()
    assert int(t2[0]) == 0 and int(t2[1]) == n * (n - 1) // 2 > 2 ** 32
    pos2 = np.concatenate([np.array([0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, int(t2[1]) - 1], dtype=np.int64),
                           rs.randint(0, int(t2[1]), size=93, dtype=np.int64)])
    a2, b2, _ = kr.unrank_rule(y2, pos2)
    assert np.array_equal(b2 * (b2 - 1) // 2 + a2, pos2)                 # the triangular numbering, in closed form
    ia2, ib2 = ml.unrank(ix2, pos2)
    assert np.array_equal(ia2.cpu().numpy(), a2) and np.array_equal(ib2.cpu().numpy(), b2)
