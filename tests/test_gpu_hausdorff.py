"""GPU suite of the Hausdorff re-ranking variant (ssg_amd.rerank_hausdorff, csrc/hausdorff.hip).  Everything is compared bit for bit:
against the goldens the reference wrote (tests/golden/hausdorff_cases.npz) and, stage by stage and for the entry points called by
name, against the numpy restatement tests/hausdorff_ref.py (itself held against the goldens by tests/test_hausdorff_host.py)."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import hausdorff_ref
from conftest import GOLDEN, bits, clustered

pytestmark = pytest.mark.gpu

CASES = hausdorff_ref.load_cases(os.path.join(GOLDEN, "hausdorff_cases.npz"))
_REF = {}


def ref_of(name):
    """the restatement's stages of one golden case (computed once, never modified)"""
    if name not in _REF:
        c = CASES[name]
        _REF[name] = hausdorff_ref.re_ranking(c["src"], c["tgt"], c["k"], c["lambda_value"], c["MemorySave"])
    return _REF[name]


def dev_sets(stages):
    idx, nnz = stages["a_idx"].cpu().numpy(), stages["a_nnz"].cpu().numpy()
    return [idx[i, :nnz[i]] for i in range(len(nnz))]


def P(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("name", sorted(CASES))
def test_goldens_bit_for_bit_with_every_stage(name, capsys):
    from ssg_amd import rerank_hausdorff as rh
    c = CASES[name]
    e, f = rh.re_ranking(c["src"], c["tgt"], k=c["k"], lambda_value=c["lambda_value"], MemorySave=c["MemorySave"], Minibatch=c["Minibatch"])
    assert capsys.readouterr().out == "computing source distance...\ncomputing original distance...\n"
    assert e.dtype == np.float16 and f.dtype == np.float64 and e.shape == f.shape == c["final_dist"].shape
    assert np.array_equal(bits(e), bits(c["euclidean_dist"]))
    assert np.array_equal(np.asarray(f), c["final_dist"])
    assert f.valid_handle() is not None and f.valid_handle().mode == 2          # DBSCAN.fit_predict(final_dist) needs no re-upload
    r, stages = ref_of(name), {}
    dev = torch.device("cuda", 0)
    h = rh.re_ranking_hausdorff_device(torch.from_numpy(c["src"]).to(dev), torch.from_numpy(c["tgt"]).to(dev), k=c["k"], lambda_value=c["lambda_value"],
                                       stages=stages, memory_save=c["MemorySave"])
    assert sorted(stages) == ["D", "E", "H", "a_idx", "a_nnz", "vec"]
    assert np.array_equal(bits(stages["D"].cpu().numpy()), bits(r["D"]))
    assert np.array_equal(stages["vec"].cpu().numpy(), r["vec"])
    got = dev_sets(stages)
    assert all(np.array_equal(g, s) for g, s in zip(got, r["sets"])) and all(i not in g for i, g in enumerate(got))
    assert np.array_equal(stages["E"].cpu().numpy(), r["E"])
    assert np.array_equal(stages["H"].cpu().numpy(), r["H"])
    assert h.mode == 2 and h.M.dtype == torch.float64 and h.euclid.dtype == torch.float16
    # a second call returns identical bits
    assert np.array_equal(h.final_dist().cpu().numpy(), np.asarray(f)) and np.array_equal(bits(h.euclid.cpu().numpy()), bits(e))


def test_capacity_retry_for_tie_heavy_rows():
    """70 copies of one row: their sets hold the 69 other copies -- more than the first capacity of 64 -- so the sets are built twice"""
    from ssg_amd import rerank_hausdorff as rh
    tgt = clustered(100, 24, seed=5)
    tgt[:70] = tgt[0]
    src = clustered(12, 24, seed=6)
    r = hausdorff_ref.re_ranking(src, tgt, 4, 0.1)
    assert max(len(s) for s in r["sets"]) > 64
    stages = {}
    h = rh.re_ranking_hausdorff_device(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), k=4, lambda_value=0.1, stages=stages)
    assert stages["a_idx"].shape[1] == 100
    assert all(np.array_equal(g, s) for g, s in zip(dev_sets(stages), r["sets"]))
    assert np.array_equal(stages["H"].cpu().numpy(), r["H"]) and np.array_equal(h.final_dist().cpu().numpy(), r["final_dist"])


def _wide_rows(rng, m, d):
    """float32 rows whose norms spread over four decades: an operand taken from the wrong row or column shows in every digit"""
    return (rng.standard_normal((m, d)) * 10.0 ** rng.uniform(-2, 2, (m, 1))).astype(np.float32)


@pytest.mark.parametrize("m,n,d", [(1, 1, 1), (3, 5, 7), (65, 33, 40), (130, 97, 2048), (257, 64, 100)])
def test_distance_entry_points_by_name(m, n, d):
    from ssg_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(m * 1000 + n)
    x, y = _wide_rows(rng, m, d), _wide_rows(rng, n, d)
    s = hausdorff_ref.seq_sqdist(x, y)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    st = _lib.stream()

    def framed(rows, cols):
        """a [rows, cols] view in the middle of a NaN-filled buffer: a write outside the view shows"""
        buf = torch.full((rows + 2, cols + 5), float("nan"), dtype=torch.float64, device="cuda")
        return buf, buf[1:rows + 1, 2:cols + 2]

    def frame_untouched(buf, rows, cols):
        b = buf.clone()
        b[1:rows + 1, 2:cols + 2] = float("nan")
        return bool(torch.isnan(b).all())

    for take_sqrt, want in ((0, s), (1, np.sqrt(s))):
        buf, view = framed(m, n)
        _lib.check(L.ssg_seqdist_f64(P(xd), m, P(yd), n, d, take_sqrt, P(view), buf.shape[1], st), "ssg_seqdist_f64")
        assert np.array_equal(view.cpu().numpy(), want) and frame_untouched(buf, m, n)
    # self form: the block form's bits, exactly symmetric, zero diagonal
    blk = torch.empty((m, m), dtype=torch.float64, device="cuda")
    _lib.check(L.ssg_seqdist_f64(P(xd), m, P(xd), m, d, 1, P(blk), m, st), "ssg_seqdist_f64")
    buf, view = framed(m, m)
    _lib.check(L.ssg_seqdist_self_f64(P(xd), m, d, 1, P(view), buf.shape[1], st), "ssg_seqdist_self_f64")
    got = view.cpu().numpy()
    assert np.array_equal(got, blk.cpu().numpy()) and np.array_equal(got, np.sqrt(hausdorff_ref.seq_sqdist(x, x))) and frame_untouched(buf, m, m)
    assert np.array_equal(got, got.T) and not got.diagonal().any()
    # row minimum (of the squared sums), then the source vector
    buf = torch.full((m + 2,), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(L.ssg_seqdist_rowmin_f64(P(xd), m, P(yd), n, d, P(buf[1:]), st), "ssg_seqdist_rowmin_f64")
    assert np.array_equal(buf[1:m + 1].cpu().numpy(), s.min(axis=1)) and bool(torch.isnan(buf[[0, m + 1]]).all())
    vec = torch.full((m + 2,), float("nan"), dtype=torch.float64, device="cuda"); vmax = torch.zeros(1, dtype=torch.float64, device="cuda")
    _lib.check(L.ssg_hausdorff_source_finish(P(buf[1:]), m, P(vec[1:]), P(vmax), st), "ssg_hausdorff_source_finish")
    v = np.sqrt(s.min(axis=1))
    assert vmax.item() == v.max() and np.array_equal(vec[1:m + 1].cpu().numpy(), v / v.max()) and bool(torch.isnan(vec[[0, m + 1]]).all())


def test_row_minimum_with_several_column_tiles_per_workgroup():
    """65 row tiles leave 31 column slices for 40 column tiles: two tiles per workgroup, combined over the slices"""
    from ssg_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(3)
    x, y = _wide_rows(rng, 4100, 3), _wide_rows(rng, 2500, 3)
    out = torch.empty(4100, dtype=torch.float64, device="cuda")
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()      # held until the result is read: a temporary's block can be handed out again
    _lib.check(L.ssg_seqdist_rowmin_f64(P(xd), 4100, P(yd), 2500, 3, P(out), _lib.stream()), "ssg_seqdist_rowmin_f64")
    assert np.array_equal(out.cpu().numpy(), hausdorff_ref.seq_sqdist(x, y).min(axis=1))


def _hand_sets(rng, N, kind):
    sets = []
    for i in range(N):
        others = np.delete(np.arange(N), i)
        size = {"one": 1, "mixed": int(rng.integers(1, min(40, N - 1) + 1)), "all": N - 1}[kind]
        sets.append(np.sort(rng.choice(others, size=size, replace=False)))
    return sets


def _hausdorff_all_but_self(E):
    """the numpy max-min for S_i = everything but i, without the N^2/2 sub-blocks: leaving column j out of a row changes its minimum
    only where the minimum sits in column j (then the second smallest takes over); the same for the largest column minimum"""
    N = E.shape[0]
    H = np.zeros((N, N))
    for i in range(N):
        A = np.delete(E, i, axis=0)                               # rows S_i, all columns
        two = np.partition(A, 1, axis=1)[:, :2]
        R = np.repeat(two[:, :1], N, axis=1)
        R[np.arange(N - 1), A.argmin(axis=1)] = two[:, 1]         # R[a, j] = min over b != j of A[a, b]
        cm = A.min(axis=0)
        top = np.sort(cm)[-2:]
        d2 = np.full(N, top[1]); d2[cm.argmax()] = top[0]         # max over b != j of the column minima
        H[i] = np.maximum(R.max(axis=0), d2)
        H[i, i] = 0.0
    return H


@pytest.mark.parametrize("kind", ["one", "mixed", "all"])
@pytest.mark.parametrize("N", [5, 64, 97, 257])
def test_hausdorff_entry_points_by_name(N, kind):
    from ssg_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(N)
    E = rng.random((N, N)); E = np.maximum(E, E.T); np.fill_diagonal(E, 0.0)
    sets = _hand_sets(rng, N, kind)
    cap = max(len(s) for s in sets) + 3
    idx = np.full((N, cap), -7, dtype=np.int32)                 # entries past a_nnz are never read
    for i, s in enumerate(sets):
        idx[i, :len(s)] = s
    nnz = np.array([len(s) for s in sets], dtype=np.int32)
    Ed, idxd, nnzd = torch.from_numpy(E).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(nnz).cuda()
    st = _lib.stream()

    def run(ranges):
        G = torch.full((N, N), float("nan"), dtype=torch.float64, device="cuda")
        for r0, nr in ranges:
            nws = int(L.ssg_hausdorff_workspace_bytes(N, nr))
            ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
            _lib.check(L.ssg_hausdorff_directed_rows(P(Ed), P(idxd), P(nnzd), cap, N, r0, nr, P(G), P(ws), nws, st), "ssg_hausdorff_directed_rows")
        hmax = torch.full((1,), 5.0, dtype=torch.float64, device="cuda")
        _lib.check(L.ssg_hausdorff_symmetrize(P(G), N, P(hmax), st), "ssg_hausdorff_symmetrize")
        return G.cpu().numpy(), hmax.item()

    H, hmax = run([(0, N)])
    # (33 000 sub-blocks of 256 x 256 are too many for the host's pair loop: the closed form of these sets instead, held against
    # the pair loop on the three smaller sizes)
    want = _hausdorff_all_but_self(E) if kind == "all" else hausdorff_ref.hausdorff_from_sets(E, sets)
    if kind == "all" and N < 257:
        assert np.array_equal(want, hausdorff_ref.hausdorff_from_sets(E, sets))
    assert np.array_equal(H, want) and hmax == want.max()
    assert np.array_equal(H, H.T) and not H.diagonal().any() and hmax == H.max()
    # row ranges that split the matrix give the same bits as one call
    H2, hmax2 = run([(N // 3, N - N // 3), (0, N // 3)] if N >= 3 else [(0, N)])
    assert np.array_equal(H2, H) and hmax2 == hmax
    # blend over a row block, in place and into a framed buffer
    lam = 0.3
    vec = rng.random(N)
    want = (H / hmax) * (1 - lam) + (vec[None, :] + vec[:, None]) * lam
    Hd, vd, hm = torch.from_numpy(H).cuda(), torch.from_numpy(vec).cuda(), torch.tensor([hmax], dtype=torch.float64, device="cuda")
    r0 = N // 2
    out = torch.full((N - r0 + 2, N), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(L.ssg_hausdorff_blend(P(Hd[r0:]), P(hm), P(vd), N, r0, N - r0, 1 - lam, lam, P(out[1:]), st), "ssg_hausdorff_blend")
    assert np.array_equal(out[1:-1].cpu().numpy(), want[r0:]) and bool(torch.isnan(out[[0, -1]]).all())
    _lib.check(L.ssg_hausdorff_blend(P(Hd), P(hm), P(vd), N, 0, N, 1 - lam, lam, P(Hd), st), "ssg_hausdorff_blend")
    assert np.array_equal(Hd.cpu().numpy(), want)


@pytest.mark.parametrize("N", [3, 130])
def test_half_div_max_by_name(N):
    from ssg_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(N)
    D = (rng.random((N, N)) * 3.7).astype(np.float16)
    rowmax = torch.from_numpy(D.max(axis=1).view(np.uint16).astype(np.int32)).cuda()
    out = torch.full((N * N + 8,), float("nan"), dtype=torch.float16, device="cuda")
    gmax = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    _lib.check(L.ssg_half_div_max(P(torch.from_numpy(D).cuda()), P(rowmax), N, P(out[4:]), P(gmax[1:]), _lib.stream()), "ssg_half_div_max")
    assert gmax.tolist() == [-1, int(D.max().view(np.uint16)), -1]
    assert np.array_equal(bits(out[4:-4].cpu().numpy().reshape(N, N)), bits(D / np.max(D))) and bool(torch.isnan(out[:4]).all() and torch.isnan(out[-4:]).all())


def test_nan_conditions_are_raised_from_status_words():
    from ssg_amd import ReRankNaNError
    from ssg_amd import rerank_hausdorff as rh
    tgt = clustered(80, 16, seed=3)
    with pytest.raises(ReRankNaNError, match=r"rerank_hausdorff\.py:15"):          # every target row is a source row as well: vec == 0
        rh.re_ranking(np.concatenate([tgt, clustered(5, 16, seed=4)]), tgt, k=4)
    same = np.repeat(tgt[:1], 80, axis=0)
    with pytest.raises(ReRankNaNError, match=r"rerank_hausdorff\.py:60"):          # all target rows identical: H == 0
        rh.re_ranking(clustered(7, 16, seed=4), same, k=4)
    torch.cuda.synchronize()                                                       # neither is a GPU fault: the device goes on working
    e, f = rh.re_ranking(clustered(7, 16, seed=4), tgt, k=4)
    assert not np.isnan(f).any()


def _expected_pairs(X, sets, pi, pj):
    """H[i, j] of the listed pairs from the features: sets padded to one length by repeating a member (min and max ignore duplicates)"""
    m = max(len(sets[i]) for i in set(pi.tolist()) | set(pj.tolist()))
    pad = lambda s: np.concatenate([s, np.repeat(s[:1], m - len(s))])      # noqa: E731
    A = X[np.stack([pad(sets[i]) for i in pi])]                 # [P, m, d] float64
    B = X[np.stack([pad(sets[j]) for j in pj])]
    s = np.zeros((len(pi), m, m))
    for c in range(X.shape[1]):
        t = A[:, :, None, c] - B[:, None, :, c]
        s = s + t * t
    e = np.sqrt(s)
    return np.maximum(e.min(axis=2).max(axis=1), e.min(axis=1).max(axis=1))


def test_byte_offsets_above_2_to_31():
    """N = 16 400: 8 N^2 bytes pass 2^31 (from N = 16 385 on).  Expected values come from the features for the sampled pairs only; the
    sets come from the device's half matrix (checked bit for bit elsewhere); the two global maxima are located on the device and their
    values recomputed on the host."""
    from ssg_amd import rerank_hausdorff as rh
    N, Ns, d, k, lam = 16400, 64, 32, 6, 0.1
    tgt, src = clustered(N, d, seed=1), clustered(Ns, d, seed=2)
    stages = {}
    h = rh.re_ranking_hausdorff_device(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), k=k, lambda_value=lam, stages=stages)
    F = h.final_dist()
    assert F.shape == (N, N) and 8 * N * N > 2 ** 31
    # sets from the device D
    D = stages["D"].float()
    mask = D <= torch.kthvalue(D, k, dim=1).values[:, None]
    mask.fill_diagonal_(False)
    cnt = mask.sum(dim=1).cpu().numpy()
    members = mask.nonzero()[:, 1].cpu().numpy()
    sets = np.split(members, np.cumsum(cnt)[:-1])
    del D, mask
    # source vector on the host
    vec = np.sqrt(hausdorff_ref.seq_sqdist(tgt, src).min(axis=1))
    vec = vec / vec.max()
    assert np.array_equal(stages["vec"].cpu().numpy(), vec)
    # max(H): where the device found it, recomputed from the features
    Hd = stages["H"]
    hmax = Hd.max().item()
    am = int(Hd.argmax().item())
    X = tgt.astype(np.float64)
    assert _expected_pairs(X, sets, np.array([am // N]), np.array([am % N]))[0] == hmax
    rng = np.random.default_rng(9)
    pi = np.concatenate([rng.integers(0, N, 2000), np.full(N, N - 1)])
    pj = np.concatenate([rng.integers(0, N, 2000), np.arange(N)])
    Hexp = _expected_pairs(X, sets, pi, pj)
    Hexp[pi == pj] = 0.0
    assert Hexp.max() <= hmax
    want = (Hexp / hmax) * (1 - lam) + (vec[pj] + vec[pi]) * lam
    got = F[torch.from_numpy(pi).cuda(), torch.from_numpy(pj).cuda()].cpu().numpy()
    assert np.array_equal(Hd[torch.from_numpy(pi).cuda(), torch.from_numpy(pj).cuda()].cpu().numpy(), Hexp)
    assert np.array_equal(got, want)
    assert np.array_equal(F[N - 1].cpu().numpy(), want[2000:])                    # the whole last row
    si, sj = torch.from_numpy(rng.integers(0, N, 100000)).cuda(), torch.from_numpy(rng.integers(0, N, 100000)).cuda()
    assert torch.equal(F[si, sj], F[sj, si])


def test_chain_eps_rule_dbscan_and_compute_dist(ora):
    from ssg_amd import cluster, rerank
    from ssg_amd import rerank_hausdorff as rh
    from ssg_amd.selftraining import compute_dist, generate_selflabel
    c = CASES["b"]
    rho = 3e-2                                                                    # 10 clusters and 87 noise points on this case
    src, tgt = torch.from_numpy(c["src"]).cuda(), torch.from_numpy(c["tgt"]).cuda()
    h = rh.re_ranking_hausdorff_device(src, tgt, k=c["k"], lambda_value=c["lambda_value"])
    oeps, ocnt, otop = ora.eps_rule(c["final_dist"], rho)
    assert cluster.eps_rule(h, rho) == (oeps, ocnt, otop)
    want = ora.dbscan(c["final_dist"], oeps, 4)
    assert want.max() >= 1                                                        # more than one cluster: the labels say something
    assert np.array_equal(cluster.DBSCAN(eps=oeps, min_samples=4, metric="precomputed").fit_predict(h), want)
    e_list, r_list = compute_dist(c["src"], c["tgt"], c["lambda_value"], False, variant="hausdorff")
    assert e_list == [[]] and r_list[0].mode == 2 and np.array_equal(r_list[0].final_dist().cpu().numpy(), c["final_dist"])
    labels, clusters = generate_selflabel(e_list, r_list, 0, types.SimpleNamespace(no_rerank=False, rho=rho), [])
    assert np.array_equal(labels[0], want) and clusters[0].eps == oeps
    # the default variant is today's path, bit for bit; 'plain' gives the kNN-set variant's handle
    base = rerank.re_ranking_device(src, tgt, lambda_value=c["lambda_value"])
    for kw in ({}, {"variant": "kreciprocal"}):
        _, r0 = compute_dist(c["src"], c["tgt"], c["lambda_value"], False, **kw)
        assert r0[0].mode == 0 and torch.equal(r0[0].final_dist(), base.final_dist())
    from ssg_amd.rerank_plain import re_ranking_plain_device
    _, rp = compute_dist(c["src"], c["tgt"], c["lambda_value"], False, variant="plain")
    assert torch.equal(rp[0].final_dist(), re_ranking_plain_device(src, tgt, lambda_value=c["lambda_value"]).final_dist())
