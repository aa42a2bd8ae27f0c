"""GPU suite (-m gpu): the float32 k-reciprocal chain of re_ranking_init (csrc/rerank_init.hip: `ssg_affine_2m2x_f32`, `ssg_rerank_init_stage1`,
`ssg_rerank_init_expand`, `ssg_rerank_init_jaccard`) at the sizes the SSG++ label step runs it at, against the C restatement of
reid/rerank.py:171-234 (oracle/ssg_oracle.c).

(a) identical input: the three dot-product matrices are computed once (numpy float32 on the CPU) and handed to both sides, which both form
    2 - 2 * dots in float32 -- the ranking decides on identical values, so EVERY element must be within 2e-5 (what is left is expf and the
    order of a few float32 sums).  1500 + 4500 and the Market size 12 185 + 751 (the C oracle takes about 15 s for it on 8 threads, so
    the full size is used), duplicated rows (exact ties in D), k2 = 1, k1 = 5 (np.around(2.5) == 2).  The chain is run twice: through
    ssg_amd.re_ranking_init_dist, and entry point by entry point with the stage outputs compared on the way -- same bits.
(b) the stages by name: 2 - 2 * a bit for bit (NaN, inf included); rowmax == D.max(1) bit for bit; rank == the stable argsort of D / rowmax
    on every row without an exact tie among its first k1 + 2 values (and == the oracle's (value, column) order on every row); every
    v_nnz <= ssg_krecip_row_capacity(k1) and == the oracle's.
(c) the GEMM-fed form ssg_amd.re_ranking_init(q, g) against oracle.re_ranking_init(q, g) at 12 185 + 751 and at N = 5952 = 64 * 93, d = 2048:
    the two Gram matrices differ in their last bits, so a near-tie in the ranking may go either way -- at least 98 % of the rows entirely
    within 2e-5 (the rule of test_rerank_chain_vs_reference).  The 98 % is a condition on the inputs: tests/test_dist_f32_host.py checks that
    the reference alone (numpy float32 dots against float64 dots rounded to float32) stays inside it on the same features.
Every case prints one `rerank-init-diff` line (pytest -s); profiles/dist_f32_errors.txt holds them.
"""
import numpy as np
import pytest

import rerank_init_ref as rir

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    from ssg_amd import _lib
    return _lib.lib()


def _chain(L, D, nq, k1, k2, lam):
    """the sparse stages on a device float32 D [N, N], entry point by entry point (the calls of ssg_amd.rerank._init_pipeline)
    -> (out [nq, N - nq], rowmax, rank, v_nnz)"""
    from ssg_amd._lib import check, ptr, stream
    dev, st = D.device, stream()
    N = D.shape[0]
    K = min(k1 + 1, N)
    capV = int(L.ssg_krecip_row_capacity(k1))
    rowmax = torch.full((N,), float("nan"), dtype=torch.float32, device=dev)
    rank = torch.full((N, K), -1, dtype=torch.int32, device=dev)
    v_idx = torch.full((N, capV), -1, dtype=torch.int32, device=dev); v_val = torch.full((N, capV), float("nan"), dtype=torch.float32, device=dev)
    v_nnz = torch.full((N,), -1, dtype=torch.int32, device=dev)
    check(L.ssg_rerank_init_stage1(ptr(D), N, k1, k2, capV, ptr(rowmax), ptr(rank), ptr(v_idx), ptr(v_val), ptr(v_nnz), st), "ssg_rerank_init_stage1")
    assert int(v_nnz.min()) >= 1 and int(v_nnz.max()) <= capV
    if k2 != 1:
        kk = min(k2, N, K)
        mx = int(v_nnz.max().item())
        capQ = kk * mx
        q_idx = torch.full((N, capQ), -1, dtype=torch.int32, device=dev); q_val = torch.full((N, capQ), float("nan"), dtype=torch.float32, device=dev)
        q_nnz = torch.full((N,), -1, dtype=torch.int32, device=dev)
        check(L.ssg_rerank_init_expand(ptr(v_idx), ptr(v_val), ptr(v_nnz), ptr(rank), N, k1, k2, capV, capQ, mx, ptr(q_idx), ptr(q_val), ptr(q_nnz), st),
              "ssg_rerank_init_expand")
        assert int(q_nnz.min()) >= 1 and int(q_nnz.max()) <= capQ
    else:
        capQ, q_idx, q_val, q_nnz = capV, v_idx, v_val, v_nnz
    total = int(q_nnz.sum().item())
    colcnt = torch.empty(N, dtype=torch.int32, device=dev); colptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
    inv_row = torch.empty(total, dtype=torch.int32, device=dev); inv_val = torch.empty(total, dtype=torch.float32, device=dev)
    out = torch.full((nq, N - nq), float("nan"), dtype=torch.float32, device=dev)
    check(L.ssg_rerank_init_jaccard(ptr(D), ptr(rowmax), ptr(q_idx), ptr(q_val), ptr(q_nnz), capQ, N, nq, float(lam), ptr(colcnt), ptr(colptr),
                                    ptr(inv_row), ptr(inv_val), ptr(out), st), "ssg_rerank_init_jaccard")
    torch.cuda.synchronize()
    return out, rowmax, rank, v_nnz


def _affine(L, a):
    from ssg_amd._lib import check, ptr, stream
    out = torch.full_like(a, float("nan"))
    check(L.ssg_affine_2m2x_f32(ptr(a), ptr(out), a.numel(), stream()), "ssg_affine_2m2x_f32")
    return out


def _same_bits_nan(a, b):
    """bit equality of two float32 numpy arrays, any NaN equal to any NaN"""
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


CASES = [  # tag, nq, ng, seed, duplicates, k1, k2, lambda, stages against numpy
    ("1500+4500", 1500, 4500, 11, False, 20, 6, 0.3, True),
    ("1500+4500 duplicated rows", 1500, 4500, 12, True, 20, 6, 0.3, True),
    ("1500+4500 k2=1", 1500, 4500, 11, False, 20, 1, 0.3, False),
    ("1500+4500 k1=5", 1500, 4500, 11, False, 5, 3, 0.5, True),
    ("market 12185+751", 12185, 751, 13, False, 20, 6, 0.3, False),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0].replace(" ", "-") for c in CASES])
def test_identical_input_every_element(L, dev, ora, case):
    """(a) and (b): see the module docstring"""
    import ssg_amd
    tag, nq, ng, seed, dup, k1, k2, lam, numpy_stages = case
    N = nq + ng
    x = rir.features(nq, ng, 256, seed, duplicates=dup)
    qg, qq, gg = rir.dots(x, nq)
    stacked = ora.stacked_dots(qg, qq, gg)
    assert np.array_equal(stacked, stacked.T)                   # np.dot(a, a.T) is symmetric bit for bit (syrk): row max == column max
    ref, st = ora.re_ranking_init_stages(stacked, nq, k1=k1, k2=k2, lambda_value=lam)
    got = ssg_amd.re_ranking_init_dist(qg, qq, gg, k1=k1, k2=k2, lambda_value=lam)
    assert got.shape == ref.shape == (nq, ng) and got.dtype == np.float32 and np.isfinite(got).all()
    diff = np.abs(got.astype(np.float64) - ref)
    bad_rows = int((diff > rir.ROW_TOL).any(1).sum())
    print("rerank-init-diff: %-28s identical dots   N %6d nq %6d k1 %2d k2 %d  max|diff| %.3e  rows beyond 2e-5: %d of %d"
          % (tag, N, nq, k1, k2, float(diff.max()), bad_rows, nq))
    # the same chain, entry point by entry point
    D_host = 2 - 2 * stacked                                    # float32 (rerank_initial.py:50)
    assert D_host.dtype == np.float32
    D = _affine(L, torch.from_numpy(stacked).to(dev))
    assert _same_bits_nan(D.cpu().numpy(), D_host), "ssg_affine_2m2x_f32 differs from numpy's 2 - 2 * a"
    out, rowmax, rank, v_nnz = _chain(L, D, nq, k1, k2, lam)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), got.view(np.uint32)), "the wrapper and the entry points called by name differ"
    assert np.array_equal(rowmax.cpu().numpy().view(np.uint32), D_host.max(1).view(np.uint32))
    assert np.array_equal(rowmax.cpu().numpy().view(np.uint32), st["rowmax"].view(np.uint32))
    rank = rank.cpu().numpy(); v_nnz = v_nnz.cpu().numpy()
    assert v_nnz.max() <= L.ssg_krecip_row_capacity(k1)
    assert np.array_equal(rank, st["rank"]), "top-(k1+1) order differs from the oracle's (value, column) order on %d rows" % int((rank != st["rank"]).any(1).sum())
    assert np.array_equal(v_nnz, st["v_nnz"])
    if numpy_stages:
        Dn = D_host / D_host.max(1)[:, None]
        order = np.argsort(Dn, axis=1, kind="stable")[:, :k1 + 2]
        head = np.take_along_axis(Dn, order, axis=1)
        tie_free = (np.diff(head, axis=1) != 0).all(1)
        assert tie_free.sum() >= (N // 2 if dup else N * 0.99) and (~tie_free).sum() >= (100 if dup else 0), tie_free.sum()     # (measured: 2470 tied rows / 2 / 0)
        assert np.array_equal(rank[tie_free], order[tie_free, :k1 + 1].astype(np.int32))
    assert diff.max() <= rir.ROW_TOL, (tag, float(diff.max()), bad_rows)


def test_affine_2m2x_special_values(L, dev):
    """`ssg_affine_2m2x_f32` == numpy's float32 2 - 2 * a bit for bit: two roundings, no FMA; NaN, +-inf, +-0, denormals, a length that wraps the grid"""
    g = np.random.default_rng(5)
    a = (g.standard_normal(2048 * 256 * 3 + 17) * 10.0 ** g.integers(-12, 12, 2048 * 256 * 3 + 17)).astype(np.float32)
    a[:14] = [np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 1e-45, 1.7e38, 3.4e38, -3.4e38, 2.0 ** -126]
    a[5000::4999] = np.resize(a[:14], a[5000::4999].shape)
    with np.errstate(all="ignore"):
        ref = 2 - 2 * a
    assert ref.dtype == np.float32
    got = _affine(L, torch.from_numpy(a).to(dev)).cpu().numpy()
    assert _same_bits_nan(got, ref), np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))[:8]


@pytest.mark.parametrize("case", rir.GEMM_CASES, ids=["%d+%d" % c[:2] for c in rir.GEMM_CASES])
def test_gemm_fed_form_at_size(dev, ora, case):
    """(c): ssg_cosine_dist_f32 -> the chain, against numpy's dots -> the oracle; at least 98 % of the rows entirely within 2e-5"""
    import ssg_amd
    nq, ng, d, seed = case
    x = rir.features(nq, ng, d, seed)
    got = ssg_amd.re_ranking_init(x[:nq], x[nq:], k1=20, k2=6, lambda_value=0.3)
    ref = ora.re_ranking_init(x[:nq], x[nq:], k1=20, k2=6, lambda_value=0.3)
    assert got.shape == ref.shape == (nq, ng) and got.dtype == np.float32 and np.isfinite(got).all()
    diff = np.abs(got.astype(np.float64) - ref)
    ok = (diff <= rir.ROW_TOL).all(1)
    print("rerank-init-diff: %-28s GEMM-fed d %4d    N %6d nq %6d k1 20 k2 6  max|diff| %.3e  rows beyond 2e-5: %d of %d (%.4f %%)  max|diff| on the other rows %.3e"
          % ("%d+%d" % (nq, ng), d, nq + ng, nq, float(diff.max()), int((~ok).sum()), nq, 100.0 * float((~ok).mean()), float(diff[ok].max())))
    assert ok.mean() >= rir.ROW_FRACTION, (int((~ok).sum()), nq)
