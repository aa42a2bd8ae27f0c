"""CPU suite: what the float32 distance / re_ranking_init GPU tests stand on, checked without a GPU -- the oracle helpers pinned to the
reference's own recorded outputs (tests/golden/pairwise.npz, rerank_init.npz), and the condition on the inputs of the GEMM-fed
re_ranking_init comparison: the reference alone, fed numpy float32 dots or float64 dots rounded to float32, keeps at least 98 % of
its rows within 2e-5 on the very features tests/test_gpu_rerank_init_large.py uses."""
import numpy as np

import rerank_init_ref as rir


def test_sqdist_helpers_vs_reference_golden(golden, ora):
    """oracle.ssg_oracle.sqdist_f64 / sqdist_f32_reference against reid/evaluators.py:63-85 as recorded (unit-norm 200-d and un-normalised 2048-d
    features): the float32 restatement to a few ulps of the largest distance (BLAS summation order), the float64 one to float32 accuracy"""
    g = golden("pairwise.npz")
    for tag in ("u", "r"):
        F = g["feats_" + tag]; nq, g0 = int(g["nq_" + tag]), int(g["g0_" + tag])
        scale = max(1.0, float(np.abs(g["self_" + tag]).max()))
        for form, x, y, want in ((0, F[:nq], F[g0:], g["qg_" + tag]), (1, F, F, g["self_" + tag])):
            r32 = ora.sqdist_f32_reference(x, y, form); r64 = ora.sqdist_f64(x, y, form)
            assert r32.dtype == np.float32 and r64.dtype == np.float64 and r32.shape == r64.shape == want.shape
            assert np.abs(r32 - want).max() <= 8 * 2.0 ** -24 * scale, (tag, form)
            assert np.abs(r64 - want).max() <= 2e-5 * scale, (tag, form)
    x = F[:5]; rows = np.array([0, 3]); cols = np.array([4, 1, 1])
    assert np.array_equal(ora.sqdist_f64(F, F, 0, rows, cols), ora.sqdist_f64(F[rows], F[cols], 0))
    assert np.allclose(ora.sqdist_f64(x, x, 2), 2 - 2 * x.astype(np.float64) @ x.astype(np.float64).T, rtol=0, atol=1e-12)
    assert np.abs(ora.sqdist_f32_reference(x, x, 2) - ora.sqdist_f64(x, x, 2)).max() < 1e-3


def test_re_ranking_init_stages_vs_reference_golden(golden, ora):
    """oracle.ssg_oracle.re_ranking_init_stages: the final block is the one of re_ranking_init (bit for bit) and within 5e-6 of the reference's
    recorded output; rowmax / rank / v_nnz are the stage values of rerank.py:183-204 restated in numpy"""
    g = golden("rerank_init.npz")
    for tag in ("a", "b"):
        q, gal = g["q_" + tag], g["g_" + tag]
        k1, k2, lam = int(g["k1_" + tag]), int(g["k2_" + tag]), float(g["lam_" + tag])
        nq, N = q.shape[0], q.shape[0] + gal.shape[0]
        stacked = ora.stacked_dots(np.dot(q, gal.T), np.dot(q, q.T), np.dot(gal, gal.T))
        out, st = ora.re_ranking_init_stages(stacked, nq, k1=k1, k2=k2, lambda_value=lam)
        assert np.array_equal(out, ora.re_ranking_init(q, gal, k1=k1, k2=k2, lambda_value=lam))
        assert np.abs(out - g["final_" + tag]).max() < 5e-6
        od = 2. - 2 * stacked
        assert np.array_equal(st["rowmax"], np.max(od, axis=0))
        dn = np.transpose(1. * od / np.max(od, axis=0))
        K = min(k1 + 1, N)
        order = np.argsort(dn, axis=1, kind="stable")
        head = np.take_along_axis(dn, order[:, :K + 1], axis=1)
        tie_free = (np.diff(head, axis=1) != 0).all(1)
        assert tie_free.mean() > 0.9
        assert np.array_equal(st["rank"][tie_free], order[tie_free, :K])
        part = np.argpartition(dn, range(1, k1 + 1))[:, :K]          # the reference's own call (rerank.py:187)
        assert np.array_equal(st["rank"][tie_free], part[tie_free])
        assert st["v_nnz"].min() >= 1 and st["v_nnz"].max() <= (k1 + 1) * (int(np.around(k1 / 2)) + 2)


def test_reference_alone_keeps_98_percent_of_the_rows(ora):
    """the condition test_gemm_fed_form_at_size puts on its inputs: on the same features, the oracle on numpy's float32 dots and the oracle on
    float64 dots rounded to float32 (two Gram matrices that differ in their last bits, like numpy's and the GPU's) agree within 2e-5 on at
    least 98 % of the rows.  (Measured: 1 row of 12 185, 0 of 1472.)"""
    for nq, ng, d, seed in rir.GEMM_CASES:
        x = rir.features(nq, ng, d, seed)
        a = ora.re_ranking_init(x[:nq], x[nq:], k1=20, k2=6, lambda_value=0.3)
        x64 = x.astype(np.float64)
        b, _ = ora.re_ranking_init_stages((x64 @ x64.T).astype(np.float32), nq, k1=20, k2=6, lambda_value=0.3)
        ok = (np.abs(a.astype(np.float64) - b) <= rir.ROW_TOL).all(1)
        print("reference alone: %d + %d, d %d: %d of %d rows beyond 2e-5" % (nq, ng, d, int((~ok).sum()), nq))
        assert ok.mean() >= rir.ROW_FRACTION, (nq, ng, int((~ok).sum()))
