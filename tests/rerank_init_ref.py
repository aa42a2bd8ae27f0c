"""Inputs shared by tests/test_gpu_rerank_init_large.py and its host twin tests/test_dist_f32_host.py: the clustered unit-norm features
(tools/synth.py) of the float32 re-ranking tests, at the sizes of the SSG++ label step."""
import numpy as np

from conftest import clustered

# (nq, ng, d, seed) of the GEMM-fed comparison: the SSG++ Market size 12 185 + 751 (N = 12 936, padded to 12 992) and an N = 5952 = 64 * 93
# that needs neither padding nor the .contiguous() copy
GEMM_CASES = ((12185, 751, 2048, 21), (1472, 4480, 2048, 22))
ROW_TOL = 2e-5          # the project's bound for this float32 variant (test_re_ranking_init_vs_reference_golden)
ROW_FRACTION = 0.98     # rows that must lie entirely within ROW_TOL when the two Gram matrices differ in their last bits


def features(nq, ng, d, seed, duplicates=False):
    x = clustered(nq + ng, d, seed)
    if duplicates:          # exact ties in D: query rows repeated in the gallery, gallery rows repeated in the gallery and among the queries
        x[nq + 100:nq + 160] = x[10:70]
        x[nq + 900:nq + 940] = x[nq + 300:nq + 340]
        x[200:220] = x[nq + 2000:nq + 2020]
    return x


def dots(x, nq):
    """the three float32 dot-product matrices of rerank.py:174-176 (numpy, computed once and handed to both sides)"""
    q, g = x[:nq], x[nq:]
    return np.dot(q, g.T), np.dot(q, q.T), np.dot(g, g.T)
