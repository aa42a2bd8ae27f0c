"""Case table of the re-ranking parameter grid: tools/make_golden.py (kgrid_fixture -> tests/golden/rerank_kgrid.npz),
tests/test_rerank_grid_host.py and tests/test_gpu_rerank_grid.py all import it.

`re_ranking_device` accepts 1 <= k1 <= 63, 1 <= k2 <= 64, any lambda and N >= 2.  Inside that range the k-reciprocal kernels
(csrc/krecip.hip, csrc/jaccard.hip) change their control flow with the parameters; `derived` restates the host-side arithmetic that
decides it, and every case names what it is there to reach (`why`) and the properties it must have on its input (`claims`, checked by
the generator and again by the host test from the oracle's stages).

The fixture holds what the UNTOUCHED reference (reid/rerank.py re_ranking, selftraining.py's eps rule, sklearn's DBSCAN) gave on these
inputs; the inputs themselves are regenerated from their seeds (their sha256 is stored)."""
import hashlib
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from synth import clustered  # noqa: E402

FIXTURE = "rerank_kgrid.npz"
RHOS = (2e-2, 0.2)                           # the eps rule's rho: the script default's order of magnitude and a wide one
FULL_N = 100                                 # final_dist is stored as float64 up to this N; above it only its sha256
STAGES = ("euclid", "V", "V_qe", "jaccard", "final")
QE_LDS_LIMIT = 160 * 1024                    # bytes of LDS one workgroup of the query expansion may ask for
QE_FIRST_GUESS = 64                          # rerank.re_ranking_device's first guess of the longest V row

Case = namedtuple("Case", "name N Ns d gen seed k1 k2 lam why claims")


def _build_table():
    cases = []

    def add(N, k1, k2, lam, why, gen="clustered", d=32, seed=None, **claims):
        n = len(cases) + 1
        name = "c%02d_n%d_k%d_%d_l%s" % (n, N, k1, k2, ("%g" % lam).replace(".", "p"))
        cases.append(Case(name, N, 64, d, gen, 100 + n if seed is None else seed, k1, k2, lam, why, claims))

    def weak(N, k1, k2, lam, why, **claims):
        add(N, k1, k2, lam, why, gen="weak", d=12 if N == 320 else 8, seed=5, **claims)

    add(96, 20, 1, 0.3, "k2 == 1 on the main path: V feeds the inverted index, capQ = capV")
    add(96, 1, 1, 0.3, "`holds`, not `holds4`; kh = 1; sums of fewer than 8 weights", holds4=False, kh=1)
    add(96, 1, 2, 0.3, "the same with K widened by k2", holds4=False, kh=1, K=2)
    add(96, 2, 2, 0.3, "kh = 2, K = 3", holds4=False, kh=2, K=3)
    add(96, 3, 2, 0.3, "the first k1 on `holds4` (kh = 3, K = 4)", holds4=True, kh=3, K=4)
    add(96, 5, 3, 0.3, "round(2.5) = 2", kh=3)
    add(96, 7, 4, 0.3, "round(3.5) = 4", kh=5)
    add(160, 33, 7, 0.3, "kh = 17: a second trip of the 16-entry loops", kh=17)
    weak(320, 41, 11, 0.2, "longest V row > 64: the first guess misses, the tail is redone by the reported length", vmax_gt=64)
    weak(320, 63, 1, 0.2, "K1 = 64 (every lane live); longest V row > 128 (recursive pairwise sum)", K1=64, vmax_gt=128)
    weak(256, 33, 2, 0.5, "longest V row on / next to the first guess of 64", vmax_in=(63, 64, 65))
    weak(200, 17, 33, 0.5, "k2 > k1 + 1 with 33 lists", kk=33, K=33)
    weak(320, 63, 31, 0.2, "the largest k2 that fitted four waves of LDS after the redo", K1=64, kk=31, vmax_gt=64)
    weak(320, 63, 64, 0.2, "the corner of the accepted range", K1=64, kk=64, vmax_gt=64)
    add(65, 63, 64, 0.3, "N = 65, K = K1 = kk = 64: all rows but one are every row's neighbours", K=64, K1=64, kk=64)
    add(21, 20, 6, 0.3, "N = k1 + 1", K=21, K1=21)
    add(12, 20, 6, 0.3, "N < k1 + 1: K, K1 and kh all clamped by N", K=12, K1=12, kh=11)
    add(5, 4, 9, 0.3, "N < k2", K=5, kk=5)
    add(2, 20, 6, 0.3, "the smallest N the entry accepts", K=2, K1=2, kh=2, kk=2, holds4=False)
    add(96, 20, 6, 0.0, "J' = the Jaccard distance: exact zeros in final_dist that the eps rule's nonzero() drops", zero_pairs=True)
    add(96, 20, 6, 1.0, "J' == 0 everywhere, the sparse copy's constant is 0", jp_all_zero=True)
    add(96, 20, 6, 1.5, "negative J': first-generation Jaccard kernel, no sparse copy", jp_negative=True)
    return tuple(cases)


CASES = _build_table()
BY_NAME = {c.name: c for c in CASES}


def inputs(case):
    """(src, tgt) float32.  clustered: unit-norm identity centres + noise, 8 rows per identity; weak: unit-norm Gaussian rows (no
    identities: long, ragged k-reciprocal sets)."""
    if case.gen == "clustered":
        return clustered(case.Ns, case.d, case.seed + 1000, per_id=8, intra=0.6), clustered(case.N, case.d, case.seed, per_id=8)
    rng = np.random.default_rng(case.seed)
    tgt = rng.standard_normal((case.N, case.d)); tgt /= np.linalg.norm(tgt, axis=1, keepdims=True)
    src = rng.standard_normal((case.Ns, case.d)); src /= np.linalg.norm(src, axis=1, keepdims=True)
    return src.astype(np.float32), tgt.astype(np.float32)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def round_half_even_div2(k1):
    """int(np.around(k1 / 2)) in integers"""
    return k1 // 2 if k1 % 2 == 0 or (k1 // 2) % 2 == 0 else k1 // 2 + 1


def qe_list_bytes(capL):
    """LDS of one staged V row of the query expansion: columns, head prefix (one more entry), half values padded to 4 bytes"""
    return 4 * capL + 4 * (capL + 1) + ((2 * capL + 3) & ~3)


def qe_wave_bytes(kk, capL):
    """LDS of one wave (= one row) of the query expansion: kk staged lists + their kk lengths (64 bytes up to 16 lists, else 256)"""
    return (kk * qe_list_bytes(capL) + (64 if kk <= 16 else 256) + 15) & ~15


def qe_waves(kk, capL):
    """rows per workgroup the host entry picks: the largest of 4, 2, 1 that fits; 0 = does not fit at all"""
    for w in (4, 2, 1):
        if w * qe_wave_bytes(kk, capL) <= QE_LDS_LIMIT:
            return w
    return 0


def derived(case):
    """the host-side numbers that pick the kernels' paths (the host entries of csrc/krecip.hip, rerank.re_ranking_device)"""
    N, k1, k2 = case.N, case.k1, case.k2
    K = min(max(k1 + 1, k2), N)                              # rank columns kept
    K1 = min(k1 + 1, N, K)                                   # forward neighbours of a row
    kh = min(round_half_even_div2(k1) + 1, N, K)             # neighbours of a candidate in the 1/2-k expansion
    return dict(K=K, K1=K1, kh=kh, holds4=((kh + 3) & ~3) <= K, kk=None if k2 == 1 else min(k2, N, K),
                capV=(k1 + 1) * (round_half_even_div2(k1) + 2),
                om_bits=int(np.float16(1.0 - case.lam).view(np.uint16)))


_ORACLE_RUNS = {}


def oracle_run(ora, case):
    """(src, tgt, euclid, final, stages) of the C oracle on a case, computed once per process and shared (do not write to the arrays).
    tools/make_golden.py has checked the oracle against the reference on these very inputs, stage by stage."""
    if case.name not in _ORACLE_RUNS:
        src, tgt = inputs(case)
        oe, of, st = ora.re_ranking(src, tgt, k1=case.k1, k2=case.k2, lambda_value=case.lam, rank_mode="introsort", stages=True)
        _ORACLE_RUNS[case.name] = (src, tgt, oe, of, st)
    return _ORACLE_RUNS[case.name]


def check_stage(g, case, stage, got, ref):
    """`got` (half bits / float64) against the fixture: the stored array where there is one, the sha256 otherwise -- a mismatch is
    located with `ref`, the oracle's array of the same stage"""
    p = case.name + "__"
    if p + stage in g.files:                   # (final_dist, float64, up to N = FULL_N)
        assert np.array_equal(got, g[p + stage]), "%s %s vs the reference's array: %s" % (case.name, stage, first_difference(got, g[p + stage]))
    assert sha(got) == str(g[p + "sha_" + stage]), "%s %s vs the reference's sha256; against the oracle: %s" % (
        case.name, stage, first_difference(_bits(got), _bits(ref)))


def check_eps_and_labels(g, case, eps_rule, dbscan, what=""):
    """eps_rule(rho) -> (eps, count, top_num) and dbscan(eps) -> labels against the reference's at both rho.  Where the reference's
    top_num is 0 (fewer than 1 / (2 rho) pairs) its eps is the mean of an empty slice, NaN, which sklearn refuses: count and top_num
    are compared, eps must be NaN, and there are no labels."""
    p = case.name + "__"
    for r, rho in enumerate(RHOS):
        eps, cnt, top = eps_rule(rho)
        want = (float(g[p + "eps%d" % r]), int(g[p + "count%d" % r]), int(g[p + "top%d" % r]))
        if want[2] == 0:
            assert np.isnan(want[0]) and np.isnan(eps) and (cnt, top) == want[1:], (case.name, what, rho, (eps, cnt, top), want)
            assert p + "labels%d" % r not in g.files
            continue
        assert (eps, cnt, top) == want, (case.name, what, rho, (eps, cnt, top), want)
        labels = dbscan(eps)
        assert np.array_equal(labels, g[p + "labels%d" % r]), (case.name, what, rho, "DBSCAN labels (incl. numbering)")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.dtype == np.float16 else a


def check_claims(case, st, final):
    """assert the properties `case.claims` lists, from the stage arrays of a run (reference or oracle): st['V'] dense half [N, N],
    st['jaccard'] half [N, N]; final float64 [N, N]"""
    dv = derived(case)
    vmax = int((np.asarray(st["V"]) != 0).sum(axis=1).max())
    for k, want in case.claims.items():
        if k in dv:
            assert dv[k] == want, (case.name, k, dv[k], want)
        elif k == "vmax_gt":
            assert vmax > want, (case.name, "longest V row", vmax, "not >", want)
        elif k == "vmax_in":
            assert vmax in want, (case.name, "longest V row", vmax, "not in", want)
        elif k == "zero_pairs":
            nz = int(np.count_nonzero(np.triu(final, 1)))
            assert nz < case.N * (case.N - 1) // 2, (case.name, "no exact zero above the diagonal")
        elif k == "jp_all_zero":
            assert case.lam == 1.0 and dv["om_bits"] == 0
        elif k == "jp_negative":
            jp = np.asarray(st["jaccard"]).astype(np.float64) * (1.0 - case.lam)
            assert dv["om_bits"] & 0x8000 and (jp < 0).any(), (case.name, "no negative J'")
        else:
            raise KeyError(k)
    return vmax


def sparse_to_dense(idx, val, nnz, N):
    """sparse rows (device tensors: columns int32 [n, cap], half values [n, cap], lengths [n]) -> dense uint16 [n, N] of half bits"""
    idx = idx.cpu().numpy(); val = val.cpu().numpy().view(np.uint16); nnz = nnz.cpu().numpy()
    out = np.zeros((idx.shape[0], N), np.uint16)
    for i in range(idx.shape[0]):
        n = int(nnz[i])
        assert np.all(np.diff(idx[i, :n]) > 0), "sparse row %d not sorted by column" % i
        out[i, idx[i, :n]] = val[i, :n]
    return out


def first_difference(a, b):
    """where two arrays of one shape first differ, for the message of a failed hash comparison"""
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    if a.dtype == np.float16:
        a = a.view(np.uint16); b = b.view(np.uint16)
    if a.shape != b.shape:
        return "shapes %r / %r" % (a.shape, b.shape)
    bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
    return "equal" if len(bad) == 0 else "%d differ, first at %r: %r / %r" % (len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])
