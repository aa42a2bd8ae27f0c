"""CPU checks of the retrieval-metric references: the exact, definitional tests/rank_ref.py against what the reference itself
returned (tests/golden/eval_cases.npz) and against the argsort-based restatement oracle/eval_oracle.py on the whole grid that
tests/test_gpu_rank_metrics.py runs on the device, so the device tests rest on two independent statements of the metrics; the grid's
own promises (match counts, ties on both sides of a match); and the id remapping ssg_amd.ranking does before it touches the device.

AP is compared as a rational: |float - exact| <= P * 2^-51 + 2^-52 for a query with P matches (rank_ref.ap_bound), the mean over
queries with the largest P of the case."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_ref as ref  # noqa: E402


def assert_ap_within_bound(got, result, what=""):
    """float APs against the exact ones of a rank_ref result, query by query; NaN exactly where the query is skipped"""
    worst = 0.0
    for q, exact in enumerate(result.ap_exact):
        if exact is None:
            assert np.isnan(got[q]), (what, q)
            continue
        err = abs(Fraction(float(got[q])) - exact)
        assert err <= Fraction(ref.ap_bound(int(result.nmatch[q]))), (what, q, float(err), int(result.nmatch[q]))
        worst = max(worst, float(err))
    return worst


@pytest.mark.parametrize("tag", "abc")
def test_rank_ref_vs_reference_golden(golden, tag):
    g = golden("eval_cases.npz")
    a = (g["dist_" + tag], g["qid_" + tag], g["gid_" + tag], g["qcam_" + tag], g["gcam_" + tag])
    r = ref.per_query(*a)
    assert np.array_equal(r.first, g["first_" + tag])
    assert np.array_equal(ref.cmc(*a, first_match_break=True, result=r), g["cmc_" + tag])
    assert np.array_equal(ref.cmc(*a, result=r), g["cmc_all_" + tag])
    assert_ap_within_bound(g["ap_" + tag], r, tag)
    exact, pmax = ref.mean_ap_exact(r)
    assert abs(Fraction(float(g["map_" + tag])) - exact) <= Fraction(ref.ap_bound(pmax))


@pytest.mark.parametrize("name", list(ref.GRID))
def test_rank_ref_vs_eval_oracle(name):
    """two independent statements of the metrics on every case of the grid.  AP on the finite cases only: the oracle restates
    sklearn, whose np.diff of two equal infinities is NaN, not 0 (sklearn itself refuses non-finite scores)."""
    from oracle import eval_oracle
    case = ref.GRID[name]()
    a = ref.args(case)
    with np.errstate(over="ignore", invalid="ignore"):       # the oracle's np.diff: FLT_MAX - (-FLT_MAX), inf - inf
        ofirst, oap = eval_oracle.per_query(*a)
    r = ref.per_query(*a)
    assert np.array_equal(r.first, ofirst)
    if case["finite"]:
        assert_ap_within_bound(oap, r, name)
        exact, pmax = ref.mean_ap_exact(r)
        assert abs(Fraction(float(eval_oracle.mean_ap(*a))) - exact) <= Fraction(ref.ap_bound(pmax))
    for sep in (False, True):
        rs = ref.per_query(*a, separate_camera_set=sep)
        for fmb in (False, True):
            for topk in (1, 7, 100):
                try:
                    want = eval_oracle.cmc(*a, topk=topk, separate_camera_set=sep, first_match_break=fmb)
                except RuntimeError:
                    want = None
                if want is None:
                    with pytest.raises(RuntimeError, match="No valid query"):
                        ref.cmc(*a, topk=topk, separate_camera_set=sep, first_match_break=fmb, result=rs)
                else:
                    assert np.array_equal(ref.cmc(*a, topk=topk, separate_camera_set=sep, first_match_break=fmb, result=rs), want), (sep, fmb, topk)


def test_hand_computed():
    """three entries, matches ranked first and third: AP = 1/2 * 1/1 + 1/2 * 2/3; a row of one value is one threshold: AP = P / n"""
    r = ref.per_query(np.array([[0.3, 0.1, 0.2]], np.float32), [1], [1, 1, 2], [0], [1, 1, 1])
    assert r.first[0] == 0 and list(r.bins[0]) == [0, 1] and r.nmatch[0] == 2 and r.ap_exact[0] == Fraction(5, 6)
    r = ref.per_query(np.zeros((1, 5), np.float32), [1], [2, 1, 2, 1, 2], [0], [1] * 5)
    assert r.first[0] == 1 and list(r.bins[0]) == [1, 2] and r.ap_exact[0] == Fraction(2, 5)
    assert np.array_equal(ref.cmc(np.zeros((1, 5), np.float32), [1], [2, 1, 2, 1, 2], [0], [1] * 5, topk=3), [0, .5, 1])
    # the all-shots loop stops at the first bin >= topk, the cumulative curve keeps what was credited before it
    assert np.array_equal(ref.cmc(np.zeros((1, 5), np.float32), [1], [2, 1, 2, 1, 2], [0], [1] * 5, topk=2), [0, .5])
    # -0.0 is 0.0: the match at column 1 is tied with column 0, which the index puts first
    assert ref.per_query(np.array([[0.0, -0.0]], np.float32), [1], [2, 1], [0], [1, 1]).first[0] == 1
    assert ref.ap_bound(ref.RK_CAP) < 1e-12


def test_all_invalid_raises():
    from oracle import eval_oracle
    a = ref.args(ref.validity_case("all_invalid"))
    assert list(ref.per_query(*a).first) == [-1, -1]
    for f in (ref.cmc, eval_oracle.cmc, eval_oracle.mean_ap):
        with pytest.raises(RuntimeError, match="No valid query"):
            f(*a)
    with pytest.raises(RuntimeError, match="No valid query"):
        ref.mean_ap_exact(ref.per_query(*a))


def test_nan_in_the_reference():
    """a NaN in a valid entry of a query with a valid true match has no defined result; in a filtered entry, or in a query that
    is skipped anyway, it is never looked at"""
    case = ref.validity_case("mixed")
    dist, qid, gid, qcam, gcam = ref.args(case)
    base = ref.per_query(*ref.args(case))
    q = 0
    filtered = [j for j in range(len(gid)) if gid[j] == qid[q] and gcam[j] == qcam[q]]
    match = [j for j in range(len(gid)) if gid[j] == qid[q] and gcam[j] != qcam[q]]
    other = [j for j in range(len(gid)) if gid[j] != qid[q]]
    assert filtered and match and other
    d = dist.copy(); d[q, filtered] = np.nan; d[1] = np.nan           # query 1 has no valid true match
    got = ref.per_query(d, qid, gid, qcam, gcam)
    assert np.array_equal(got.first, base.first) and got.ap_exact == base.ap_exact
    for j in (match[0], other[0]):
        d = dist.copy(); d[q, j] = np.nan
        with pytest.raises(ValueError, match="query 0"):
            ref.per_query(d, qid, gid, qcam, gcam)


@pytest.mark.parametrize("kind", ref.TIE_KINDS)
def test_tie_cases_tie_on_both_sides(kind):
    case = ref.tie_case(kind)
    assert ref.tied_both_sides(case, False) and ref.tied_both_sides(case, True)
    assert case["finite"] == bool(np.isfinite(case["dist"]).all())


def test_stride_case_neighbours():
    case = ref.tie_case("stride")
    for q, j in enumerate((256, 290, 317, 343)):
        row = case["dist"][q]
        assert list(np.flatnonzero(row == row[j])) == [j - 256, j - 1, j, j + 1, j + 256]
        assert case["gid"][j] == case["qid"][q] and all(case["gid"][k] != case["qid"][q] for k in (j - 256, j - 1, j + 1, j + 256))
        assert (row < row[j]).sum() > 100 and (row > row[j]).sum() > 100


@pytest.mark.parametrize("P", ref.MATCH_COUNTS + (ref.RK_CAP + 1,))
def test_match_count_cases_have_P_matches(P):
    case = ref.match_count_case(P)
    qid, gid, qcam, gcam = case["qid"], case["gid"], case["qcam"], case["gcam"]
    assert case["dist"].shape == (3, P + 300)
    for sep in (False, True):
        assert int(((gid == qid[0]) & (gcam != qcam[0])).sum()) == P
    assert int(((gid == qid[0]) & (gcam == qcam[0])).sum()) == 12 and int((gid == -1).sum()) == 18
    assert int(((gid == qid[1]) & (gcam != qcam[1])).sum()) == 5 and not (gid == qid[2]).any()


@pytest.mark.parametrize("n", ref.GALLERY_SIZES)
def test_gallery_size_cases(n):
    for m, where, col in ((1, "last", n - 1), (1, "first", 0), (3, "last", n - 1)):
        case = ref.gallery_size_case(n, m, where)
        assert case["dist"].shape == (m, n)
        assert list(np.flatnonzero(case["gid"] == case["qid"][0])) == [col]
        if m == 3 and n > 1:
            assert list(np.flatnonzero(case["gid"] == case["qid"][1])) == [0]


def test_int32_labels():
    """ssg_amd.ranking's id conversion: labels inside int32 pass unchanged; outside, query and gallery are replaced together by dense
    ranks, so two labels are equal afterwards exactly when they were before (a cast merges 5 and 5 + 2^32, 2^31 and -2^31)"""
    from ssg_amd.ranking import _int32_labels
    q, g = _int32_labels([3, -1, 2 ** 31 - 1], np.array([-2 ** 31, 3, 7, -1]))
    assert q.dtype == np.int32 and g.dtype == np.int32
    assert list(q) == [3, -1, 2 ** 31 - 1] and list(g) == [-2 ** 31, 3, 7, -1]
    rng = np.random.default_rng(3)
    names = np.array([5, 5 + 2 ** 32, 5 - 2 ** 32, 2 ** 31, -2 ** 31, -1, 2 ** 32 - 1, 2 ** 62, -2 ** 31 - 1, 0], np.int64)
    for _ in range(4):
        qi, gi = names[rng.integers(0, names.size, 9)], names[rng.integers(0, names.size, 40)]
        q, g = _int32_labels(qi, gi)
        assert q.dtype == np.int32 and g.dtype == np.int32 and q.shape == qi.shape and g.shape == gi.shape
        assert np.array_equal(q[:, None] == g[None, :], qi[:, None] == gi[None, :])
        assert np.array_equal(q[:, None] < g[None, :], qi[:, None] < gi[None, :])          # ranks: the order survives too
    q, g = _int32_labels(np.zeros(0), [2 ** 40, 2 ** 40 + 2 ** 32])
    assert q.size == 0 and g[0] != g[1]
    q, g = _int32_labels(np.zeros(3), np.ones(2))                      # the default cameras arrive as float arrays
    assert list(q) == [0, 0, 0] and list(g) == [1, 1]


def test_single_gallery_shot_ids_do_not_wrap():
    """the host half of the single-gallery-shot protocol converts its ids the same way: 5 and 5 + 2^32 stay two gallery identities,
    and the query with the larger one is not taken for the smaller"""
    from ssg_amd.ranking import _sgs_host_checks
    gid = np.array([5, 5 + 2 ** 32, 5, 9, 5 + 2 ** 32], np.int64)
    m, n, qid, gid32, qcam, gcam, gden, qden, G, sizes = _sgs_host_checks(np.zeros((3, 5), np.float32), [5 + 2 ** 32, 5, 7], gid, [0, 0, 0], [1] * 5)
    assert G == 3 and list(sizes) == [2, 1, 2] and list(gden) == [0, 2, 0, 1, 2] and list(qden) == [2, 0, -1]
    assert qid.dtype == np.int32 and gid32.dtype == np.int32
