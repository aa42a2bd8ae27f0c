"""The retrieval-metric kernel (csrc/ranking.hip through ssg_amd.ranking: per_query, per_query_all, cmc, mean_ap, and the raw
ssg_rank_metrics_all entry point) over the whole range it accepts, against the exact reference tests/rank_ref.py -- which
tests/test_rank_ref_host.py holds against oracle/eval_oracle.py and the reference's own recorded outputs on the same grid.

Covered: the match count P of one query up to the cap of 2048 (the rank sort and the bin loops take a second trip past 256; 2048
uses the last LDS slot and bin) and the refusal at 2049; gallery sizes around the 256-thread stride; a row pitch with poisoned
padding; ties of a match with non-matches at lower and higher indices (one value, three values, across the stride, +-0, +-inf,
denormals, FLT_MAX); queries without a valid true match, the junk pid -1, ids at the int32 edges and beyond them, the default ids and
cameras, separate_camera_set; nm_cap below the match count; topk edges; NaN distances; run-to-run bits; the input dtype.

Integers (first rank, match count, all-shots bins) and the CMC curves must be equal; an AP is compared as a rational with the exact
one: |AP - exact| <= P * 2^-51 + 2^-52 (rank_ref.ap_bound), the mean over queries with the largest P of the case.  Every comparison
prints a `rank-ap-error` line (pytest -s); profiles/rank_metrics_errors.txt is the largest per family of such a log."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = -123456789
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda", 0)


_REF = {}


def reference(name, case, sep):
    """rank_ref.per_query of a grid case, computed once per module run and left unchanged"""
    key = (name, sep)
    if key not in _REF:
        _REF[key] = ref.per_query(*ref.args(case), separate_camera_set=sep)
    return _REF[key]


def check_ap(ap, r, family, what):
    """device APs against the exact ones, query by query -> the largest deviation; NaN exactly where the query is skipped"""
    ap = np.asarray(ap)
    worst, worst_bound = -1.0, 0.0
    for q, exact in enumerate(r.ap_exact):
        if exact is None:
            assert np.isnan(ap[q]), (what, q, ap[q])
            continue
        err, bound = float(abs(Fraction(float(ap[q])) - exact)), ref.ap_bound(int(r.nmatch[q]))
        if err > worst:
            worst, worst_bound = err, bound
        assert err <= bound, "%s query %d: |AP - exact| %.3e above the bound %.3e (P = %d)" % (what, q, err, bound, int(r.nmatch[q]))
    print("rank-ap-error family=%s case=%s: largest |AP - exact| %.3e, held to %.3e" % (family, what, max(worst, 0.0), worst_bound))
    return worst


def check_against_reference(ranking, dist, case, name, rs, topks=(100,)):
    """every Python entry point on `dist` (the case's block in whatever layout / dtype the test chose) against rank_ref;
    rs = {sep: reference result}"""
    _, qid, gid, qcam, gcam = ref.args(case)
    ids = (qid, gid, qcam, gcam)
    for sep in (False, True):
        r = rs[sep]
        first, ap = ranking.per_query(dist, *ids, separate_camera_set=sep)
        assert first.dtype == torch.int32 and ap.dtype == torch.float64
        assert np.array_equal(first.cpu().numpy(), r.first), (name, sep)
        check_ap(ap.cpu().numpy(), r, case["family"], "%s sep=%d" % (name, sep))
        nm, nmb = ranking.per_query_all(dist, *ids, separate_camera_set=sep)
        assert np.array_equal(nm, r.nmatch), (name, sep)
        for q in range(len(nm)):
            assert np.array_equal(nmb[q, :nm[q]], r.bins[q]), (name, sep, q)
            assert not nmb[q, nm[q]:].any(), (name, sep, q)                  # the rest of the row is as the wrapper zeroed it
        for topk in topks:
            for fmb in (False, True):
                want = ref.cmc(*ref.args(case), topk=topk, separate_camera_set=sep, first_match_break=fmb, result=r)
                got = ranking.cmc(dist, *ids, topk=topk, separate_camera_set=sep, first_match_break=fmb)
                assert got.shape == (topk,) and np.array_equal(got, want), (name, sep, topk, fmb)
    exact, pmax = ref.mean_ap_exact(rs[False])
    err = float(abs(Fraction(float(ranking.mean_ap(dist, *ids))) - exact))
    assert err <= ref.ap_bound(pmax), "%s: |mAP - exact| %.3e above %.3e" % (name, err, ref.ap_bound(pmax))


def run_grid_case(name):
    from ssg_amd import ranking
    case = ref.GRID[name]()
    rs = {sep: reference(name, case, sep) for sep in (False, True)}
    check_against_reference(ranking, case["dist"], case, name, rs)
    return case, rs


# ------------------------------------------------------------------ match-count edges
@pytest.mark.parametrize("P", ref.MATCH_COUNTS)
def test_match_count(dev, P):
    """one query with exactly P valid true matches, junk around them: P > 256 takes the second trip of the rank sort, 2048 the
    last LDS slot and the last bin"""
    case, rs = run_grid_case("count_%d" % P)
    assert rs[False].nmatch[0] == P and rs[True].nmatch[0] == P


def raw_all(dev, dist, case, nm_cap, sep=0, tail=64):
    """ssg_rank_metrics_all on a contiguous block with every output pre-filled -> numpy (first, ap, overflow, nm_before [m, nm_cap],
    the `tail` words behind it, nmatch)"""
    from ssg_amd import _lib
    L = _lib.lib()
    d = torch.from_numpy(np.ascontiguousarray(dist, dtype=np.float32)).to(dev)
    m, n = d.shape
    assert all(np.abs(case[k]).max() < 2 ** 31 for k in ("qid", "gid"))            # the cases that come here fit int32 as they are
    tq, tqc, tg, tgc = (torch.from_numpy(np.asarray(case[k]).astype(np.int32)).to(dev) for k in ("qid", "qcam", "gid", "gcam"))
    first = torch.full((m,), CANARY, dtype=torch.int32, device=dev); ap = torch.full((m,), 123.0, dtype=torch.float64, device=dev)
    ovf = torch.full((1,), CANARY, dtype=torch.int32, device=dev)
    nmb = torch.full((m * nm_cap + tail,), CANARY, dtype=torch.int32, device=dev); nm = torch.full((m,), CANARY, dtype=torch.int32, device=dev)
    _lib.check(L.ssg_rank_metrics_all(_lib.ptr(d), m, n, d.stride(0), _lib.ptr(tq), _lib.ptr(tqc), _lib.ptr(tg), _lib.ptr(tgc), sep,
                                      _lib.ptr(first), _lib.ptr(ap), _lib.ptr(ovf), _lib.ptr(nmb), _lib.ptr(nm), nm_cap, _lib.stream()),
               "ssg_rank_metrics_all")
    torch.cuda.synchronize()
    nmb = nmb.cpu().numpy()
    return (first.cpu().numpy(), ap.cpu().numpy(), int(ovf.item()), nmb[:m * nm_cap].reshape(m, nm_cap), nmb[m * nm_cap:], nm.cpu().numpy())


def test_match_cap_overflow(dev):
    """2049 valid true matches: every Python entry point raises SSGError (an ordinary error return: the gather stores slot k only
    while k < 2048); through the raw entry point the query is marked -1 / NaN / 0 matches, the word counts it, and the ordinary
    query next to it is evaluated as if it were alone"""
    from ssg_amd import SSGError, ranking
    case = ref.match_count_case(ref.RK_CAP + 1)
    a = ref.args(case)
    for call in (lambda: ranking.per_query(*a), lambda: ranking.per_query_all(*a), lambda: ranking.cmc(*a), lambda: ranking.mean_ap(*a),
                 lambda: ranking.cmc(*a, first_match_break=True), lambda: ranking.cmc(*a, separate_camera_set=True)):
        with pytest.raises(SSGError, match="more than 2048 true matches") as e:
            call()
        assert type(e.value) is SSGError                      # not the NaN error
    r = ref.per_query(*a)
    assert list(r.nmatch) == [ref.RK_CAP + 1, 5, 0]
    first, ap, ovf, nmb, tail, nm = raw_all(dev, case["dist"], case, nm_cap=ref.RK_CAP)
    assert ovf == 1 and list(first) == [-1, r.first[1], -1] and list(nm) == [0, 5, 0]
    assert np.isnan(ap[0]) and np.isnan(ap[2])
    assert abs(Fraction(float(ap[1])) - r.ap_exact[1]) <= ref.ap_bound(5)
    assert np.array_equal(nmb[1, :5], r.bins[1])
    assert (nmb[0] == CANARY).all() and (nmb[1, 5:] == CANARY).all() and (nmb[2] == CANARY).all() and (tail == CANARY).all()


# ------------------------------------------------------------------ gallery-size edges
@pytest.mark.parametrize("n", ref.GALLERY_SIZES)
def test_gallery_size(dev, n):
    """n around the 256-thread stride, m = 1 and m = 3; a query whose only match is the last column, one whose only match is column 0"""
    for name in ("size_%d_m1_last" % n, "size_%d_m1_first" % n, "size_%d_m3" % n):
        case, rs = run_grid_case(name)
        assert rs[False].nmatch[0] == 1


# ------------------------------------------------------------------ row pitch and layout
@pytest.mark.parametrize("poison", [NAN, -1e30])
@pytest.mark.parametrize("name", ["count_257", "tie_three_values", "size_257_m3", "size_1_m3"])
def test_pitch_and_layout(dev, name, poison):
    """ld > n with poisoned padding columns (a CUDA view padded[:, :n]) and a transposed view with poisoned padding rows (column
    stride != 1, which the wrapper makes contiguous): the padding is never read as data -- NaN would raise or mark the query,
    -1e30 would be ranked first"""
    from ssg_amd import ranking
    case = ref.GRID[name]()
    rs = {sep: reference(name, case, sep) for sep in (False, True)}
    m, n = case["dist"].shape
    d = torch.from_numpy(case["dist"]).to(dev)
    padded = torch.full((m + 1, n + 37), poison, dtype=torch.float32, device=dev)
    padded[:m, :n] = d
    view = padded[:m, :n]
    assert view.stride(0) == n + 37 and view.stride(1) == 1
    check_against_reference(ranking, view, case, name + " padded", rs)
    tpadded = torch.full((n + 5, m + 3), poison, dtype=torch.float32, device=dev)
    tpadded[:n, :m] = d.t()
    tview = tpadded[:n, :m].t()
    assert tview.shape == (m, n) and tview.stride(1) == m + 3
    check_against_reference(ranking, tview, case, name + " transposed", rs)
    assert torch.equal(padded[:m, :n], d) and torch.equal(tpadded[:n, :m], d.t())          # and nothing was written to the block


def test_row_pitch_below_n(dev):
    """blocks whose row stride is below n -- a broadcast row, a [n, 1] column seen as [1, n] -- are made contiguous, not refused"""
    from ssg_amd import ranking
    name = "tie_three_values"
    case = ref.GRID[name]()
    row = dict(case, dist=np.repeat(case["dist"][:1], 4, axis=0))
    rs = {sep: ref.per_query(*ref.args(row), separate_camera_set=sep) for sep in (False, True)}
    n = row["dist"].shape[1]
    one = torch.from_numpy(case["dist"][0]).to(dev)
    bcast = one[None, :].expand(4, n)
    assert bcast.stride(0) == 0
    check_against_reference(ranking, bcast, row, "broadcast row", rs)
    single = dict(case, dist=case["dist"][:1], qid=case["qid"][:1], qcam=case["qcam"][:1])
    col = one.clone().reshape(n, 1).t()
    check_against_reference(ranking, col, single, "column as a row", {sep: ref.per_query(*ref.args(single), separate_camera_set=sep) for sep in (False, True)})


def test_list_lengths_are_checked(dev):
    """id / camera lists that do not match the block are refused before anything is launched, by both entry points"""
    from ssg_amd import ranking
    d = np.zeros((2, 5), np.float32)
    for f in (ranking.per_query, ranking.per_query_all, ranking.cmc, ranking.mean_ap):
        with pytest.raises(ValueError, match="do not match"):
            f(d, [1, 2], [1, 2, 3, 4], [0, 0], [1, 1, 1, 1, 1])
        with pytest.raises(ValueError, match="do not match"):
            f(d, [1, 2, 3], [1, 2, 3, 4, 5], [0, 0], [1, 1, 1, 1, 1])


# ------------------------------------------------------------------ ties
@pytest.mark.parametrize("kind", ref.TIE_KINDS)
def test_ties(dev, kind):
    """a match tied with valid non-matches at lower and higher gallery indices (tests/test_rank_ref_host.py checks that every case
    has one): the (distance, index) order decides the first rank and the all-shots bins, equal distances form one AP threshold.
    Infinities are ordered values; -0.0 is 0.0; denormals are not flushed"""
    run_grid_case("tie_" + kind)


# ------------------------------------------------------------------ validity
@pytest.mark.parametrize("kind", ref.VALIDITY_KINDS)
def test_validity(dev, kind):
    case, rs = run_grid_case("valid_" + kind)
    if kind == "mixed":
        assert list(rs[False].first >= 0) == [True, False, False, True, True, True]
    if kind == "id_wrap":
        # what a cast of the ids to int32 would compute differs from the reference: the case can tell the two apart
        wrapped = ref.per_query(case["dist"], case["qid"].astype(np.int32), case["gid"].astype(np.int32), case["qcam"], case["gcam"])
        assert not np.array_equal(wrapped.first, rs[False].first) and not np.array_equal(wrapped.nmatch, rs[False].nmatch)
    if kind == "separate_cameras":
        assert list(rs[False].nmatch) != list(rs[True].nmatch) or list(rs[False].first) != list(rs[True].first)


def test_no_valid_query(dev):
    from ssg_amd import ranking
    a = ref.args(ref.validity_case("all_invalid"))
    first, ap = ranking.per_query(*a)
    assert list(first.cpu().numpy()) == [-1, -1] and np.isnan(ap.cpu().numpy()).all()
    nm, nmb = ranking.per_query_all(*a)
    assert list(nm) == [0, 0] and not nmb.any()
    for call in (lambda: ranking.cmc(*a), lambda: ranking.cmc(*a, first_match_break=True), lambda: ranking.cmc(*a, separate_camera_set=True),
                 lambda: ranking.mean_ap(*a)):
        with pytest.raises(RuntimeError, match="No valid query"):
            call()


# ------------------------------------------------------------------ nm_cap below the match count (a C caller's choice)
@pytest.mark.parametrize("nm_cap", [1, 299])
def test_nm_cap_below_match_count(dev, nm_cap):
    """P = 300 with room for nm_cap bins per row: exactly min(P, nm_cap) entries of each row are written, the canaries behind them
    (the rest of a shorter row, the row of a query without matches, the words behind the buffer) are intact, nmatch is still P"""
    P = 300
    case = ref.match_count_case(P)
    r = ref.per_query(*ref.args(case))
    assert list(r.nmatch) == [P, 5, 0]
    first, ap, ovf, nmb, tail, nm = raw_all(dev, case["dist"], case, nm_cap)
    assert ovf == 0 and np.array_equal(first, r.first) and np.array_equal(nm, r.nmatch)
    check_ap(ap, r, "nm_cap", "nm_cap=%d" % nm_cap)
    for q in range(3):
        lim = min(int(r.nmatch[q]), nm_cap)
        assert np.array_equal(nmb[q, :lim], r.bins[q][:lim]), q
        assert (nmb[q, lim:] == CANARY).all(), q
    assert (tail == CANARY).all()


# ------------------------------------------------------------------ topk
def test_topk_edges(dev):
    """topk = 1, topk beyond the gallery, and the all-shots stop rule with a bin equal to topk (credited to nobody, and the loop
    stops there: the reference's `if k - j >= topk: break`)"""
    from ssg_amd import ranking
    for name in ("valid_mixed", "tie_three_values"):
        case = ref.GRID[name]()
        rs = {sep: reference(name, case, sep) for sep in (False, True)}
        n = case["dist"].shape[1]
        exact_bins = sorted({int(b[k]) for b in rs[False].bins for k in range(1, len(b)) if b[k] > b[0]})
        assert exact_bins, name                               # a topk that equals a later bin of a query whose first bin is below it
        check_against_reference(ranking, case["dist"], case, name + " topk", rs, topks=(1, n + 50, exact_bins[0], exact_bins[len(exact_bins) // 2]))


# ------------------------------------------------------------------ NaN distances
def _entries_of_query(case, q, sep):
    """(filtered, valid matches, valid non-matches) gallery columns of query q"""
    qid, gid, qcam, gcam = case["qid"], np.asarray(case["gid"]), case["qcam"], np.asarray(case["gcam"])
    valid = (gcam != qcam[q]) if sep else ((gid != qid[q]) | (gcam != qcam[q]))
    return np.flatnonzero(~valid), np.flatnonzero(valid & (gid == qid[q])), np.flatnonzero(valid & (gid != qid[q]))


@pytest.mark.parametrize("sep", [False, True])
def test_nan_in_filtered_entries_is_not_read(dev, sep):
    """NaN in every entry the id / camera filter removes for query 0, and a whole NaN row for a query without a valid true match:
    no error, and query 0's numbers are those of the block with these columns removed"""
    from ssg_amd import ranking
    case = ref.validity_case("mixed")
    dist, qid, gid, qcam, gcam = ref.args(case)
    filtered, match, other = _entries_of_query(case, 0, sep)
    assert len(filtered) and len(match) and len(other)
    d = dist.copy(); d[0, filtered] = np.nan; d[1] = np.nan
    keep = np.setdiff1d(np.arange(dist.shape[1]), filtered)
    removed = ref.per_query(dist[:1, keep], qid[:1], gid[keep], qcam[:1], gcam[keep], separate_camera_set=sep)
    whole = ref.per_query(dist, qid, gid, qcam, gcam, separate_camera_set=sep)
    assert removed.first[0] == whole.first[0] and removed.ap_exact[0] == whole.ap_exact[0] and np.array_equal(removed.bins[0], whole.bins[0])
    first, ap = ranking.per_query(d, qid, gid, qcam, gcam, separate_camera_set=sep)
    assert np.array_equal(first.cpu().numpy(), whole.first) and first[0] == removed.first[0]
    check_ap(ap.cpu().numpy(), whole, "nan_filtered", "filtered NaN sep=%d" % sep)
    assert abs(Fraction(float(ap[0])) - removed.ap_exact[0]) <= ref.ap_bound(int(removed.nmatch[0]))
    nm, nmb = ranking.per_query_all(d, qid, gid, qcam, gcam, separate_camera_set=sep)
    assert np.array_equal(nm, whole.nmatch) and np.array_equal(nmb[0, :nm[0]], removed.bins[0])
    for fmb in (False, True):
        assert np.array_equal(ranking.cmc(d, qid, gid, qcam, gcam, separate_camera_set=sep, first_match_break=fmb),
                              ref.cmc(dist, qid, gid, qcam, gcam, separate_camera_set=sep, first_match_break=fmb, result=whole))
    if not sep:
        exact, pmax = ref.mean_ap_exact(whole)
        assert abs(Fraction(float(ranking.mean_ap(d, qid, gid, qcam, gcam))) - exact) <= ref.ap_bound(pmax)


@pytest.mark.parametrize("where", ["match", "non_match"])
def test_nan_in_a_valid_entry_raises(dev, where):
    """a NaN in a valid true match, and separately in a valid non-match, of queries 3 and 5: every entry point raises RankNaNError
    naming query 3; through the raw entry point the two queries are marked -2 / NaN / 0 matches, the word counts them, and the
    other queries' outputs are those of the clean block"""
    from ssg_amd import SSGError, ranking
    case = ref.validity_case("mixed")
    dist, qid, gid, qcam, gcam = ref.args(case)
    clean = ref.per_query(*ref.args(case))
    d = dist.copy()
    for q in (3, 5):
        _, match, other = _entries_of_query(case, q, False)
        d[q, (match if where == "match" else other)[-1]] = np.nan
    a = (d, qid, gid, qcam, gcam)
    for call in (lambda: ranking.per_query(*a), lambda: ranking.per_query_all(*a), lambda: ranking.cmc(*a), lambda: ranking.mean_ap(*a),
                 lambda: ranking.cmc(*a, first_match_break=True), lambda: ranking.per_query(torch.from_numpy(d).to(dev), *a[1:])):
        with pytest.raises(SSGError, match="query 3 has a NaN") as e:
            call()
        assert type(e.value) is ranking.RankNaNError
    first, ap, ovf, nmb, tail, nm = raw_all(dev, d, case, nm_cap=64)
    assert ovf == 2
    for q in range(6):
        if q in (3, 5):
            assert first[q] == -2 and np.isnan(ap[q]) and nm[q] == 0 and (nmb[q] == CANARY).all()
        else:
            assert first[q] == clean.first[q] and nm[q] == clean.nmatch[q] and np.array_equal(nmb[q, :nm[q]], clean.bins[q])
            if clean.ap_exact[q] is None:
                assert np.isnan(ap[q])
            else:
                assert abs(Fraction(float(ap[q])) - clean.ap_exact[q]) <= ref.ap_bound(int(clean.nmatch[q]))
    assert (tail == CANARY).all()


def test_nan_among_many_matches(dev):
    """the NaN in the last of 257 matches (gathered in the second trip of the 256-thread loop), and in the last valid non-match"""
    from ssg_amd import SSGError, ranking
    case = ref.match_count_case(257)
    for pick in (1, 2):
        cols = _entries_of_query(case, 0, False)[pick]
        d = case["dist"].copy(); d[0, cols[-1]] = np.nan
        with pytest.raises(SSGError, match="query 0 has a NaN") as e:
            ranking.mean_ap(d, *ref.args(case)[1:])
        assert type(e.value) is ranking.RankNaNError
        d = case["dist"].copy(); d[2, cols[-1]] = np.nan          # query 2 has no valid true match: skipped before its row is ranked
        assert np.array_equal(ranking.per_query(d, *ref.args(case)[1:])[0].cpu().numpy(), reference("count_257", case, False).first)


# ------------------------------------------------------------------ determinism, input dtype
@pytest.mark.parametrize("name", ["count_1023", "tie_three_values", "tie_plus_inf"])
def test_two_calls_same_bits(dev, name):
    from ssg_amd import ranking
    a = ref.args(ref.GRID[name]())
    one, two = ranking.per_query(*a), ranking.per_query(*a)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1].view(torch.int64), two[1].view(torch.int64))
    one, two = ranking.per_query_all(*a), ranking.per_query_all(*a)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    assert np.array_equal(ranking.cmc(*a), ranking.cmc(*a)) and ranking.mean_ap(*a).tobytes() == ranking.mean_ap(*a).tobytes()


@pytest.mark.parametrize("name", ["count_255", "tie_three_values"])
def test_input_dtype(dev, name):
    """a float64 block and a float16 block whose values float32 holds exactly give the float32 block's bits (numpy, CPU and CUDA tensors)"""
    from ssg_amd import ranking
    dist, *ids = ref.args(ref.GRID[name]())
    assert np.array_equal(dist.astype(np.float16).astype(np.float32), dist)
    first, ap = ranking.per_query(dist, *ids)
    nm, nmb = ranking.per_query_all(dist, *ids)
    for other in (dist.astype(np.float64), dist.astype(np.float16), torch.from_numpy(dist.astype(np.float64)), torch.from_numpy(dist.astype(np.float16)).to(dev),
                  torch.from_numpy(dist).to(dev)):
        f2, ap2 = ranking.per_query(other, *ids)
        assert torch.equal(first, f2) and torch.equal(ap.view(torch.int64), ap2.view(torch.int64))
        nm2, nmb2 = ranking.per_query_all(other, *ids)
        assert np.array_equal(nm, nm2) and np.array_equal(nmb, nmb2)
