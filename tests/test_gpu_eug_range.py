"""GPU half of the whole-range tests of the SSG++ label step (csrc/eug.hip behind ssg_amd.eug): kernel a (ssg_eug_nn_f32) at every
width class, row-count structure, exact tie and special value it accepts, kernel b (ssg_eug_dist_label_f32) at its shape edges and
the selection kernel around its 1024-thread block -- each against numpy itself (tests/eug_ref.py; tests/test_eug_range_host.py
holds the restatements and the case tables to the installed numpy without a GPU).  Every comparison is for equal bits: argmin, min
as uint32, labels, scores as -min widened to float64, NaN at the same places.  There is no tolerance in this file."""
import numpy as np
import pytest
import torch

import eug_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def u32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_f64(a, b):
    """equal bits, NaN at the same places"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype == np.float64 and a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def splits(nu, nl):
    from ssg_amd import _lib
    return int(_lib.lib().ssg_eug_nn_splits(nu, nl))


def run_nn(u, l, l_label, dev):
    from ssg_amd.eug import nearest_labelled
    labels, scores, argmin, minval = nearest_labelled(torch.from_numpy(u).to(dev), torch.from_numpy(l).to(dev), l_label)
    torch.cuda.synchronize()
    assert labels.dtype == torch.int64 and scores.dtype == torch.float64 and argmin.dtype == torch.int32 and minval.dtype == torch.float32
    return labels.cpu().numpy(), scores.cpu().numpy(), argmin.cpu().numpy(), minval.cpu().numpy()


def check_nn(u, l, dev, seed=0, tag=None):
    """nearest_labelled against numpy row by row: argmin, min bits (NaN at the same places), labels, scores; -> numpy's (argmin, min)"""
    l_label = ref.labels_perm(len(l), seed)
    lab, sc, am, mv = run_nn(u, l, l_label, dev)
    want_am, want_mv = ref.nn_ref(u, l)
    bad = np.flatnonzero(am != want_am)
    assert bad.size == 0, (tag, "argmin", bad[:8], am[bad[:8]], want_am[bad[:8]])
    nan = np.isnan(want_mv)
    assert np.array_equal(np.isnan(mv), nan), (tag, "NaN positions")
    bad = np.flatnonzero((u32(mv) != u32(want_mv)) & ~nan)
    assert bad.size == 0, (tag, "min", bad[:8], mv[bad[:8]], want_mv[bad[:8]])
    assert np.array_equal(lab, l_label[want_am]), tag
    with np.errstate(all="ignore"):
        assert same_f64(sc, (-want_mv).astype(np.float64)), tag
    return want_am, want_mv


# ------------------------------------------------------------------ kernel a: widths


@pytest.mark.parametrize("d", ref.D_EDGE)
def test_nearest_labelled_every_width_class(dev, d):
    """Nu = 33, Nl = 130: two u blocks (the second ragged), three l tiles (the last ragged), three splits; at 8191 and 32768 also
    with a wide dynamic range"""
    ns = splits(ref.NU, ref.NL)
    assert ns == 3 and ref.structure(ref.NU, ref.NL, ns) == (2, 3, 1)
    for wide in ([False, True] if d in ref.D_WIDE else [False]):
        u, l = ref.features(ref.NU, ref.NL, d, ref.width_seed(d), wide=wide)
        check_nn(u, l, dev, seed=d, tag=(d, wide))


# ------------------------------------------------------------------ kernel a: row counts
ROW_CASES = [(1, 1, 9), (1, 64, 9), (31, 63, 9), (32, 64, 9), (33, 65, 9), (64, 129, 9), (8197, 1283, 9), (65600, 130, 3)]


@pytest.mark.parametrize("nu, nl, d", ROW_CASES)
def test_nearest_labelled_row_count_structures(dev, nu, nl, d):
    ns = splits(nu, nl)
    ublocks, ntiles, per = ref.structure(nu, nl, ns)
    if (nu, nl) == (8197, 1283):                 # 20 whole tiles and a ragged one, several splits of more than one tile each
        assert ntiles == 21 and nl % ref.TL and ns >= 2 and per >= 2 and nu % ref.TU
    elif (nu, nl) == (65600, 130):               # one split over three tiles (more u blocks than the split heuristic wants workgroups)
        assert ns == 1 and ntiles == 3 and per == 3 and ublocks == 2050
    else:                                        # small and ragged: one split per tile
        assert ublocks == -(-nu // 32) <= 2 and ntiles == -(-nl // 64) <= 3 and per == 1 and ns == ntiles
    u, l = ref.features(nu, nl, d, 100 + nu)
    check_nn(u, l, dev, seed=nu, tag=(nu, nl, d))


# ------------------------------------------------------------------ kernel a: exact ties


@pytest.mark.parametrize("kind", ref.TIE_KINDS)
@pytest.mark.parametrize("nu, nl, d", ref.TIE_SHAPES)
def test_nearest_labelled_ties_first_index_wins(dev, nu, nl, d, kind):
    ns = splits(nu, nl)
    _, ntiles, per = ref.structure(nu, nl, ns)
    u, l, aim, groups = ref.tie_case(nu, nl, d, kind, per, 300 + len(kind) + nu)
    tile = lambda j: j // ref.TL                  # noqa: E731
    split = lambda j: tile(j) // per              # noqa: E731
    for j, copies in groups:                     # the case has the structure it is named for
        c = copies[0]
        if kind in ("next", "zero"):
            assert c == j + 1
        elif kind == "lanes":
            assert j // 16 == c // 16
        elif kind == "column":
            assert tile(j) == tile(c) and j // 16 != c // 16
        elif kind == "tile":
            assert tile(c) == tile(j) + 1 and (per == 1 or split(c) == split(j))
        elif kind == "splits":
            assert split(c) != split(j)
        elif kind == "ragged":
            assert tile(c) == ntiles - 1 and nl % ref.TL
    if kind == "column":
        assert any(c[0] % 16 < j % 16 for j, c in groups)                 # a copy in a lower lane than its original
    if kind == "everywhere":
        assert len({split(c) for c in groups[0][1]}) >= 2 and len({tile(c) for c in groups[0][1]}) >= 3
    want_am, want_mv = check_nn(u, l, dev, seed=nl, tag=(kind, nu, nl, d))
    # the reference itself: every aimed row answers the ORIGINAL of its group, the copies stand at exactly its distance
    with np.errstate(all="ignore"):
        for r, q in aim.items():
            j, copies = groups[q]
            assert want_am[r] == j, (kind, r)
            dist = np.linalg.norm(l[[j] + list(copies)] - u[r], axis=1)
            assert (u32(dist) == u32(want_mv[r:r + 1])).all()
    zeros = sum(1 for r in aim if want_mv[r] == 0)
    assert zeros >= (len(aim) if kind == "zero" else len(groups) if kind != "all_equal" else 0)
    if kind == "all_equal":
        assert (want_am == 0).all()


# ------------------------------------------------------------------ kernel a: special values


@pytest.mark.parametrize("kind", ref.SPECIAL_KINDS)
@pytest.mark.parametrize("d", ref.SPECIAL_WIDTHS)
def test_nearest_labelled_special_values(dev, d, kind):
    u, l = ref.special_case(kind, d, 500 + d)
    am, mv = check_nn(u, l, dev, seed=d, tag=(kind, d))
    # the reference answers what the case is for
    if kind == "nan_l":
        assert (am == 70).all() and np.isnan(mv).all()
    elif kind == "nan_l2_splits":
        assert (am == 20).all() and np.isnan(mv).all()
    elif kind == "nan_l2_tile":
        assert (am == 64 + 15).all() and np.isnan(mv).all()
    elif kind == "nan_u":
        assert am[17] == 0 and am[32] == 0 and np.isnan(mv[[17, 32]]).all() and np.isnan(mv).sum() == 2
    elif kind == "inf_l":
        assert (am != 5).all() and np.isfinite(mv).all()
    elif kind == "inf_u":
        assert am[3] == 0 and am[32] == 0 and np.isposinf(mv[[3, 32]]).all() and np.isfinite(np.delete(mv, [3, 32])).all()
    elif kind == "inf_both":
        assert am[9] == 77 and am[32] == 129 and np.isnan(mv[[9, 32]]).all() and np.isnan(mv).sum() == 2
    elif kind == "overflow":
        assert (am == 0).all() and np.isposinf(mv).all()
    elif kind == "denormal":
        # the distance itself is a normal number (the root of a denormal is); what must be neither zero nor normal is the sum of
        # squares under it, and every single square
        tiny = np.finfo(F32).tiny
        sq = (l[am] - u) * (l[am] - u)
        s = sq.sum(axis=1, dtype=F32)
        assert (s > 0).all() and (s < tiny).all() and (sq < tiny).all() and (mv > 0).all()


# ------------------------------------------------------------------ kernel a: wrapper inputs


def test_nearest_labelled_wrapper_inputs(dev):
    """float64 and float16 numpy features, a non-contiguous slice, a CPU torch tensor and a CUDA tensor give the bits of the float32
    contiguous CUDA input; int32 labels, negative labels and labels above 2^31 are carried through unchanged"""
    from ssg_amd.eug import estimate_label_device, nearest_labelled
    rng = np.random.default_rng(9)
    nu, nl, d = 33, 130, 137
    u64, l64 = rng.standard_normal((nu, d)), rng.standard_normal((nl, d))
    u, l = u64.astype(F32), l64.astype(F32)
    assert not np.array_equal(u.astype(np.float64), u64)
    l_label = ref.labels_perm(nl, 1)
    base = run_nn(u, l, l_label, dev)
    want_am, want_mv = ref.nn_ref(u, l)
    assert np.array_equal(base[2], want_am) and np.array_equal(u32(base[3]), u32(want_mv))

    def same(out, want=base):
        out = [t.cpu().numpy() for t in out]
        return all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(out, want))
    assert same(nearest_labelled(u64, l64, l_label))                                       # float64 numpy, rounded to float32 once
    assert same(nearest_labelled(torch.from_numpy(u), torch.from_numpy(l), l_label))       # CPU tensors
    assert same(nearest_labelled(torch.from_numpy(u).to(dev), l, l_label.tolist()))        # CUDA and numpy mixed, a list of labels
    wide_u, wide_l = np.zeros((nu, 2 * d), F32), np.zeros((2 * nl, d + 3), F32)
    wide_u[:, ::2] = u
    wide_l[::2, 3:] = l
    assert not wide_u[:, ::2].flags.c_contiguous and not wide_l[::2, 3:].flags.c_contiguous
    assert same(nearest_labelled(wide_u[:, ::2], wide_l[::2, 3:], l_label))                # non-contiguous numpy slices
    assert same(nearest_labelled(torch.from_numpy(wide_u).to(dev)[:, ::2], torch.from_numpy(wide_l).to(dev)[::2, 3:], l_label))
    uh, lh = u.astype(np.float16), l.astype(np.float16)
    half = run_nn(uh.astype(F32), lh.astype(F32), l_label, dev)
    assert same(nearest_labelled(uh, lh, l_label), half) and not np.array_equal(half[3], base[3])
    am16, mv16 = ref.nn_ref(uh.astype(F32), lh.astype(F32))
    assert np.array_equal(half[2], am16) and np.array_equal(u32(half[3]), u32(mv16))
    # labels
    for lab in (l_label.astype(np.int32), -l_label, l_label + (1 << 31), l_label * (1 << 40) - 5):
        out = nearest_labelled(u, l, lab)[0].cpu().numpy()
        assert out.dtype == np.int64 and np.array_equal(out, np.asarray(lab).astype(np.int64)[want_am])
    labels, scores = estimate_label_device(u, l, -l_label, rerank=False)
    assert labels.dtype == scores.dtype == np.float64 and np.array_equal(labels, (-l_label)[want_am].astype(np.float64))
    assert same_f64(scores, (-want_mv).astype(np.float64))


def test_nearest_labelled_refusals(dev):
    """d = 32769 raises the C layer's message, a label count that does not match raises; both before any launch"""
    from ssg_amd.eug import nearest_labelled
    z = torch.zeros(2, 32769, device=dev)
    with pytest.raises(ValueError, match=r"ssg_eug_nn_f32: need nu, nl > 0 and 0 < d <= 32768"):
        nearest_labelled(z, z, np.arange(2))
    with pytest.raises(ValueError, match=r"l_label \[Nl\] expected"):
        nearest_labelled(z[:, :9], z[:, :9], np.arange(3))
    with pytest.raises(ValueError, match="expected"):
        nearest_labelled(z[:, :9], z[:, :8], np.arange(2))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ kernel b


@pytest.mark.parametrize("kind", ref.DIST_KINDS)
@pytest.mark.parametrize("nu, nl", ref.DIST_SHAPES)
def test_dist_label_shape_edges(dev, nu, nl, kind):
    """Nu below, at and around the 64 row chunks of the column-max pass, Nl = 1, several 256-column blocks, ties 1 and 64 columns
    apart, NaN, negative and infinite entries, against the reference's loop on numpy"""
    from ssg_amd.eug import dissimilarity_from_dist
    D = ref.dist_case(nu, nl, kind, 900 + nu + nl)
    l_label = ref.labels_perm(nl, nl)
    want_lab, want_sc, want_conf, want_am = ref.dist_label_ref(D, l_label)
    lab, sc, conf, am = dissimilarity_from_dist(torch.from_numpy(D).to(dev), l_label, return_argmin=True)
    assert np.array_equal(am, want_am), np.flatnonzero(am != want_am)[:8]
    assert same_f64(lab, want_lab) and same_f64(sc, want_sc)
    assert same_f64(conf, want_conf), np.flatnonzero(~((conf == want_conf) | (np.isnan(conf) & np.isnan(want_conf))))[:8]
    # the case shows what it is for
    with np.errstate(all="ignore"):
        mins = D[np.arange(nu), want_am]
        if nu >= 6 and nl >= 130:
            assert ((D == mins[:, None]).sum(axis=1) >= 2).sum() >= 3     # rows with equal minima
            tied64 = [(D[r, want_am[r] + 64:] == mins[r]).any() for r in range(nu) if want_am[r] + 64 < nl]
            assert any(tied64)
        if kind == "nan" and nl > 70:
            both = np.flatnonzero(np.isnan(D[:, 5]) & np.isnan(D[:, 70]))
            assert both.size == 1 and want_am[both[0]] == 5 and np.isnan(want_sc[both[0]])
        if kind == "nan_column" and nu >= 6 and nl > 1:
            assert 0 < np.isnan(want_conf).sum() < nu and not np.isnan(want_sc).all()
        if kind == "negative" and nu * nl > 1:
            assert (mins < 0).any() and (nl <= 2 or (np.max(D, axis=0) < 0).any())
        if kind == "inf":
            assert np.isneginf(mins).any() and (nl == 1 or np.isposinf(D).any())


def test_dist_label_wrapper_inputs(dev):
    """a transposed (non-contiguous) view and a float64 input give what their float32 contiguous copy gives"""
    from ssg_amd.eug import dissimilarity_from_dist
    D = ref.dist_case(257, 65, "negative", 4)
    l_label = ref.labels_perm(65, 2)
    want = ref.dist_label_ref(D, l_label)
    Dt = np.ascontiguousarray(D.T)
    assert not Dt.T.flags.c_contiguous
    for x in (Dt.T, torch.from_numpy(Dt).to(dev).t(), D.astype(np.float64), torch.from_numpy(D.astype(np.float64)).to(dev), D):
        out = dissimilarity_from_dist(x, l_label, return_argmin=True)
        assert all(same_f64(a, b) for a, b in zip(out[:3], want[:3])) and np.array_equal(out[3], want[3])
    D64 = D.astype(np.float64) * (1 + 2.0 ** -30)                         # not float32 values: rounded once, like astype
    out = dissimilarity_from_dist(D64, l_label)
    want = ref.dist_label_ref(D64.astype(F32), l_label)
    assert all(same_f64(a, b) for a, b in zip(out, want[:3]))
    with pytest.raises(ValueError, match="l_label has 64 entries for 65 columns"):
        dissimilarity_from_dist(D, l_label[:64])


# ------------------------------------------------------------------ selection


@pytest.mark.parametrize("kind", ref.SELECT_KINDS)
@pytest.mark.parametrize("n", ref.SELECT_N)
def test_select_top_around_the_block_size(dev, n, kind):
    """sizes around the 1024-thread block; all-equal, all-NaN, infinite and mixed NaN scores; k = 0, 1, n - 1, n and both sides of a
    tie that straddles the cut; labels with -1 and NaN -- against the first k of a stable argsort of -scores"""
    from ssg_amd.eug import select_top
    scores = ref.select_case(n, kind, n + len(kind))
    labels = ref.select_labels(n, n)
    assert (labels == -1).any() and np.isnan(labels).any()
    sd = torch.from_numpy(scores).to(dev)
    ks = ref.select_ks(scores)
    assert {0, 1, n - 1, n} <= set(ks) and len(ks) >= 5
    for k in ks:
        want = ref.select_ref(scores, k)
        got = select_top(sd, k)
        assert got.dtype == bool and want.sum() == k and np.array_equal(got, want), (n, kind, k)
        assert np.array_equal(select_top(scores, k, labels=labels), ref.select_ref(scores, k, labels)), (n, kind, k)
    for k in (-1, n + 1):
        with pytest.raises(ValueError, match=r"outside \[0, %d\]" % n):
            select_top(sd, k)
