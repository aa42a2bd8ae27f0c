"""Host side of the source term's filter-and-refine contract (no GPU): tests/source_bound_ref.py restates the operation as the oracle
does, rerank.source_bound_params keeps its properties and its values, and every input of tests/test_gpu_source_bound.py is what it
claims to be in float64 -- including that the one-product bound, emulated without accumulation error, stays within tol / 2."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import clustered
from ssg_amd import rerank

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import source_bound_ref as ref  # noqa: E402


# ------------------------------------------------------------------ the restatement agrees with the oracle
@pytest.mark.parametrize("N,Ns,d", [(60, 77, 96), (129, 45, 64), (33, 260, 160)])
def test_rowmin_bits_equals_the_oracle(N, Ns, d, ora):
    tgt = clustered(N, d, 3); src = clustered(Ns, d, 4, intra=0.7)
    tgt[7] = tgt[2]; src[5] = tgt[9]                    # an exact zero among the minima
    b = ref.rowmin_bits(tgt, src)
    v_raw, v, mx = ora.source_vec(tgt, src)
    # the oracle returns 1 - exp(-min) in half arithmetic: monotone in the bits, so apply it to every half and look the bits up
    one_minus_exp = (np.float16(1) - ora.half_exp_table()[(np.arange(0x7C01) ^ 0x8000)]).astype(np.float16)
    assert np.array_equal(one_minus_exp[b].view(np.uint16), v_raw.view(np.uint16))
    assert b[9] == 0 and np.array_equal(b, ref.half_bits_of(ref.sqdist(tgt, src)).min(axis=1))
    gm, padded = ref.granule_min(tgt, ref.pad_rows(src, Ns + (-Ns) % 128), Ns, 8)
    assert np.array_equal(ref.half_bits_of(gm[:, ~padded].min(axis=1)), b) and padded.sum() == ((-Ns) % 128) // 8


# ------------------------------------------------------------------ rerank.source_bound_params
STATS = [(0.4375, 0.5, 1.0000001192092896, 1.000000238418579), (3000.5, 0.001953125, 17000.25, 0.0625), (0.0, 0.3, 0.0, 1.5), (70.0, 1e-7, 90.0, 3e-7),
         (16384.0, 16385.0, 20000.0, 20000.0), (1e-30, 1e-3, 1e-30, 1e-3)]


@pytest.mark.parametrize("stats", STATS)
@pytest.mark.parametrize("bound", ref.BOUNDS)
def test_params_scales_and_workspace(stats, bound):
    nrows, Ns_pad, d = 389, 256, 96
    tol, st, ss, nws = rerank.source_bound_params(stats, d, bound, nrows, Ns_pad)
    assert tol > 0 and math.isfinite(tol)
    if bound == "f32":
        assert st == 0.0 and ss == 0.0
        assert nws == nrows + Ns_pad + nrows * (Ns_pad // 8)                       # header comment of source_rowmin_filtered_impl
        return
    assert nws == nrows + Ns_pad + nrows * (Ns_pad // 8) + (nrows + Ns_pad) * d
    for s, m in ((st, stats[0]), (ss, stats[1])):
        assert 0 < s <= 256.0 and math.frexp(s)[0] == 0.5                          # a power of two
        assert m * s <= 16384.0
        assert s == 256.0 or m * s > 8192.0                                        # and the largest one allowed
    if stats[0] == 0.0:
        assert st == 256.0                                                         # mt == 0


def test_params_scale_branches():
    p = lambda mt, ms: rerank.source_bound_params((mt, ms, 1.0, 1.0), 64, "half", 8, 256)[1:3]   # noqa: E731
    assert p(0.0, 0.0) == (256.0, 256.0)
    assert p(64.0, 64.0000076) == (256.0, 128.0)        # mt > 64 is where the scale leaves 256
    assert p(1500.0, 16384.0) == (8.0, 1.0)
    assert p(1e-6, 40000.0) == (256.0, 0.25)


@pytest.mark.parametrize("bound", ref.BOUNDS)
def test_params_tol_is_monotone_in_each_norm(bound):
    base = [0.3, 0.4, 1.0, 1.25]
    t0 = rerank.source_bound_params(base, 2048, bound, 700, 1024)[0]
    for i in (2, 3):
        prev = t0
        for f in (1.0 + 2.0 ** -20, 1.5, 4.0, 1000.0):
            s = list(base); s[i] *= f
            t = rerank.source_bound_params(s, 2048, bound, 700, 1024)[0]
            assert t > prev
            prev = t
    # a coarser pass never gets a smaller tolerance, a longer reduction never a smaller one
    tols = [rerank.source_bound_params(base, 2048, b, 700, 1024)[0] for b in ("f32", "split", "half")]
    assert tols[0] < tols[1] < tols[2]
    assert rerank.source_bound_params(base, 4096, bound, 700, 1024)[0] > t0


# what source_vector computed inline before source_bound_params existed: (stats, d, nrows, Ns_pad) -> bound -> (tol, st, ss, floats)
RECORDED = [
    ((0.4375, 0.5, 1.0000001192092896, 1.000000238418579), 2048, 700, 1024,
     {"half": ("0x1.6231d9a10187cp-8", 256.0, 256.0, 3622076), "split": ("0x1.87c129a0b2075p-10", 256.0, 256.0, 3622076),
      "f32": ("0x1.060806643209dp-11", 0.0, 0.0, 91324)}),
    ((3000.5, 0.001953125, 17000.25, 0.0625), 96, 389, 256,
     {"half": ("0x1.7c091d4122495p+10", 4.0, 256.0, 75013), "split": ("0x1.7aff3840e0c02p+10", 4.0, 256.0, 75013),
      "f32": ("0x1.7afbdb059b6adp+10", 0.0, 0.0, 13093)}),
]


@pytest.mark.parametrize("rec", RECORDED)
def test_params_equal_the_recorded_values(rec):
    stats, d, nrows, Ns_pad, want = rec
    for bound, (tol, st, ss, nws) in want.items():
        assert rerank.source_bound_params(stats, d, bound, nrows, Ns_pad) == (float.fromhex(tol), st, ss, nws)


def test_granule_rule():
    assert ref.granule_of(600, 768, 32) == 8 and ref.granule_of(389, 256, 96) == 4 and ref.granule_of(70, 4608, 64) == 4
    assert ref.granule_of(200, 384, 64) == 4 and ref.granule_of(300, 768, 2048) == 4
    assert ref.granule_of(131072, 13056, 2048) == 8                                  # nrows * Ns_pad / (4 (nrows + Ns_pad)) > d
    assert ref.granule_of(389, 256, 96, {"SSG_SB_GRAN": "8"}) == 8 and ref.granule_of(389, 256, 96, {"SSG_SB_DMA": "0"}) == 8
    for name in ref.CASES:                                                         # where 4 is chosen the doubled table fits the workspace
        c = ref.case(name); nrows, d = c.tgt.shape
        if ref.granule_of(nrows, c.Ns_pad, d) == 4:
            halves = ((nrows + c.Ns_pad) * d + 1) // 2
            assert nrows + c.Ns_pad + nrows * (c.Ns_pad // 4) + 4 + halves <= ref.params(name, "half")[3]


# ------------------------------------------------------------------ the inputs are what they claim
def _two_smallest(D):
    part = np.partition(D, 1, axis=1)
    return part[:, 0], part[:, 1]


@pytest.mark.parametrize("name", ref.CASES)
def test_case_premise(name):
    c = ref.case(name); t = ref.truth(name); D = t["D"]
    tol = ref.params(name, "half")[0]
    assert c.Ns_pad % 128 == 0 and c.Ns_pad >= c.src.shape[0] and c.tgt.shape[1] % 32 == 0 and c.tgt.dtype == c.src.dtype == np.float32
    m1, m2 = _two_smallest(D)
    assert np.all(m2 > m1), "a row without a unique float64 minimum"
    if c.winner is not None:
        assert np.array_equal(D.argmin(axis=1), c.winner)
    if c.kind == "perm":
        assert np.all(m2 - m1 > 2 * tol)
    elif c.kind == "near_ties":
        r = np.arange(D.shape[0])
        near, far = D[r, c.winner], D[r, c.rival]
        assert np.all(c.winner > c.rival) and np.all(c.winner // 256 != c.rival // 256)
        assert np.array_equal(far, m2) and np.all(far - near < tol / 2)
        ulps = ref.half_bits_of(far).astype(int) - ref.half_bits_of(near).astype(int)
        assert np.array_equal(ulps, 1 + r % 3)
        # without the tolerance the answer would be wrong: on some rows the emulated bound orders the two sources the other way round
        e = ref.emulate_half_bound(c.tgt, c.src, *ref.params(name, "half")[1:3])
        assert (e[r, c.rival] < e[r, c.winner]).sum() >= 10
    elif c.kind == "rounding":
        r = np.arange(D.shape[0])
        e = ref.emulate_half_bound(c.tgt, c.src, *ref.params(name, "half")[1:3])
        dup, riv = e[r, c.winner], e[r, c.rival]
        assert np.all(D[r, c.winner] == 0) and np.all(ref.half_bits_of(D[r, c.rival]) > 0) and np.all(c.winner // 8 != c.rival // 8)
        assert np.all(dup > riv) and np.all(riv == e.min(axis=1))                  # the bound prefers the rival
        assert np.all(dup > 0.5 * tol / 2) and np.all(dup < 1.0 * tol / 2)         # excess over the true value, 0
    if name == "perm_d32":
        assert set(c.winner) == set(range(600))                                    # every column is some row's winner
    if name == "wide_refine":
        for G, g in ((4, {0, 511, 512, 1024, 1099}), (8, {0, 511, 512, 549})):
            assert g <= set(c.winner // G)
    if name == "duplicates_and_tiny":
        assert np.all(m1[:50] == 0) and np.all((m1[50:] > 0) & (m1[50:] < 2.0 ** -14))    # half(d^2) is sub-normal
    if name.startswith("ranges"):
        st, ss = ref.params(name, "half")[1:3]
        assert (st, ss) == {"ranges_x100": (256.0, 256.0), "ranges_x3000": (8.0, 8.0), "ranges_x1e-6": (256.0, 256.0),
                            "ranges_zero_tgt": (256.0, 256.0)}[name]
        if name == "ranges_x1e-6":
            assert (np.abs(c.tgt) * st < 2.0 ** -14).mean() > 0.9                         # nine scaled halves in ten are sub-normal


@pytest.mark.parametrize("name", ref.CASES)
def test_emulated_half_bound_keeps_the_contract(name):
    """the one-product bound with exact accumulation is within tol / 2 of the truth for every row and granule: the inputs are feasible"""
    c = ref.case(name); t = ref.truth(name)
    tol, st, ss, _ = ref.params(name, "half")
    e = ref.emulate_half_bound(c.tgt, c.src, st, ss)
    assert np.abs(e - t["D"]).max() <= tol / 2                                     # per distance
    for G in (4, 8):
        eg, padded = ref.granules(e, c.Ns_pad, G)
        tg, _ = t[G]
        assert np.abs(eg[:, ~padded] - tg[:, ~padded]).max() <= tol / 2


@pytest.mark.parametrize("name", [n for n in ref.CASES if n.startswith("ranges")])
def test_stats64_are_upper_bounds(name):
    c = ref.case(name)
    s = ref.stats64(c.tgt, c.src)
    assert all(np.float32(v) == v for v in s)
    exact = (np.abs(c.tgt.astype(np.float64)).max(), np.abs(c.src.astype(np.float64)).max(),
             np.sqrt((c.tgt.astype(np.float64) ** 2).sum(1)).max(), np.sqrt((c.src.astype(np.float64) ** 2).sum(1)).max())
    for got, ex in zip(s, exact):
        assert ex <= got <= ex * (1 + 2.0 ** -23) + 1e-45
