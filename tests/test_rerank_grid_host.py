"""CPU suite: tests/golden/rerank_kgrid.npz (the UNTOUCHED reference over the k1 / k2 / lambda / N range `re_ranking_device`
accepts, tools/make_golden.py --only-kgrid) against the C oracle, and the case table of tests/rerank_grid_ref.py against what it
claims to cover.  tests/test_gpu_rerank_grid.py runs the same cases through the HIP path."""
import numpy as np
import pytest

import rerank_grid_ref as grid


@pytest.fixture(scope="module")
def g(golden):
    return golden(grid.FIXTURE)


def test_fixture_holds_the_table(g):
    assert g["names"].tolist() == [c.name for c in grid.CASES] and len(grid.CASES) == 22
    for c in grid.CASES:
        src, tgt = grid.inputs(c)
        assert src.shape == (c.Ns, c.d) and tgt.shape == (c.N, c.d) and src.dtype == tgt.dtype == np.float32
        assert grid.sha(src) == str(g[c.name + "__sha_src"]) and grid.sha(tgt) == str(g[c.name + "__sha_tgt"]), c.name
        assert (c.name + "__final" in g.files) == (c.N <= grid.FULL_N), c.name


@pytest.mark.parametrize("name", [c.name for c in grid.CASES])
def test_oracle_reproduces_the_reference(name, g, ora):
    """every stage of the oracle equals the reference's (arrays where stored, sha256 otherwise), so do the eps rule and DBSCAN at
    both rho; the case has the property it is in the table for, recomputed from the oracle's stages"""
    c = grid.BY_NAME[name]
    src, tgt, oe, of, st = grid.oracle_run(ora, c)
    rank = g[name + "__rank"]
    assert rank.shape == (c.N, min(c.k1 + 1, c.N)) and np.array_equal(st["rank"][:, :rank.shape[1]], rank), "initial rank"
    for stage, arr in (("euclid", oe), ("V", st["V"]), ("V_qe", st["V_qe"]), ("jaccard", st["jaccard"]), ("final", of)):
        grid.check_stage(g, c, stage, arr, arr)
    grid.check_eps_and_labels(g, c, lambda rho: ora.eps_rule(of, rho), lambda eps: ora.dbscan(of, eps, 4))
    assert grid.check_claims(c, st, of) == int(g[name + "__vmax"])
    if c.k2 == 1:
        assert st["V_qe"] is st["V"] or np.array_equal(st["V_qe"], st["V"])
    if c.lam == 1.0:
        assert not st["jaccard_scaled"].view(np.uint16).any()                    # J' == 0: final_dist is the source term alone
    if c.lam == 0.0:
        assert np.array_equal(of, st["jaccard"].astype(np.float64))             # final_dist is the Jaccard distance itself


def test_table_sits_on_both_sides_of_every_branch(g):
    """the host-side arithmetic that picks the kernels' paths (`grid.derived`, restated from csrc/krecip.hip and rerank.py), over the
    table: at least one case on each side of every parameter-dependent branch of the k-reciprocal stages"""
    dv = {c.name: grid.derived(c) for c in grid.CASES}
    vmax = {c.name: int(g[c.name + "__vmax"]) for c in grid.CASES}
    cases = grid.CASES

    def some(pred):
        return [c.name for c in cases if pred(c, dv[c.name])]

    # kh = round_half_even(k1 / 2) + 1: an odd k1 whose half rounds down (2.5 -> 2), one that rounds up (3.5 -> 4), an even k1
    assert grid.round_half_even_div2(5) == 2 and grid.round_half_even_div2(7) == 4 and grid.round_half_even_div2(63) == 32
    assert [grid.round_half_even_div2(k) for k in range(1, 9)] == [int(np.around(k / 2)) for k in range(1, 9)]
    assert some(lambda c, d: c.k1 % 2 == 1 and c.k1 // 2 % 2 == 0 and c.N > c.k1) and some(lambda c, d: c.k1 % 2 == 1 and c.k1 // 2 % 2 == 1 and c.N > c.k1)
    assert some(lambda c, d: c.k1 % 2 == 0)
    # membership tests on 4-entry vectors (`holds4`: roundup4(kh) <= K) or element by element (`holds`): the latter at k1 <= 2 and
    # where N clamps K
    assert some(lambda c, d: d["holds4"]) and some(lambda c, d: not d["holds4"] and c.k1 <= 2) and some(lambda c, d: not d["holds4"] and d["K"] == c.N)
    assert some(lambda c, d: d["holds4"] and d["kh"] > 16) and some(lambda c, d: d["holds4"] and d["kh"] <= 16)     # one / two trips of its 16-entry loop
    assert all(d["holds4"] == (c.k1 > 2) for c, d in ((c, dv[c.name]) for c in cases) if c.N > max(c.k1 + 1, c.k2))
    # K1 = min(k1 + 1, N, K): all 64 lanes live, fewer, clamped by N
    assert some(lambda c, d: d["K1"] == 64) and some(lambda c, d: d["K1"] < 64) and some(lambda c, d: d["K1"] == c.N < c.k1 + 1)
    assert all(1 <= d["K1"] <= 64 and d["K1"] + d["K1"] * d["kh"] <= d["capV"] for d in dv.values())       # what the k-reciprocal entry point demands
    # np.unique in 64-entry trips and numpy's pairwise sum: fewer than 8 weights, up to 128, above (recursive)
    assert some(lambda c, d: vmax[c.name] < 8) and some(lambda c, d: 8 <= vmax[c.name] <= 64) and some(lambda c, d: 64 < vmax[c.name] <= 128)
    assert some(lambda c, d: vmax[c.name] > 128)
    # query expansion: skipped at k2 == 1; kk = min(k2, N, K) lists: k2 itself, clamped by N; k2 > k1 + 1 widens K; up to 64 lists
    assert some(lambda c, d: d["kk"] is None) and some(lambda c, d: d["kk"] == c.k2) and some(lambda c, d: d["kk"] == c.N < c.k2)
    assert some(lambda c, d: c.k2 > c.k1 + 1 and d["K"] == c.k2) and some(lambda c, d: d["kk"] == 64)
    assert some(lambda c, d: d["kk"] is not None and d["kk"] <= 16) and some(lambda c, d: d["kk"] is not None and d["kk"] > 16)   # 64 / 256 bytes of list lengths
    # the guess protocol: the first guess (64 entries) holds / is met exactly / misses by one / misses widely
    qe = [c for c in cases if c.k2 != 1]
    assert [c.name for c in qe if vmax[c.name] < grid.QE_FIRST_GUESS] and [c.name for c in qe if vmax[c.name] == grid.QE_FIRST_GUESS]
    assert [c.name for c in qe if vmax[c.name] == grid.QE_FIRST_GUESS + 1] and [c.name for c in qe if vmax[c.name] > 2 * grid.QE_FIRST_GUESS]
    # LDS of the query expansion: 4, 2 and 1 rows per workgroup are all reached, on the first guess or on the redo; nothing in the table
    # is beyond one row per workgroup; four rows per workgroup of the corner case would not fit
    waves = set()
    for c in qe:
        kk = dv[c.name]["kk"]
        first = min(grid.QE_FIRST_GUESS, dv[c.name]["capV"])
        waves.add(grid.qe_waves(kk, first))
        if vmax[c.name] > first:
            waves.add(grid.qe_waves(kk, vmax[c.name]))
    assert waves == {4, 2, 1}
    assert 4 * grid.qe_wave_bytes(64, 64) > grid.QE_LDS_LIMIT and 4 * grid.qe_wave_bytes(31, 129) <= grid.QE_LDS_LIMIT < 4 * grid.qe_wave_bytes(32, 129)
    assert grid.qe_wave_bytes(64, 255) == grid.QE_LDS_LIMIT and grid.qe_waves(64, 256) == 0
    # lambda: J' is the Jaccard distance / scaled / zero / negative (half(1 - lambda) has its sign bit set)
    assert some(lambda c, d: d["om_bits"] == 0x3C00) and some(lambda c, d: 0 < d["om_bits"] < 0x3C00) and some(lambda c, d: d["om_bits"] == 0)
    assert some(lambda c, d: d["om_bits"] & 0x8000)


def test_library_picks_the_rows_per_workgroup_the_table_assumes():
    """the Python restatement of the query expansion's LDS arithmetic (`grid.qe_waves`) against the library's own answer, over the
    table's shapes and a sweep of (k2, longest row) up to and beyond the limit; no kernel is launched"""
    from ssg_amd import _lib
    L = _lib.lib()
    for k2 in (2, 6, 16, 17, 31, 32, 33, 48, 63, 64):
        for mx in (1, 2, 28, 63, 64, 65, 75, 129, 169, 255, 256, 511, 512, 1000, 2176):
            assert L.ssg_query_expand_rows_per_group(4000, 64, k2, mx) == grid.qe_waves(k2, mx), (k2, mx)
    assert L.ssg_query_expand_rows_per_group(5, 5, 9, 5) == grid.qe_waves(5, 5) == 4           # kk clamped by N and K
    assert L.ssg_query_expand_rows_per_group(320, 64, 64, 0) == 4                             # an empty table still stages one entry per list
    assert L.ssg_query_expand_rows_per_group(320, 64, 0, 8) == 0
    # the entry point itself refuses what does not fit, before it touches a pointer: 64 lists of 256 entries
    assert L.ssg_query_expand(None, None, None, None, 4000, 0, 10, 64, 64, 2176, 64 * 256, 256, None, None, None, None, None) == -1
    assert b"LDS" in L.ssg_last_error() and b"k2=64 max_nnz=256" in L.ssg_last_error()
