"""Host side of the int8 Gram's tests (no GPU): tests/gram_i8_ref.py is the operation -- against the oracle's cdist restatement, against
values derived by hand, against a second integer route -- its encoder reference keeps the digit and flag rules, and every case of the
table is what the table says it is: the kernel, the pipeline tail and the tile grid it is listed for (gi_use_dma's rule and the tile
arithmetic of ssg_sqdist_self_i8, replayed)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gram_i8_ref as ref  # noqa: E402

SMALL_D2 = [n for n, c in ref.CASES.items() if c.family in ("unit", "wide", "ties")]          # every d2 < 32: U < 2^53
LARGE_D2 = [n for n, c in ref.CASES.items() if c.family in ("coarse", "antipodal", "extreme")]


# ------------------------------------------------------------------ the reference is the operation
@pytest.mark.parametrize("name", SMALL_D2)
def test_reference_equals_the_oracle(name, ora):
    c = ref.CASES[name]
    t = ref.truth(name)
    assert int(t["U"].max()) < (32 << 48)
    if c.family in ("unit", "ties"):
        assert int(t["U"].max()) < (4 << 48)                       # the integer epilogue
    else:
        assert int(t["U"].max()) >= (4 << 48)                      # the float64 branch, still exact
    got = ora.euclid(ref.inputs(name), bool(c.memory_save)).view(np.uint16)
    assert np.array_equal(got, t["D"]), int((got != t["D"]).sum())


def _h(d2):
    """float16(float16(sqrt(d2))^2) of a hand-derived squared distance"""
    with np.errstate(over="ignore"):
        hh = np.float16(np.sqrt(np.float64(d2)))
        return int((hh * hh).view(np.uint16))


@pytest.mark.parametrize("d,b01", [(8192, 0x7800), (16384, 0x7C00)])
def test_antipodal_values_by_hand(d, b01):
    """rows: 0 all +1, 1 all -1, 2 alternating +-1, 3 zeros, 4 all 0.5"""
    D = ref.truth("antipodal_n66_d%d_4dig" % d)["D"]
    assert D[0, 1] == D[1, 0] == b01                                # d2 = 4 d: 32768 -> sqrt 181.02 -> 181 -> 32761 -> 32768; 65536 -> inf
    want = {(0, 2): 2 * d, (1, 2): 2 * d,                           # half the entries differ by 2
            (0, 3): d, (1, 3): d, (2, 3): d,                        # against zeros: the squared norm
            (0, 4): d / 4, (1, 4): 2.25 * d, (2, 4): 1.25 * d, (3, 4): d / 4}
    for (i, j), d2 in want.items():
        assert D[i, j] == D[j, i] == _h(d2), (i, j, hex(D[i, j]), hex(_h(d2)))
    assert _h(2 * 8192) == 0x7400 and _h(8192) == 0x7000           # (powers of 4: the root is exact)
    assert not np.diag(D).any()
    U = ref.truth("antipodal_n66_d%d_4dig" % d)["U"]
    assert int(U[0, 1]) == 4 * d << 48 and (d < 16384 or int(U[0, 1]) == 1 << 64)


@pytest.mark.parametrize("name", [n for n in LARGE_D2 if not ref.CASES[n].memory_save])
def test_reference_equals_the_integer_route(name):
    t = ref.truth(name)
    assert int(t["U"].max()) >= (32 << 48)
    got = ref.dist_bits_direct(t["U"])
    assert np.array_equal(got, t["D"]), int((got != t["D"]).sum())


def test_integer_route_rounds_like_numpy():
    """sqrt_half_direct on every half midpoint square +-1 and on squares of halves: numpy's float64 sqrt -> half agrees below d2 = 4
    (the argument of gram_i8.hip's integer epilogue), and ties go to even"""
    us = []
    for h in list(range(0, 0x4400, 37)) + [1, 2, 0x3FF, 0x400, 0x3BFF, 0x3C00, 0x43FF]:
        m = ref._half_units24(h) + ref._half_units24(h + 1)        # units of 2^-25; m^2 / 4 in units of 2^-48 when m is even
        for u in ((m * m) // 4 - 1, (m * m) // 4, (m * m) // 4 + 1, (m * m + 3) // 4, ref._half_units24(h) ** 2):
            if 0 <= u < (4 << 48):
                us.append(u)
    got = np.array([ref.sqrt_half_direct(u) for u in us], np.uint16)
    want = np.sqrt(np.array(us, np.float64) * 2.0 ** -48).astype(np.float16).view(np.uint16)
    assert np.array_equal(got, want)
    assert ref.sqrt_half_direct(1 << 64) == 0x5C00 and ref.sqrt_half_direct(65520 ** 2 << 48) == 0x7C00 and ref.sqrt_half_direct(4 * 8192 << 48) == 0x59A8


@pytest.mark.parametrize("name", [n for n, c in ref.CASES.items() if c.family == "ties"])
def test_ties_case_sits_on_half_midpoints(name):
    """sqrt(d2) is exactly the midpoint above an odd half (rounds up) and above an even half (rounds down), many times each"""
    U = ref.truth(name)["U"]
    mids = {(ref._half_units24(h) + ref._half_units24(h + 1)) ** 2: h for h in range(0x3800, 0x3C00)}          # 4 U of the midpoints of [0.5, 1)
    lower = [mids[4 * int(u)] for u in U.ravel() if 4 * int(u) in mids]
    odd = sum(h & 1 for h in lower)
    assert odd >= 100 and len(lower) - odd >= 100
    D = ref.truth(name)["D"]
    hh = np.sqrt(U.astype(np.float64) * 2.0 ** -48).astype(np.float16).view(np.uint16)
    on = np.array([4 * int(u) in mids for u in U.ravel()]).reshape(U.shape)
    assert not (hh[on] & 1).any() and np.array_equal(D[on], (hh[on].view(np.float16) ** 2).view(np.uint16))     # ties go to even


def test_no_case_is_ambiguous_or_holds_the_sentinel():
    for name in ref.CASES:
        t = ref.truth(name)                                         # (asserts exact float64(U), no 0xFFFF, the digits fit)
        for i, j in ref.duplicates(name):
            assert t["D"][i, j] == 0 and t["D"][j, i] == 0
        assert np.array_equal(t["D"], t["D"].T) and not np.diag(t["D"]).any()
        assert np.array_equal(t["norms"], (ref.to_int(ref.inputs(name)).astype(object) ** 2).sum(axis=1).astype(np.int64))


# ------------------------------------------------------------------ the encoder reference
@pytest.mark.parametrize("name", ["unit_n65_d33_3dig", "wide_n65_d40_4dig", "extreme_n65_d16384_3dig", "extreme_n65_d16384_4dig", "antipodal_n66_d8192_4dig"])
def test_digits_reconstruct(name):
    dg = ref.truth(name)["digits"]
    assert dg.dtype == np.int8 and dg.shape == ref.inputs(name).shape + (ref.CASES[name].nd,)
    assert np.array_equal(ref.decode(dg), ref.to_int(ref.inputs(name)))


def test_flag_rules():
    def flag(v, nd):
        x = np.zeros((3, 5), np.float32); x[1, 2] = v
        return ref.encode(x, nd)[1]
    assert flag(0.5, 3) and not flag(ref.NEG3, 3) and not flag(ref.POS3, 3)
    assert flag(ref.POS3_NEXT, 3) and flag(-0.50390625, 3)           # the neighbouring halves on either side do not fit
    assert [tuple(ref.encode(np.array([[v]]), 3)[0][0, 0]) for v in (ref.NEG3, ref.POS3)] == [(0, -128, -128), (0, 112, 127)]
    assert not flag(1.0, 4) and not flag(-1.0, 4) and flag(1.0009765625, 4) and flag(-1.0009765625, 4)
    assert flag(np.nan, 3) and flag(np.inf, 3) and flag(np.nan, 4) and flag(-np.inf, 4)
    assert not flag(1.0004, 4)                                       # rounds to the half 1.0
    # the accumulator bound the header states: |T_w| <= NL * d * 2^14 < 2^31 at d = 16384, met with equality by rows of -128 digits
    assert 4 * 16384 * 128 * 128 == 2 ** 30 and 3 * 16384 * 128 * 128 < 2 ** 31


# ------------------------------------------------------------------ the table's claims
@pytest.mark.parametrize("name", list(ref.CASES))
def test_case_takes_the_listed_path(name):
    c = ref.CASES[name]
    r = ref.route(c.N, c.d, c.nd, ref.CONFIGS["default"])
    for k, v in c.claims.items():
        assert r[k] == v, (name, k, r[k], v)
    assert r["symmetric"] and r["sb"] == 6
    assert ref.route(c.N, c.d, c.nd, ref.CONFIGS["nodma"])["path"] == "reg"
    assert c.N <= 833 and c.d <= 16384 and (c.d <= 2048 or c.N <= 66)
    for row0, nrows in c.stripes:
        assert 0 <= row0 and nrows >= 1 and row0 + nrows <= c.N and not ref.route(c.N, c.d, c.nd, {}, row0, nrows)["symmetric"]


def test_table_covers_what_it_is_for():
    # from 256 k blocks on (d > 8160) ssg_sqdist_self_i8 launches the kernels with the modulo-2^64 epilogue: every one of them runs
    wide = {(ref.route(c.N, c.d, c.nd, ref.CONFIGS[cfg])["path"], c.nd, ref.route(c.N, c.d, c.nd, ref.CONFIGS[cfg]).get("kb2"))
            for cfg in ref.CONFIGS for n in ref.cases_of(cfg) for c in [ref.CASES[n]] if (c.d + 31) // 32 >= 256}
    assert wide == {("dma", 3, None), ("reg", 3, 1), ("reg", 3, 2), ("reg", 4, 1)}
    routes = {n: ref.route(c.N, c.d, c.nd, {}) for n, c in ref.CASES.items()}
    dma = [r for r in routes.values() if r["path"] == "dma"]
    assert {r["tail3"] for r in dma} == {0, 1, 2} and {r["tail4"] for r in dma} == {0, 1, 2, 3}
    assert {4, 6, 7, 8, 14}.issubset({r["T"] for r in dma}) and {1, 2}.issubset({r["T"] for r in routes.values()})
    assert any(r["tiles"] > r["used"] for r in dma)                                  # padding tiles of the super-block grid
    # register path: one, two and three stages by default; four and more (even and odd) with SSG_I8_DMA=0; two blocks per stage with KB2
    reg = {ref.route(c.N, c.d, c.nd, ref.CONFIGS["nodma"])["nst"] for c in ref.CASES.values()}
    assert {1, 2, 3, 4, 5, 6, 7, 64}.issubset(reg)
    kb2 = [ref.route(ref.CASES[n].N, ref.CASES[n].d, ref.CASES[n].nd, ref.CONFIGS["nodma_kb2"]) for n in ref.cases_of("nodma_kb2")]
    assert {r["nst"] for r in kb2 if r["kb2"] == 2} >= {1, 2, 3, 32, 256} and any(r["kb2"] == 1 and r["nkb"] % 2 for r in kb2)
    assert ref.route(385, 160, 3, ref.CONFIGS["sb0"])["tiles"] == 28 and ref.route(385, 160, 3, ref.CONFIGS["sb2"])["tiles"] == 40
    # odd N: (row * N + col) & 7 takes every value, so both stores run; d % 32 != 0 together with N % 64 != 0
    assert any(c.N % 2 and routes[n]["path"] == "dma" for n, c in ref.CASES.items())
    assert any(c.N % 64 and c.d % 32 for c in ref.CASES.values()) and any(c.N < 64 and c.d < 32 for c in ref.CASES.values())
    assert any(c.memory_save and c.stripes for c in ref.CASES.values())
    assert ref.cases_of("sb0") == [n for n, c in ref.CASES.items() if not c.big] and ref.cases_of("nodma") == list(ref.CASES)


def test_layout_decoders_invert_the_documented_layouts():
    """decode_E against an index-by-index restatement of the two layouts"""
    n, d, nd = 70, 40, 3
    nkb = 2
    dg = np.random.default_rng(0).integers(-128, 128, (n, nkb * 32, nd)).astype(np.int8)
    for planar in (False, True):
        E = np.zeros(ref.encoded_bytes(n, d, nd), np.int8)
        for row in range(n):
            for k in range(nkb * 32):
                for L in range(nd):
                    if planar:
                        off = (((row // 64) * nkb + k // 32) * nd + L) * 64 * 32 + (row % 64) * 32 + k % 32
                    else:
                        off = ((((row // 64) * nkb + k // 32) * 64 + row % 64) * nd + L) * 32 + k % 32
                    E[off] = dg[row, k, L]
        assert np.array_equal(ref.decode_E(E, n, d, nd, planar), dg)
