"""Exact reference of the int8 Gram (csrc/gram_i8.hip) and the case table of tests/test_gram_i8_host.py / tests/test_gpu_gram_i8.py.

The operation (reid/rerank.py:33,61-62): feat = x.astype(float16); D = float16(float16(cdist(feat, feat))^2), or with MemorySave (:49-59)
D = float16(cdist^2).  For |feat| <= 1, X = feat * 2^24 is an integer and U = |Xi|^2 + |Xj|^2 - 2<Xi, Xj> = d2 * 2^48 is an integer in
[0, 2^64].  This module computes U EXACTLY and without the kernel's radix-256 digits: X is split into two 13-bit limbs, the three limb
products are float64 matmuls whose every partial sum is an integer below 2^53, and the limbs are combined in int64 (norms below 2^60) or in
Python ints.  The epilogue is the reference's, in numpy: s = sqrt(float64(U) * 2^-48), hh = float16(s), D = float16(hh * hh).

float64(U) rounds when U >= 2^53 (d2 >= 32) has more than 53 significant bits -- and scipy's running sum then rounds elsewhere.  So that
the reference never has two defensible answers, every input is built to keep U exactly representable; `truth` asserts it."""
import functools
import zlib
from collections import namedtuple

import numpy as np

GI_T = 64                                    # tile edge and panel height of the kernel
SENTINEL = 0xFFFF                            # what the GPU test pre-fills D with: a NaN pattern the reference never produces
NEG3 = -0.501953125                          # smallest half that fits 3 balanced digits: X = -0x808000 -> (0, -128, -128)
POS3 = 0.497802734375                        # largest half that fits 3 balanced digits:  X =  0x7F7000 -> (0,  112,  127)
POS3_NEXT = 0.498046875                      # the next half above POS3 (X = 0x7F8000 > 127 * 65793): needs a fourth digit

Case = namedtuple("Case", "name family N d nd memory_save stripes big claims")


# ------------------------------------------------------------------ the case table
def _stripes(N):
    """(row0, nrows): starts at 0 but not the whole matrix / unaligned start / exactly one panel / the last row / crosses the last panel of
    N = 385.  (37, 200) is cut to the rows that exist when N < 237."""
    out = [(0, 100), (37, min(200, N - 37)), (64, 64), (N - 1, 1)]
    if 321 + 64 <= N:
        out.append((321, 64))
    return tuple(out)


def _build_table():
    cases = {}

    def add(family, N, d, nd, ms=0, stripes=(), big=False, **claims):
        name = "%s_n%d_d%d_%ddig%s" % (family, N, d, nd, "_ms" if ms else "")
        assert name not in cases
        cases[name] = Case(name, family, N, d, nd, ms, tuple(stripes), big, claims)

    # register path (fewer than 4 k blocks); d = 1, 31, 33 end in a partial k block; 1, 2 (d = 33), 3 (d = 96) stages
    for N in (1, 2, 63, 64, 65, 127):
        for d in (1, 31, 33, 96):
            add("unit", N, d, 3, path="reg", nkb=(d + 31) // 32, T=(N + 63) // 64)
    # LDS-DMA path: tails 1, 2, 0, 1 with three stages and 0, 1, 2, 3 with four; T = 4, 6 (one super-block), 7 and 8 (two super-blocks
    # per edge, padding tiles), 14 (three); odd N: the rows alternate between the vector and the scalar store
    for N, T, nb in ((200, 4, 1), (384, 6, 1), (385, 7, 2), (449, 8, 2), (833, 14, 3)):
        for d, t3, t4 in ((128, 1, 0), (160, 2, 1), (192, 0, 2), (224, 1, 3)):
            add("unit", N, d, 3, stripes=_stripes(N) if (N, d) == (385, 160) else (), path="dma", nkb=d // 32, tail3=t3, tail4=t4, T=T, nb=nb)
    add("unit", 449, 96, 3, stripes=_stripes(449), path="reg", nkb=3, T=8, nb=2)
    add("unit", 130, 2048, 3, path="dma", nkb=64, tail3=1, tail4=0, T=3, nb=1)          # the workload's width
    # exact ties of half(sqrt(d2)): the only inputs on which the midpoint comparisons of the integer epilogue decide alone (see `inputs`)
    add("ties", 66, 33, 3, path="reg", nkb=2, T=2)
    add("ties", 66, 128, 3, path="dma", nkb=4, tail3=1, tail4=0, T=2)
    add("wide", 65, 40, 4, path="reg", nkb=2, T=2)
    add("wide", 200, 64, 4, stripes=_stripes(200), path="reg", nkb=2, T=4)
    add("wide", 385, 160, 4, path="reg", nkb=5, T=7)
    add("coarse", 130, 224, 4, path="reg", nkb=7, T=3)
    add("coarse", 65, 16384, 4, big=True, path="reg", nkb=512, T=2)
    add("antipodal", 66, 8192, 4, big=True, path="reg", nkb=256, T=2)
    add("antipodal", 66, 16384, 4, big=True, path="reg", nkb=512, T=2)
    add("extreme", 65, 16384, 3, big=True, path="dma", nkb=512, tail3=2, tail4=0, T=2)
    add("extreme", 65, 16384, 4, big=True, path="reg", nkb=512, T=2)
    add("unit", 385, 160, 3, ms=1, stripes=_stripes(385), path="dma", nkb=5, tail3=2, tail4=1, T=7, nb=2)
    add("wide", 200, 64, 4, ms=1, path="reg", nkb=2, T=4)
    add("coarse", 130, 224, 4, ms=1, path="reg", nkb=7, T=3)
    return cases


CASES = _build_table()
# the five child processes of the GPU test (the three knobs are read once per process)
CONFIGS = {"default": {}, "nodma": {"SSG_I8_DMA": "0"}, "nodma_kb2": {"SSG_I8_DMA": "0", "SSG_I8_KB2": "2"}, "sb0": {"SSG_I8_SB": "0"},
           "sb2": {"SSG_I8_SB": "2"}}
BIG_CONFIGS = ("default", "nodma")           # the d = 8192 and d = 16384 cases run in these two only,
BIG_EXTRA = {"nodma_kb2": ("extreme_n65_d16384_3dig",)}       # but for the one that reaches the two-blocks-per-stage kernel of d >= 8192


def cases_of(config):
    return [n for n, c in CASES.items() if not c.big or config in BIG_CONFIGS or n in BIG_EXTRA.get(config, ())]


# ------------------------------------------------------------------ inputs
def _coarse(rng, N, d):
    return rng.integers(-2, 3, (N, d)).astype(np.float32) * np.float32(0.5)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """float32 [N, d] of a case (seeded by its name); read-only"""
    c = CASES[name]
    N, d = c.N, c.d
    rng = np.random.default_rng(zlib.crc32(("%s/%d/%d" % (c.family, N, d)).encode()))          # (the two digit counts / memory_save share the input)
    if c.family in ("unit", "wide"):
        x = rng.standard_normal((N, d))
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        if c.family == "unit":
            # narrow rows (d = 1: every normalised entry is +-1) do not fit 3 digits: the whole matrix is scaled down then, so the rows
            # still share ONE norm <= 1 and every d2 stays below 4
            x *= min(1.0, 0.49 / np.abs(x).max())
            x = x.astype(np.float32)
            if N > 2:
                x[N - 2] = 0
        else:
            x = np.clip(2.0 * x, -1.0, 1.0).astype(np.float32)
            x[0, 0] = 1.0; x[1, 0] = -1.0
    elif c.family == "ties":
        # one live coordinate, +(0.25 + i 2^-12) on even rows and -(0.25 + i 2^-12) on odd ones: an even and an odd row are exactly
        # 0.5 + (i + j) 2^-12 apart, i + j odd -- the midpoint between two halves of [0.5, 1), lower neighbours of both parities.  The
        # float32 candidate root is right everywhere else, so only here does the result hang on the comparison with the midpoint squares.
        x = np.zeros((N, d), np.float32)
        i = np.arange(N)
        x[:, 0] = np.where(i % 2 == 0, 1.0, -1.0) * (0.25 + i * 2.0 ** -12)
    elif c.family == "coarse":
        x = _coarse(rng, N, d)
    elif c.family == "antipodal":
        x = _coarse(rng, N, d)
        x[0] = 1.0; x[1] = -1.0; x[2] = np.where(np.arange(d) % 2 == 0, 1.0, -1.0); x[3] = 0.0; x[4] = 0.5
    elif c.family == "extreme":
        x = np.where(rng.integers(0, 2, (N, d)) == 0, NEG3, POS3).astype(np.float32)         # mixed-sign rows
        x[0::4] = NEG3; x[1::4] = POS3
    else:
        raise KeyError(c.family)
    if N > 7 and c.family in ("unit", "wide", "coarse"):
        x[7] = x[3]                                                                      # an exact zero off the diagonal
    x = np.ascontiguousarray(x, np.float32)
    x.setflags(write=False)
    return x


def duplicates(name):
    return ((7, 3),) if CASES[name].N > 7 and CASES[name].family in ("unit", "wide", "coarse") else ()


# ------------------------------------------------------------------ exact arithmetic
def to_int(x):
    """X = float16(x) * 2^24 as exact int64 (|float16(x)| <= 1, finite)"""
    h = np.asarray(x, np.float32).astype(np.float16).astype(np.float64)
    assert np.isfinite(h).all() and np.abs(h).max(initial=0.0) <= 1.0
    Xf = h * 16777216.0
    X = Xf.astype(np.int64)
    assert np.array_equal(X.astype(np.float64), Xf)
    return X


def exact_gram(X):
    """<Xi, Xj> as exact int64 (|.| <= d * 2^48 <= 2^62): limbs X = hi * 2^13 + lo, 0 <= lo < 2^13, |hi| <= 2^11"""
    lo = (X & 8191).astype(np.float64); hi = (X >> 13).astype(np.float64)
    assert X.shape[1] <= 16384 and np.abs(hi).max(initial=0.0) <= 2048
    ll, lh, hh = lo @ lo.T, lo @ hi.T, hi @ hi.T                     # every partial sum is an integer of at most 2^14 * 2^26 = 2^40
    for m in (ll, lh, hh):
        assert np.abs(m).max(initial=0.0) < 2.0 ** 53 and np.array_equal(m, np.rint(m))
    return (hh.astype(np.int64) << 26) + ((lh + lh.T).astype(np.int64) << 13) + ll.astype(np.int64)


def exact_U(X):
    """(U, norms): U[i, j] = |Xi|^2 + |Xj|^2 - 2<Xi, Xj> exactly, 0 on the diagonal -- int64 when it provably fits, else Python ints"""
    G = exact_gram(X)
    n = np.diag(G).copy()
    if int(n.max()) < 2 ** 60:                                       # U <= 4 max(n) < 2^62
        U = n[:, None] + n[None, :] - 2 * G
    else:
        no, Go = n.astype(object), G.astype(object)
        U = no[:, None] + no[None, :] - 2 * Go
    np.fill_diagonal(U, 0)
    return U, n


def U_to_f64(U):
    """(float64(U) round-to-nearest-even, whether every conversion was exact)"""
    if U.dtype == object:
        Uf = U.astype(np.float64)                                    # PyLong -> double: correctly rounded
        exact = all(int(f) == u for f, u in zip(Uf.ravel().tolist(), U.ravel().tolist()))
    else:
        Uf = U.astype(np.float64)
        exact = bool(np.array_equal(Uf.astype(np.int64), U))         # (U < 2^62: the way back cannot overflow)
    return Uf, exact


def epilogue(Uf, memory_save):
    """reid/rerank.py:61-62 (MemorySave: :49-59) on float64(U) -> half bits"""
    with np.errstate(over="ignore"):
        s = np.sqrt(Uf * 2.0 ** -48)
        if memory_save:
            D = (s * s).astype(np.float16)
        else:
            hh = s.astype(np.float16)
            D = hh * hh                                              # numpy's half product: float32 (exact) then one rounding
    return np.ascontiguousarray(D).view(np.uint16)


def dist_bits(x, memory_save=False):
    """half bits of the whole [N, N] matrix of any |float16(x)| <= 1 input + (U, norms, exact)"""
    U, n = exact_U(to_int(x))
    assert (U >= 0).all()
    Uf, exact = U_to_f64(U)
    return epilogue(Uf, memory_save), U, n, exact


@functools.lru_cache(maxsize=None)
def truth(name):
    """dict: D (half bits [N, N]), rowmax (uint32 [N]), norms (int64 [N]), U, digits (int8 [N, d, nd]); computed once, read-only"""
    c = CASES[name]
    D, U, n, exact = dist_bits(inputs(name), bool(c.memory_save))
    assert exact, "%s: a U is not representable in float64 -- the reference would be ambiguous" % name
    assert not (D == SENTINEL).any() and not (D & 0x8000).any()
    dg, bad = encode(inputs(name), c.nd)
    assert not bad, "%s does not fit %d digits" % (name, c.nd)
    out = {"D": D, "rowmax": D.max(axis=1).astype(np.uint32), "norms": n, "U": U, "digits": dg}
    for v in out.values():
        v.setflags(write=False)
    return out


# ------------------------------------------------------------------ the encoder
def encode(x, nd):
    """(balanced radix-256 digits int8 [N, d, nd] of X, flag).  The flag: a half-rounded value is NaN, beyond 1 in magnitude, or does not
    fit nd digits (the digits of such a value are not specified)."""
    h = np.asarray(x, np.float32).astype(np.float16).astype(np.float64)
    bad = ~(np.abs(h) <= 1.0)
    r = np.where(bad, 0.0, h * 16777216.0).astype(np.int64)
    dg = np.zeros(h.shape + (nd,), np.int8)
    for L in range(nd):
        t = ((r + 128) & 255) - 128
        dg[..., L] = t
        r = (r - t) >> 8
    return dg, bool(bad.any() or (r != 0).any())


def decode(dg):
    """int64 value of balanced digits [..., nd]"""
    return sum(dg[..., L].astype(np.int64) << (8 * L) for L in range(dg.shape[-1]))


def decode_E(E, n, d, nd, planar):
    """digits int8 [n, nkb * 32, nd] out of the encoder's table, by the layouts of the header comment of gram_i8_encode_kernel:
    panel-major [row / 64][k block][row % 64][digit][32 k], planar [row / 64][k block][digit][row % 64][32 k]"""
    nkb = (d + 31) // 32; P = (n + GI_T - 1) // GI_T
    E = np.asarray(E).view(np.int8).reshape(-1)
    assert E.size == P * GI_T * nkb * 32 * nd
    if planar:
        a = E.reshape(P, nkb, nd, GI_T, 32).transpose(0, 3, 1, 4, 2)
    else:
        a = E.reshape(P, nkb, GI_T, nd, 32).transpose(0, 2, 1, 4, 3)
    return a.reshape(P * GI_T, nkb * 32, nd)[:n]


# ------------------------------------------------------------------ which code a call runs (ssg_sqdist_self_i8 / gi_use_dma / gi_pick_tile, replayed)
def encoded_bytes(N, d, nd):
    return (N + GI_T - 1) // GI_T * GI_T * ((d + 31) // 32) * 32 * nd


def use_dma(N, d, nd, env):
    return int(env.get("SSG_I8_DMA", "1")) != 0 and nd == 3 and encoded_bytes(N, d, nd) < 0xfffffff0 and (d + 31) // 32 >= 4


def route(N, d, nd, env, row0=0, nrows=None):
    """path 'dma' / 'reg', k blocks, per-stage k blocks, DMA tails, tile grid of one ssg_sqdist_self_i8 call under the knobs `env`"""
    nrows = N if nrows is None else nrows
    nkb = (d + 31) // 32
    T = (N + GI_T - 1) // GI_T
    symmetric = row0 == 0 and nrows == N
    sbv = int(env.get("SSG_I8_SB", "6"))
    sb = (0 if sbv < 0 or sbv > 64 else sbv) if symmetric else 0
    nb = (T + sb - 1) // sb if sb else 0
    r = {"nkb": nkb, "T": T, "symmetric": symmetric, "sb": sb, "nb": nb,
         "tiles": (nb * (nb + 1) // 2 * sb * sb if sb else T * (T + 1) // 2) if symmetric else (nrows + GI_T - 1) // GI_T * T}
    r["used"] = T * (T + 1) // 2 if symmetric else r["tiles"]
    if use_dma(N, d, nd, env):
        r.update(path="dma", tail3=nkb % 3, tail4=nkb % 4)
    else:
        kb2 = 2 if (nd == 3 and int(env.get("SSG_I8_KB2", "1")) == 2 and nkb % 2 == 0) else 1
        r.update(path="reg", kb2=kb2, nst=nkb // kb2)
    return r


# ------------------------------------------------------------------ a second route to half(sqrt(U * 2^-48)): integers only
def _half_units24(h):
    e, m = h >> 10, h & 1023
    return m if e == 0 else (1024 | m) << (e - 1)


_MID = None


def sqrt_half_direct(U):
    """half bits of the DIRECT round-to-nearest-even of sqrt(U * 2^-48), U a Python int: the count of half midpoints below the root,
    by math.isqrt and integer squares alone"""
    import bisect
    import math
    global _MID
    if _MID is None:                                        # midpoint between half h and h + 1 in units of 2^-25; above 65504: 65520
        _MID = [_half_units24(h) + (_half_units24(h + 1) if h + 1 < 0x7C00 else 65536 << 24) for h in range(0x7C00)]
    U4 = 4 * int(U)                                         # (2 sqrt(U)) in units of 2^-25 against the midpoints
    r = math.isqrt(U4)
    h = bisect.bisect_left(_MID, r)                         # midpoints strictly below floor(2 sqrt U)
    if h < 0x7C00 and _MID[h] == r:
        if r * r < U4 or (h & 1):                           # above the midpoint, or exactly on it with an odd lower neighbour
            h += 1
    return h


def dist_bits_direct(U):
    """the matrix by the integer route (Python ints; the final half product is numpy's, one exact-product rounding)"""
    out = np.empty(U.shape, np.uint16)
    flat = out.reshape(-1)
    with np.errstate(over="ignore"):
        for i, u in enumerate(U.ravel().tolist()):
            hh = np.uint16(sqrt_half_direct(u)).view(np.float16)
            flat[i] = (hh * hh).view(np.uint16)
    return out
