"""float64 restatement (numpy) of the source term's filter-and-refine contract, and the inputs that pin it.

The source term is min_s half(cdist(t, s)^2) (reid/rerank.py:35-40).  csrc/source_term.hip computes it in two passes: a matrix-core
pass writes one bound per target row and granule of G = 4 or 8 sources into a table, a float64 pass re-evaluates the granules whose
bound is within `tol` of the row's smallest.  The contract between them (rerank.source_bound_params): every table entry is within
tol / 2 of the true minimum of its granule.  Shared by tests/test_source_bound_host.py (the inputs are what they claim, on the CPU),
tests/test_gpu_source_bound.py + tests/source_bound_child.py (the kernels keep the contract) and tools/source_bound_errors.py."""
import functools
import math
from collections import namedtuple

import numpy as np

# kind: "perm" = every row has one planted winner, the runner-up is more than 2 tol away; "near_ties" / "rounding" = see the builders;
# "plain" = nothing claimed beyond a unique float64 minimum.  c_entry_only: Ns_pad is no multiple of 256 (source_vector pads to 256).
Case = namedtuple("Case", "name tgt src Ns_pad kind winner rival")


def sqdist(tgt, src):
    """float64 sum_k (x_k - y_k)^2 (the difference form of cdist) -> [nrows, Ns]"""
    t = np.asarray(tgt, np.float64); s = np.asarray(src, np.float64)
    out = np.empty((t.shape[0], s.shape[0]))
    step = max(1, (1 << 23) // max(1, s.shape[0] * s.shape[1]))
    for r in range(0, t.shape[0], step):
        df = t[r:r + step, None, :] - s[None, :, :]
        out[r:r + step] = np.einsum("rsk,rsk->rs", df, df)
    return out


def granules(D, Ns_pad, G):
    """[nrows, Ns] per-source values -> ([nrows, Ns_pad / G] minima over the real sources of every granule, +inf where a granule holds
    none; bool [Ns_pad / G] = granule is fully padded)"""
    nrows, Ns = D.shape
    full = np.full((nrows, Ns_pad), np.inf)
    full[:, :Ns] = D
    return full.reshape(nrows, Ns_pad // G, G).min(axis=2), (np.arange(Ns_pad // G) * G) >= Ns


def granule_min(tgt, src, Ns, G):
    """src [Ns_pad, d] (rows >= Ns are padding) -> (float64 granule minima over s < Ns, fully padded granules)"""
    return granules(sqdist(tgt, np.asarray(src)[:Ns]), np.asarray(src).shape[0], G)


def half_bits_of(D):
    """float64 squared distances -> bits of float16(sqrt(D) ** 2) (np.power(cdist, 2).astype(float16)); monotone in D (D >= 0)"""
    with np.errstate(over="ignore"):
        return (np.sqrt(D) ** 2).astype(np.float16).view(np.uint16)


def rowmin_bits(tgt, src):
    """min_s of the half bits of float16(float64(sqrt(acc)) ** 2), acc = float64 sum_k (x_k - y_k)^2 -> uint16 [nrows]"""
    return half_bits_of(sqdist(tgt, src)).min(axis=1)


def f32_up(v):
    """the smallest float32 >= v"""
    f = np.float32(v)
    return float(f if float(f) >= v else np.nextafter(f, np.float32(np.inf)))


def stats64(tgt, src):
    """(max|x|, max|y|, max target row norm, max source row norm) from float64, as float32 values rounded UP: true upper bounds"""
    t = np.asarray(tgt, np.float64); s = np.asarray(src, np.float64)
    return (f32_up(np.abs(t).max()), f32_up(np.abs(s).max()), f32_up(np.sqrt((t * t).sum(1)).max()), f32_up(np.sqrt((s * s).sum(1)).max()))


def granule_of(nrows, Ns_pad, d, knobs=None):
    """sources per granule of the one-product pass (ssg_source_rowmin_filtered1): 4 when the LDS-DMA kernel runs (SSG_SB_DMA != 0),
    SSG_SB_GRAN is 4 (its default) and the doubled table fits the documented workspace next to the half copies; else 8"""
    knobs = knobs or {}
    dma = int(knobs.get("SSG_SB_DMA", 1)); gran = int(knobs.get("SSG_SB_GRAN", 4))
    doc = nrows + Ns_pad + nrows * (Ns_pad // 8) + (nrows + Ns_pad) * d
    need4 = nrows + Ns_pad + nrows * (Ns_pad // 4) + 4 + ((nrows + Ns_pad) * d + 1) // 2
    return 4 if (dma and gran == 4 and need4 <= doc and nrows * d * 2 < 0x7fffffff and Ns_pad * d * 2 < 0x7fffffff) else 8


def emulate_half_bound(tgt, src, st, ss):
    """the one-product bound without accumulation error: |x|^2 + |y|^2 - 2 <half(x st), half(y ss)> / (st ss) with exact products, a
    float64 sum and float64 norms -> [nrows, Ns]"""
    t = np.asarray(tgt, np.float32); s = np.asarray(src, np.float32)
    th = (t * np.float32(st)).astype(np.float16).astype(np.float64); sh = (s * np.float32(ss)).astype(np.float16).astype(np.float64)
    t64 = t.astype(np.float64); s64 = s.astype(np.float64)
    return (t64 * t64).sum(1)[:, None] + (s64 * s64).sum(1)[None, :] - 2.0 * (th @ sh.T) / (float(st) * float(ss))


def pad_rows(src, Ns_pad):
    out = np.zeros((Ns_pad, src.shape[1]), np.float32)
    out[:src.shape[0]] = src
    return out


# ------------------------------------------------------------------ input builders
def _perm(name, nrows, Ns, d, seed, Ns_pad=None, planted=()):
    """row r's nearest source is column planted[r], or (37 r + 11) % Ns: the source plus a tenth of its length of noise; every other
    source is an independent draw, squared distance about 2"""
    rng = np.random.default_rng(seed)
    src = (rng.standard_normal((Ns, d)) / math.sqrt(d)).astype(np.float32)
    win = np.array([planted[r] if r < len(planted) else (37 * r + 11) % Ns for r in range(nrows)])
    tgt = (src[win] + 0.1 * rng.standard_normal((nrows, d)) / math.sqrt(d)).astype(np.float32)
    return Case(name, tgt, src, Ns_pad or Ns + (-Ns) % 256, "perm", win, None)


def _near_ties():
    """per row two sources whose squared distances are half values 1..3 ulps apart in [2^-6, 2^-5): the farther one in the first
    256-source tile, the nearer one (the later index) in the second or third; every other source is about 2 away"""
    rng = np.random.default_rng(21)
    nrows, Ns, d = 150, 600, 64
    src = (rng.standard_normal((Ns, d)) / math.sqrt(d)).astype(np.float32)
    tgt = (rng.standard_normal((nrows, d)) / math.sqrt(d)).astype(np.float32)
    far = np.arange(nrows); near = 300 + 2 * np.arange(nrows)
    for r in range(nrows):
        hb = 2.0 ** -6 + ((r * 37) % 1000) * 2.0 ** -16
        ha = hb + (1 + r % 3) * 2.0 ** -16
        for col, h in ((far[r], ha), (near[r], hb)):
            u = rng.standard_normal(d); u /= np.linalg.norm(u)
            src[col] = (tgt[r].astype(np.float64) + math.sqrt(h) * u).astype(np.float32)
    return Case("near_ties", tgt, src, 768, "near_ties", near, far)


def _rounding_worst_case(d):
    """the one-product bound's worst case: every coordinate of a target, scaled by 256, sits one float32 step under the midpoint of the
    halves 32 and 32 + 2^-5, so half(256 x) = 32 sign(x) and an exact duplicate gets the bound 2 (|x|^2 - |half x|^2) ~ 2^-9 |x|^2
    instead of 0.  The rival (another granule, another tile) is representable: 2^-3 sign(x), d / 2 coordinates moved out by 2^-8; its
    true squared distance is ~ 2^-11 |x|^2 and its bound is ~ 0.75 of the duplicate's."""
    rng = np.random.default_rng(30 + d)
    nrows, Ns = 64, 400
    mag = np.nextafter(np.float32(32.0 * (1.0 + 2.0 ** -11)), np.float32(0)) / np.float32(256)
    sign = np.where(rng.random((nrows, d)) < 0.5, -1.0, 1.0).astype(np.float32)
    tgt = sign * mag
    src = rng.standard_normal((Ns, d)); src = (src / np.linalg.norm(src, axis=1, keepdims=True) * 0.9 * math.sqrt(d) / 8.0).astype(np.float32)
    dup = np.arange(nrows); rival = 260 + 2 * np.arange(nrows)
    src[dup] = tgt
    z = sign * np.float32(2.0 ** -3)
    for r in range(nrows):
        moved = rng.permutation(d)[: d // 2]
        z[r, moved] += sign[r, moved] * np.float32(2.0 ** -8)
    src[rival] = z
    return Case("rounding_worst_case_d%d" % d, tgt, src, 512, "rounding", dup, rival)


def _duplicates_and_tiny():
    """rows 0..49: an exact duplicate among the sources (distance 0); rows 50..99: a source that differs in one coordinate by 2e-4..1e-3,
    so half(d^2) is sub-normal (4e-8..1e-6)"""
    rng = np.random.default_rng(41)
    nrows, Ns, d = 100, 300, 64
    src = rng.standard_normal((Ns, d)); src = (src / np.linalg.norm(src, axis=1, keepdims=True)).astype(np.float32)
    tgt = rng.standard_normal((nrows, d)); tgt = (tgt / np.linalg.norm(tgt, axis=1, keepdims=True)).astype(np.float32)
    win = (37 * np.arange(nrows) + 11) % Ns
    src[win] = tgt
    for r in range(50, nrows):
        src[win[r], r % d] += np.float32(2e-4 + 8e-4 * (r - 50) / 49.0)
    return Case("duplicates_and_tiny", tgt, src, 512, "plain", win, None)


def _d2048():
    from synth import clustered
    return Case("d2048", clustered(300, 2048, 3), clustered(520, 2048, 4, intra=0.7), 768, "plain", None, None)


RANGES = (("x100", 100.0), ("x3000", 3000.0), ("x1e-6", 1e-6), ("zero_tgt", None))


def _ranges(which):
    """the perm_d96 data times 100 (finite halves), 3000 (scale 8, halves overflow to inf), 1e-6 (the scaled halves are sub-normal), and
    with all-zero targets (max|x| = 0)"""
    base = _perm("perm_d96", 389, 77, 96, 2)
    f = dict(RANGES)[which]
    if f is None:
        return Case("ranges_zero_tgt", np.zeros_like(base.tgt), base.src, base.Ns_pad, "plain", None, None)
    return Case("ranges_" + which, base.tgt * np.float32(f), base.src * np.float32(f), base.Ns_pad, "plain", base.winner, None)


# wide_refine: 1152 granules of 4 (three trips of the refine kernel's 512-granule loops) or 576 of 8 (two); winners planted in granules
# 511 and 512 of either size, at both ends of the last trip, and in the first granule
_WIDE_PLANTED = (2044, 2047, 2048, 2051, 4088, 4095, 4096, 4103, 4399, 4396, 4392, 4100, 0, 3, 7, 2040, 4092)

BUILDERS = {
    "perm_d32": lambda: _perm("perm_d32", 600, 600, 32, 1),
    "perm_d96": lambda: _perm("perm_d96", 389, 77, 96, 2),
    "k_leftovers_d128": lambda: _perm("k_leftovers_d128", 130, 260, 128, 3),
    "k_leftovers_d160": lambda: _perm("k_leftovers_d160", 130, 260, 160, 4),
    "k_leftovers_d192": lambda: _perm("k_leftovers_d192", 130, 260, 192, 5),
    "k_leftovers_d224": lambda: _perm("k_leftovers_d224", 130, 260, 224, 6),
    "wide_refine": lambda: _perm("wide_refine", 70, 4400, 64, 7, planted=_WIDE_PLANTED),
    "half_tile": lambda: _perm("half_tile", 200, 300, 64, 8, Ns_pad=384),
    "d2048": _d2048,
    "near_ties": _near_ties,
    "rounding_worst_case_d32": lambda: _rounding_worst_case(32),
    "rounding_worst_case_d64": lambda: _rounding_worst_case(64),
    "duplicates_and_tiny": _duplicates_and_tiny,
    "ranges_x100": lambda: _ranges("x100"),
    "ranges_x3000": lambda: _ranges("x3000"),
    "ranges_x1e-6": lambda: _ranges("x1e-6"),
    "ranges_zero_tgt": lambda: _ranges("zero_tgt"),
}
CASES = tuple(BUILDERS)
BOUNDS = ("half", "split", "f32")


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    for a in (c.tgt, c.src):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def truth(name):
    """float64 facts of a case, computed once: D [nrows, Ns], the granule minima for G = 4 and 8, the expected rowmin bits, the stats"""
    c = case(name)
    D = sqdist(c.tgt, c.src)
    out = {"D": D, "bits": half_bits_of(D).min(axis=1), "stats": stats64(c.tgt, c.src)}
    for G in (4, 8):
        out[G] = granules(D, c.Ns_pad, G)
    return out


def params(name, bound):
    """(tol, scale_t, scale_s, workspace floats) of a case: rerank.source_bound_params on the float64 stats"""
    from ssg_amd import rerank
    c = case(name)
    return rerank.source_bound_params(truth(name)["stats"], c.tgt.shape[1], bound, c.tgt.shape[0], c.Ns_pad)


def refine_set(table, tol, padded):
    """bool [nrows, ld]: the granules the refine pass re-evaluates, {g : t[g] <= min t + tol} in the kernel's float32 arithmetic"""
    t = np.asarray(table, np.float32)
    bound = (t.min(axis=1) + np.float32(tol)).astype(np.float32)
    return (t <= bound[:, None]) & ~padded[None, :]
