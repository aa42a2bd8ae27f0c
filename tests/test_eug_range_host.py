"""CPU half of the whole-range tests of the SSG++ label step: the restatement of tests/eug_ref.py against the INSTALLED numpy at every
width of D_EDGE (a numpy that sums in another order fails here, with a clear message, and not as a GPU mismatch); that the widths
fill the evaluation stack and that their data tells numpy's order from a naive one; the scalar rules of csrc/eug.hip -- the leaf
program for EVERY accepted width, the np.argmin order, the np.argsort key -- compiled for x86 from the SAME SOURCE TEXT
(tools/hostexec/eug_rules.cpp); and the refusals that are made before any launch."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import eug_ref as ref

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "self-similarity-grouping_amd", "csrc", "eug.hip")
RULES = ("eug_build_program", "eug_better", "eug_score_key")


def u32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def numpy_norms(u, l):
    with np.errstate(all="ignore"):
        return np.stack([np.linalg.norm(l - x, axis=1) for x in u])


@pytest.fixture(scope="module")
def width_data():
    """d -> (u, l, numpy's [Nu, Nl] norms) of the GPU suite's width cases, computed once"""
    cache = {}

    def get(d, wide=False):
        if (d, wide) not in cache:
            u, l = ref.features(ref.NU, ref.NL, d, ref.width_seed(d), wide=wide)
            cache[d, wide] = (u, l, numpy_norms(u, l))
        return cache[d, wide]
    return get


@pytest.mark.parametrize("d", ref.D_EDGE)
def test_restatement_is_the_installed_numpy(width_data, d):
    """pairwise_norm == np.linalg.norm(l - u, axis=1) bit for bit on all Nu x Nl pairs of the GPU suite's data.  If this fails the
    installed numpy reduces in another order than the one csrc/eug.hip replays (8 accumulators, leaves of at most 128, split at
    n/2 & ~7, chunks of 8192): numpy is right; restate it here and in eug_nn_kernel"""
    for wide in ([False, True] if d in ref.D_WIDE else [False]):
        u, l, want = width_data(d, wide)
        got, depth = ref.pairwise_norm(l[None, :, :], u[:, None, :])
        assert got.dtype == F32 and got.shape == (ref.NU, ref.NL)
        bad = np.flatnonzero(u32(got) != u32(want))
        assert bad.size == 0, ("numpy %s sums d = %d in another order than the restatement: %d of %d pairs differ, first at %d"
                               % (np.__version__, d, bad.size, want.size, bad[0]))
        assert 1 <= depth <= ref.MAXD
    # a single labelled row and a single pair reduce the same way
    u, l, want = width_data(d)
    assert np.array_equal(u32(np.linalg.norm(l[:1] - u[0], axis=1)), u32(want[0, :1]))
    assert np.array_equal(u32(ref.nn_ref(u[:2], l)[1]), u32(want[:2].min(axis=1)))


def test_stack_depth_of_the_width_list():
    """the deepest evaluation stack is EUG_MAXD = 8 at 8185, 8191, 16383 and 32767 and never more: the list really fills the stack.
    (The depth depends on the width alone.)"""
    depth = {d: ref.pairwise_norm(np.ones((1, d), F32), np.zeros(d, F32))[1] for d in ref.D_EDGE}
    assert all(depth[d] == ref.MAXD for d in ref.D_FULL_STACK), depth
    assert max(depth.values()) == ref.MAXD and min(depth.values()) == 1
    assert depth[2047] == 6 and depth[4103] == 7 and depth[8192] == 7 and depth[8184] == 7 and depth[32768] == 7
    assert {d for d in ref.D_EDGE if d % 8} and {d for d in ref.D_EDGE if d < 8} and {d for d in ref.D_EDGE if 0 < d % ref.CHUNK < 8 and d > ref.CHUNK}
    assert {-(-d // ref.CHUNK) for d in ref.D_EDGE} == {1, 2, 3, 4}


@pytest.mark.parametrize("d", [d for d in ref.D_EDGE if d >= 16])
def test_data_tells_numpy_s_order_from_a_naive_sum(width_data, d):
    """a left-to-right float32 sum of the same squares differs from numpy in at least one pair, and in at least one row MINIMUM --
    which is what the GPU suite compares -- so a kernel that summed in another order would be seen.  A condition on the data: if a
    width fails it, change eug_ref.width_seed, not the condition"""
    for wide in ([False, True] if d in ref.D_WIDE else [False]):
        u, l, want = width_data(d, wide)
        naive = ref.naive_norm(l[None, :, :], u[:, None, :])
        assert (u32(naive) != u32(want)).any()
        assert (u32(naive.min(axis=1)) != u32(want.min(axis=1))).any()
        if wide:                                  # more than the last bit
            assert (np.abs(naive.astype(np.float64) - want) > 4 * np.spacing(want)).any()


# ------------------------------------------------------------------ the scalar rules of eug.hip, compiled for x86


def cut_rules():
    """the EUG_* constants and the three rule functions, as they stand in eug.hip"""
    lines = open(HIP).read().split("\n")
    out = [ln for ln in lines if ln.startswith("constexpr int EUG_")]
    assert len(out) >= 6
    for name in RULES:
        start = [i for i, ln in enumerate(lines) if ln.startswith("__device__") and " " + name + "(" in ln]
        assert len(start) == 1, name
        end = next(i for i in range(start[0], len(lines)) if lines[i] == "}")
        out += lines[start[0]:end + 1]
    return "\n".join(out) + "\n"


@pytest.fixture(scope="module")
def hx(tmp_path_factory):
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else (shutil.which("g++") or shutil.which("c++"))
    assert cxx, "no C++ compiler"
    d = tmp_path_factory.mktemp("hx_eug")
    (d / "eug_cut.inc").write_text(cut_rules())
    so = str(d / "libhx_eug.so")
    r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I" + str(d), "-o", so,
                        os.path.join(ROOT, "tools", "hostexec", "eug_rules.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # the kernels use the rules they publish
    text = open(HIP).read()
    assert text.count("eug_build_program(") == 2 and text.count("eug_better(") >= 5 and text.count("eug_score_key(") == 3
    L = ctypes.CDLL(so)
    L.hx_eug_better.argtypes = [ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.c_int]
    L.hx_eug_fold.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    L.hx_eug_score_key.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    L.hx_eug_build_program.argtypes = [ctypes.c_int, ctypes.c_void_p]
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def consts(hx):
    c = np.zeros(7, np.int32)
    hx.hx_eug_constants(_p(c))
    return dict(zip(("TU", "TL", "KW", "MAXD", "CHUNK", "MAXLEAF", "CM_CHUNKS"), c.tolist()))


def program(hx, d, buf=None):
    buf = np.full((d + 1, 4), -7, np.int32) if buf is None else buf
    n = hx.hx_eug_build_program(d, _p(buf))
    return buf[:n]


def test_constants_are_what_the_cases_assume(hx, consts):
    assert consts == dict(TU=ref.TU, TL=ref.TL, KW=ref.PW_BLOCK, MAXD=ref.MAXD, CHUNK=ref.CHUNK, MAXLEAF=512, CM_CHUNKS=64)
    assert consts["MAXLEAF"] * 64 == max(ref.D_EDGE) == 32768          # the accepted maximum of ssg_eug_nn_f32


def test_leaf_program_of_every_accepted_width(hx, consts):
    """for EVERY d in 1..32768: the leaves tile [0, d) in ascending order without a gap, every length is in 1..128, the chunk flag
    stands exactly on the last leaf before each multiple of 8192 and on the last leaf, the program fits EUG_MAXLEAF, no chunk needs
    more than EUG_MAXD live stack entries (a push per leaf, `pops` pops after it), no pop finds fewer than two entries, and one
    entry is left at each chunk end"""
    dmax = consts["MAXLEAF"] * 64
    buf = np.empty((dmax + 1, 4), np.int32)
    peak_of = np.zeros(dmax + 1, np.int64)
    for d in range(1, dmax + 1):
        buf[:consts["MAXLEAF"] + 2] = -7
        p = program(hx, d, buf)
        n = len(p)
        assert 1 <= n <= consts["MAXLEAF"], d
        start, length, pops, flag = (p[:, k].astype(np.int64) for k in range(4))
        stop = start + length
        assert start[0] == 0 and stop[-1] == d and np.array_equal(start[1:], stop[:-1]), d
        assert length.min() >= 1 and length.max() <= consts["KW"], d
        assert np.array_equal(flag, ((stop % consts["CHUNK"] == 0) | (stop == d)).astype(np.int64)), d
        assert pops.min() >= 0, d
        # live entries, counted within each chunk (a chunk end hands its one entry to the running sum)
        net = np.cumsum(1 - pops)                                         # after each leaf and its pops, over the whole program
        ends = np.flatnonzero(flag)
        base = np.zeros(n, np.int64)                                      # what the earlier chunks left behind
        base[ends[:-1] + 1] = 1
        live_after = net - np.cumsum(base)
        assert np.array_equal(live_after[ends], np.ones(len(ends), np.int64)), d
        assert live_after.min() >= 1, d                                   # every pop found two entries
        peak_of[d] = (live_after + pops).max()                            # right after the push
        assert peak_of[d] <= consts["MAXD"], d
    assert peak_of[1:].max() == consts["MAXD"]
    assert all(peak_of[d] == consts["MAXD"] for d in ref.D_FULL_STACK) and all(peak_of[d] == consts["MAXD"] for d in range(8185, 8192))
    assert peak_of[8192] == 7 and peak_of[2047] == 6 and peak_of[4103] == 7 and peak_of[128] == 1


@pytest.mark.parametrize("d", ref.D_EDGE)
def test_leaf_program_executed_is_the_restatement(hx, width_data, d):
    """the kernel's program run with eug_ref's leaf function, the kernel's push / pop / chunk rule: pairwise_norm, hence numpy, bit
    for bit, with the stack depth the restatement counted"""
    u, l, want = width_data(d)
    got, peak = ref.run_program(program(hx, d), l[None, :16, :], u[:4, None, :])
    assert np.array_equal(u32(got), u32(want[:4, :16]))
    assert peak == ref.pairwise_norm(l[:1], u[0])[1]


SPECIALS = [np.nan, -np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf]


def test_better_is_np_argmin(hx):
    """eug_better orders every pair of {NaN, -inf, -1, -0.0, +0.0, denormal, 1, inf} x two indices the way np.argmin of the
    two-element array does (the first NaN wins, else the smaller value, else the lower index; -0.0 == +0.0), also against the
    kernel's start value; folded over an array in any order it is np.argmin"""
    for v in SPECIALS:
        for m in SPECIALS:
            for i, j in ((3, 9), (9, 3), (0, 0x7ffffffe), (64, 0)):
                arr = np.array([v, m] if i < j else [m, v], F32)
                v_wins = int(np.argmin(arr)) == (0 if i < j else 1)
                assert bool(hx.hx_eug_better(v, i, m, j)) == v_wins, (v, i, m, j)
        # against (+inf, 0x7fffffff), the value every lane starts from: any real entry wins, +inf included
        assert hx.hx_eug_better(v, 5, np.inf, 0x7fffffff) == 1
    rng = np.random.default_rng(2)
    pool = np.array(SPECIALS + [0.25, 0.25, 0.5], F32)
    for trial in range(300):
        n = int(rng.integers(1, 70))
        vals = rng.choice(pool[1:] if trial % 3 else pool, n).astype(F32)
        for order in (np.arange(n), np.arange(n)[::-1], rng.permutation(n)):
            best = ctypes.c_float()
            order = np.ascontiguousarray(order, dtype=np.int32)
            got = hx.hx_eug_fold(_p(vals), _p(order), n, ctypes.byref(best))
            want = int(np.argmin(vals))
            assert got == want, (trial, vals)
            assert np.isnan(vals[want]) if np.isnan(best.value) else u32([best.value])[0] == u32(vals)[want]


def test_score_key_is_stable_argsort_of_minus_score(hx):
    """taking the largest eug_score_key first, equal keys by index, is np.argsort(-x, kind="stable") on the specials as float64:
    larger score first, -0.0 == +0.0, NaN (of either sign) last"""
    rng = np.random.default_rng(3)
    pool = np.array(SPECIALS + [5e-324, -5e-324, 1e300, -1e300, np.float64(np.float32(1e-45)), 0.5, -np.nan], np.float64)
    for n in (len(pool), 1, 2, 257, 4000):
        x = pool.copy() if n == len(pool) else rng.choice(pool, n)
        key = np.empty(n, np.uint64)
        hx.hx_eug_score_key(_p(x), n, _p(key))
        assert np.array_equal(np.argsort(~key, kind="stable"), np.argsort(-x, kind="stable"))
        assert np.array_equal(key == 0, np.isnan(x)) and np.array_equal(key[x == 0], np.full((x == 0).sum(), 1 << 63, np.uint64))


# ------------------------------------------------------------------ refusals, before any launch


def test_entry_points_refuse_out_of_range_arguments_without_a_gpu():
    """the C layer with NULL pointers: d = 32769 is refused with the range in the message, d = 32768 is accepted (it gets as far as
    the buffer check); k outside [0, n]; empty matrices"""
    from ssg_amd import _lib
    L = _lib.lib()
    ns = L.ssg_eug_nn_splits(ref.NU, ref.NL)
    assert ns == 3 and ref.structure(ref.NU, ref.NL, ns) == (2, 3, 1)
    none = (None,) * 6
    assert L.ssg_eug_nn_f32(None, ref.NU, None, ref.NL, 32769, None, ns, *none, None) == -1
    assert b"0 < d <= 32768" in L.ssg_last_error()
    assert L.ssg_eug_nn_f32(None, ref.NU, None, ref.NL, 32768, None, ns, *none, None) == -1
    assert b"missing buffer" in L.ssg_last_error()
    assert L.ssg_eug_nn_f32(None, ref.NU, None, ref.NL, 0, None, ns, *none, None) == -1 and b"0 < d" in L.ssg_last_error()
    assert L.ssg_eug_nn_f32(None, 0, None, ref.NL, 9, None, 1, *none, None) == -1 and b"nu, nl > 0" in L.ssg_last_error()
    assert L.ssg_eug_nn_f32(None, ref.NU, None, ref.NL, 9, None, ns + 1, *none, None) == -1 and b"nsplit must be" in L.ssg_last_error()
    for n, k in ((1024, 1025), (1024, -1), (1, 2), (0, 0)):
        assert L.ssg_eug_select_top(None, n, k, None, None, None) == -1, (n, k)
        assert b"0 <= k <= n" in L.ssg_last_error()
    assert L.ssg_eug_dist_label_f32(None, 4, 0, None, None, None, None, None, None, None) == -1 and b"nu, nl > 0" in L.ssg_last_error()
    assert L.ssg_eug_dist_label_f32(None, 4, 4, None, None, None, None, None, None, None) == -1 and b"missing buffer" in L.ssg_last_error()
    # the structures the GPU suite names
    s = L.ssg_eug_nn_splits(8197, 1283)
    assert ref.structure(8197, 1283, s)[1] == 21 and s >= 2 and ref.structure(8197, 1283, s)[2] >= 2
    s = L.ssg_eug_nn_splits(65600, 130)
    assert s == 1 and ref.structure(65600, 130, s) == (2050, 3, 3)


def test_wrappers_refuse_before_any_launch():
    """host tensors (device='cpu') never reach a kernel: a label count that does not match, widths that differ, k outside [0, n],
    a label count that does not match the scores"""
    import torch
    from ssg_amd.eug import dissimilarity_from_dist, nearest_labelled, select_top
    u, l = ref.features(5, 7, 9, 1)
    with pytest.raises(ValueError, match=r"l_label \[Nl\] expected"):
        nearest_labelled(u, l, np.arange(6), device="cpu")
    with pytest.raises(ValueError, match=r"l_label \[Nl\] expected"):
        nearest_labelled(u, l, np.arange(8), device="cpu")
    with pytest.raises(ValueError, match="expected"):
        nearest_labelled(u, l[:, :8], np.arange(7), device="cpu")
    with pytest.raises(ValueError, match="expected"):
        nearest_labelled(u[0], l, np.arange(7), device="cpu")
    with pytest.raises(ValueError, match="l_label has 6 entries for 7 columns"):
        dissimilarity_from_dist(torch.zeros(5, 7), np.arange(6), device="cpu")
    s = np.arange(1024, dtype=np.float64)
    for k in (-1, 1025):
        with pytest.raises(ValueError, match=r"k = %d outside \[0, 1024\]" % k):
            select_top(s, k, device="cpu")
    with pytest.raises(ValueError, match="1023 labels for 1024 scores"):
        select_top(s, 5, labels=np.zeros(1023), device="cpu")
    assert select_top(np.zeros(0), 0, device="cpu").shape == (0,)
