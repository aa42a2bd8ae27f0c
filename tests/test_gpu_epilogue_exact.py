"""GPU suite (-m gpu): the convolution epilogues of csrc/conv.hip, bit for bit against a numpy restatement, on every kernel conv_route
can pick for a split-half launch.

ssg_conv2d_nhwc_x runs as a 1 x 1 convolution with Cin = Cout = 256 over M one-pixel images.  The weights are a diagonal of per-row
powers of two 2^e[c] that the per-channel scale cs[c] = 2^-e[c] undoes, and every input value is a (hi, lo) pair whose sum is exact in
float32.  Each accumulator then holds one non-zero product per matrix instruction and is known exactly, acc = (hi + lo) * 2^e[c], and
the output must equal

    encode(relu(acc * cs + bias [+ decode(res)]))       decode = float32(hi) + float32(lo), encode: hi = half(v), lo = half(v - hi)

pattern for pattern; the range flag must be raised exactly when the restatement holds a non-finite hi half.  The inputs mix a pool of
special pairs (every finite half below 2^15 as hi with lo = 0, the ties half an ulp away and the smallest subnormal halves; pool length
prime, so every chunk, lane parity and patch row meets all of them) with random pairs; half the channels have a zero bias, so there the
encoder sees the special values themselves, the other half and the residual feed it full-width float32 values.  `near` adds 65519
(hi = 65504: no flag; launches without a residual), `over` adds 65520 (hi = inf: flag).  M is ragged (+ 17 rows), so the last tile's
exchange runs with lanes whose rows are out of range.

    M            residual  relu  kernel
    51200 + 17   no        1     LDS-DMA 256 x 256, straight-line epilogue
    32768 + 17   yes       1     LDS-DMA 128 x 256, straight-line epilogue
    32768 + 17   yes       0     LDS-DMA 128 x 256, general epilogue
    20480 + 17   yes / no  1     LDS-DMA 128 x 128
    4096 + 17    yes       1     register-staged 128 x 64 (fewer than 300 tiles of 128 x 128)
    SSG_CONV_DMA=0 in a fresh child process: register-staged 128 x 256 and 128 x 128
NaN: the lo half of an infinite hi is half(inf - inf), whose sign and payload IEEE 754 leaves open: any NaN equals any NaN.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C = 256
MMAX = 51200 + 17
CASES = [("tall", 51200 + 17, False, 1), ("wide_res", 32768 + 17, True, 1), ("wide_res_general", 32768 + 17, True, 0),
         ("dma128_res", 20480 + 17, True, 1), ("dma128", 20480 + 17, False, 1), ("igemm64_res", 4096 + 17, True, 1)]
CHILD_CASES = [("igemm256_res", 32768 + 17, True, 1), ("igemm128", 20480 + 17, False, 1)]


def _f16(bits):
    return bits.astype(np.uint16).view(np.float16).astype(np.float32)


def _pairs(rng, n, lim):
    """n (hi, lo) half patterns, |hi| < lim, hi + lo exact in float32: the special pool in a prime cycle, random pairs in between;
    a block of 1000003 of them (prime: it drifts through the tiles) repeated"""
    total, n = n, min(n, 1000003)
    allh = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    h = allh[((allh & 0x7fff) < np.float16(lim).view(np.uint16))]
    hv = h.view(np.float16)
    with np.errstate(over="ignore"):
        hu = (np.abs(np.spacing(hv)).astype(np.float32) * np.float32(0.5)).astype(np.float16)      # half an ulp of hi (0 below 2^-23)
    tiny = np.float16(2.0 ** -24)
    pool_hi = np.concatenate([h, h, h, h, h])
    pool_lo = np.concatenate([np.zeros_like(hv), hu, -hu, np.full_like(hv, tiny), np.full_like(hv, -tiny)]).view(np.uint16)
    keep = rng.permutation(pool_hi.size)[:40009]                                                   # a prime number of them
    pool_hi, pool_lo = pool_hi[keep], pool_lo[keep]
    idx = np.arange(n) % keep.size
    hi, lo = pool_hi[idx].copy(), pool_lo[idx].copy()
    rnd = rng.random(n) < 0.5
    rh = np.ldexp(rng.standard_normal(n), rng.integers(-6, 4, n)).astype(np.float16)
    rl = (rng.uniform(-1, 1, n).astype(np.float32) * np.abs(np.spacing(rh)).astype(np.float32) * np.float32(0.5)).astype(np.float16)
    hi[rnd], lo[rnd] = rh.view(np.uint16)[rnd], rl.view(np.uint16)[rnd]
    s64 = _f16(hi).astype(np.float64) + _f16(lo).astype(np.float64)
    inexact = s64.astype(np.float32).astype(np.float64) != s64
    lo[inexact] = 0
    return np.resize(hi, total), np.resize(lo, total)


def _containers(hi, lo):
    """[M, C] half patterns -> the h8l8 tensor ([8 x hi][8 x lo] per 8 channels) as float32 words"""
    m = hi.shape[0]
    return np.concatenate([hi.reshape(m, C // 8, 8), lo.reshape(m, C // 8, 8)], axis=2).reshape(m, 2 * C).view(np.float32)


def _data():
    rng = np.random.default_rng(256256)
    d = {}
    xh, xl = _pairs(rng, MMAX * C, 32768.0)
    d["xh"], d["xl"] = xh.reshape(MMAX, C), xl.reshape(MMAX, C)
    rh, rl = _pairs(rng, (32768 + 17) * C, 64.0)
    d["rh"], d["rl"] = rh.reshape(-1, C), rl.reshape(-1, C)
    d["e"] = rng.integers(-3, 4, C)
    d["bias"] = np.where(np.arange(C) % 2 == 0, 0.0, rng.standard_normal(C)).astype(np.float32)
    rng.shuffle(d["bias"])
    return d


def _restate(d, M, res, relu, xh, xl):
    """-> (hi, lo) patterns [M, C] of the expected output"""
    with np.errstate(invalid="ignore", over="ignore"):
        acc = (_f16(xh) + _f16(xl)) * np.ldexp(np.float32(1), d["e"]).astype(np.float32)
        v = acc * np.ldexp(np.float32(1), -d["e"]).astype(np.float32) + d["bias"]
        if res:
            v = v + (_f16(d["rh"][:M]) + _f16(d["rl"][:M]))
        if relu:
            v = np.where(v > 0, v, np.float32(0))
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def _canon(b):
    return np.where((b & 0x7fff) > 0x7c00, np.uint16(0x7e00), b)


def run_case(d, M, res, relu, variant):
    """one launch against the restatement -> list of complaints (empty: equal)"""
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    xh, xl = d["xh"][:M], d["xl"][:M]
    if variant != "base":
        xh, xl = xh.copy(), xl.copy()
        rows = np.array([0, 1, 30, 31, 127, 128, 129, M // 2, M - 18, M - 2, M - 1])
        cols = np.flatnonzero(d["bias"] == 0)[(rows * 37 + np.arange(rows.size)) % (C // 2)]      # zero-bias channels: v = 65519 / 65520 itself
        xh[rows, cols] = np.float16(65504.0).view(np.uint16)
        xl[rows, cols] = np.float16(15.0 if variant == "near" else 16.0).view(np.uint16)
    w = np.zeros((C, C // 8, 16), np.uint16)
    w[np.arange(C), np.arange(C) // 8, np.arange(C) % 8] = np.ldexp(np.float32(1), d["e"]).astype(np.float16).view(np.uint16)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x, wt, bias = t(_containers(xh, xl)), t(w.reshape(C, 2 * C).view(np.float32)), t(d["bias"])
    cs = t(np.ldexp(np.float32(1), -d["e"]).astype(np.float32))
    r = t(_containers(d["rh"][:M], d["rl"][:M])) if res else None
    out = torch.full((M, C), float("nan"), dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    check(L.ssg_conv2d_nhwc_x(ptr(x), ptr(wt), ptr(bias), ptr(r), ptr(out), M, 1, 1, C, C, 1, 1, 1, 0, relu, 3, 1.0, ptr(cs), ptr(flag), stream()),
          "ssg_conv2d_nhwc_x")
    got = out.cpu().numpy().view(np.uint16).reshape(M, C // 8, 16)
    eh, el = _restate(d, M, res, relu, xh, xl)
    want_flag = int(((eh & 0x7c00) == 0x7c00).any())
    bad = []
    for name, g, e in (("hi", got[:, :, :8].reshape(M, C), eh), ("lo", got[:, :, 8:].reshape(M, C), el)):
        ne = np.argwhere(_canon(g) != _canon(e))
        if ne.size:
            i, j = ne[0]
            bad.append("%s: %d of %d differ, first at row %d channel %d: got %#06x want %#06x" % (name, len(ne), g.size, i, j, g[i, j], e[i, j]))
    if int(flag.item()) != want_flag:
        bad.append("range flag %d, restatement %d" % (int(flag.item()), want_flag))
    if want_flag != (1 if variant == "over" else 0):
        bad.append("the inputs of variant %s give flag %d in the restatement" % (variant, want_flag))
    if not ((el & 0x7c00) == 0).sum() > el.size // 8:
        bad.append("few subnormal lo halves in the expected output")
    return bad


@pytest.fixture(scope="module")
def data():
    return _data()


@pytest.mark.parametrize("variant", ["base", "over"])
@pytest.mark.parametrize("name,M,res,relu", CASES, ids=[c[0] for c in CASES])
def test_epilogue_bits(name, M, res, relu, variant, data):
    assert run_case(data, M, res, relu, variant) == []


def test_epilogue_bits_just_below_the_range_edge(data):
    """65519 = 65504 + 15 encodes to hi = 65504: equal bits and no flag"""
    assert run_case(data, 51200 + 17, False, 1, "near") == []
    assert run_case(data, 20480 + 17, False, 1, "near") == []


def test_register_staged_kernels_in_a_child_process():
    """SSG_CONV_DMA is read once per process: a fresh interpreter with SSG_CONV_DMA=0 runs the register-staged kernels on the same data"""
    env = dict(os.environ, SSG_CONV_DMA="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "child ok" in r.stdout


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dd = _data()
    fails = []
    for cname, cm, cres, crelu in CHILD_CASES:
        for var in ("base", "over"):
            fails += ["%s/%s: %s" % (cname, var, b) for b in run_case(dd, cm, cres, crelu, var)]
    print("\n".join(fails) if fails else "child ok")
    sys.exit(1 if fails else 0)
