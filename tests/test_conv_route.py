"""Which kernel instance a convolution-GEMM launch runs (csrc/conv.hip: conv_route), executed on the host.

conv_route is a pure function of the launch parameters and the routing knobs; tools/hostexec/conv_route.cpp compiles its SOURCE TEXT (cut out
of conv.hip, with `struct ConvParams`) for x86.  This file compares it, over a grid of shapes, epilogues and knob sets, with a restatement of
the rules it replaced, written from the functions the library had before: launch_conv (BK and the 128x128 LDS-DMA launches),
conv_prefers_wide / conv_prefers_bn64 (tile), launch_conv_wide (128x256 / 256x256, the 2 GiB weight guard, the register-staged fallback),
conv_line_order (fetch order) and their call sites -- the two convolution entry points, the float32 distance GEMMs and the source term's
bound pass (the only caller with epi 3: 128x256 tiles when Cout % 256 == 0, else 128x128, whatever the tile counts).  The knobs of those
functions that were retired with them stand at their defaults (BK = 16 for fp32 and stem launches without a second input and never for
the split register-staged kernel; four stages and 64-row wave tiles on 256x256).
No GPU."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
IGEMM, DMA = 0, 1
KNOBS = ("dma", "line", "wide_mintiles", "bn64_maxtiles", "tall_mintiles", "tall_res", "tall_dual")
ENV = {"SSG_CONV_DMA": "dma", "SSG_CONV_LINE": "line", "SSG_SPLIT_WIDE_MINTILES": "wide_mintiles", "SSG_SPLIT_BN64_MAXTILES": "bn64_maxtiles",
       "SSG_CONV_TALL_MINTILES": "tall_mintiles", "SSG_CONV_TALL_RES": "tall_res", "SSG_CONV_TALL_DUAL": "tall_dual"}
# the knob sets of tests/test_conv_line_fetch.py and tests/test_conv_tiled_weights.py
WIDE = {"SSG_SPLIT_WIDE_MINTILES": "1", "SSG_SPLIT_BN64_MAXTILES": "0", "SSG_CONV_TALL_MINTILES": "0"}
TALL = {"SSG_SPLIT_WIDE_MINTILES": "1", "SSG_SPLIT_BN64_MAXTILES": "0", "SSG_CONV_TALL_MINTILES": "1", "SSG_CONV_TALL_RES": "1", "SSG_CONV_TALL_DUAL": "1"}


@pytest.fixture(scope="module")
def hx(tmp_path_factory):
    cxx = CLANG if os.path.exists(CLANG) else shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("route")
    src = open(os.path.join(ROOT, "self-similarity-grouping_amd", "csrc", "conv.hip")).read()
    a = src.index("struct ConvParams {")
    params = src[a:src.index("\n};\n", a) + 4]
    route = src[src.index("struct ConvKnobs {"):src.index("// ---- end of routing")]
    # pure: no knob read, no launch, no cached state (the text is compiled without any HIP header, so a HIP call would not build either)
    assert "conv_route(const ConvParams& p" in route and "getenv" not in route and "hipLaunch" not in route and "static int " not in route
    (d / "conv_route_cut.inc").write_text(params + "\n" + route)
    so = str(d / "libroute.so")
    r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I" + str(d), "-o", so,
                        os.path.join(ROOT, "tools", "hostexec", "conv_route.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return ctypes.CDLL(so)


def knobs_of(env):
    """the knob values the library had read from `env` before this change: atoi of what is set, else the default; SSG_CONV_LINE is 1, 0 or unset (-1)"""
    k = dict(dma=3, line=-1, wide_mintiles=256, bn64_maxtiles=300, tall_mintiles=200, tall_res=0, tall_dual=0)
    for name, field in ENV.items():
        if name in env:
            k[field] = (1 if int(env[name]) == 1 else 0) if field == "line" else int(env[name])
    return k


def parent_route(M, Cout, Kpad, Cin, Cin2, res, in2, epi, split, cin4, k):
    """(family, BM, BN, BK, dual, line) by the rules of the launch functions this routing function replaced"""
    def igemm(BN, BK):
        return (IGEMM, 128, BN, BK, int(in2), 0)

    def line_order(inst):                                   # conv_line_order
        if epi != 0 or ((Kpad // 16) & 1) or Cin % 32 or (in2 and Cin2 % 32):
            return 0
        if k["line"] >= 0:
            return k["line"]
        return {"128": 1, "wide": 1, "wide_dual": 1, "tall": 1, "tall_dual": 0}[inst]

    def launch_conv(BN, CIN4):                              # launch_conv<128, BN, 64, BN / 2, CIN4>
        if split:
            if CIN4:
                return igemm(BN, 16)
            if BN == 128 and (k["dma"] & 2) and epi == 0 and not in2:
                return (DMA, 128, 128, 16, 0, line_order("128"))
            return igemm(BN, 32)
        return igemm(BN, 16) if not in2 else igemm(BN, 32)

    def launch_conv_wide():
        if (k["dma"] & 1) and epi in (0, 3) and Cout * Kpad * 4 < 0x7fffffff:
            tall, tiles_tall = k["tall_mintiles"], ((M + 255) // 256) * (Cout // 256)
            if tall > 0 and epi == 0 and in2 and k["tall_dual"] and tiles_tall >= tall:
                return (DMA, 256, 256, 16, 1, line_order("tall_dual"))
            if tall > 0 and epi == 0 and (not res or k["tall_res"]) and not in2 and tiles_tall >= tall:
                return (DMA, 256, 256, 16, 0, line_order("tall"))
            return (DMA, 128, 256, 16, int(in2), line_order("wide_dual" if in2 else "wide"))
        return igemm(256, 32)

    def prefers_wide():
        if not split or k["wide_mintiles"] <= 0 or Cout % 256 or Kpad < 128:
            return False
        return ((M + 127) // 128) * (Cout // 256) >= k["wide_mintiles"]

    def prefers_bn64():
        return split and ((M + 127) // 128) * (Cout // 128) < k["bn64_maxtiles"]

    if epi == 3:                                            # source_term.hip
        if split:
            return launch_conv_wide() if Cout % 256 == 0 else igemm(128, 32)
        return launch_conv(128, False)
    if cin4:                                                # ssg_conv2d_nhwc_xt, stem
        return launch_conv(128, True) if Cout % 128 == 0 else launch_conv(64, True)
    if prefers_wide():                                      # both entry points; the distance GEMMs (split = False) take the last line alone
        return launch_conv_wide()
    return launch_conv(128, False) if Cout % 128 == 0 and not prefers_bn64() else launch_conv(64, False)


def route(hx, cases, k):
    q = np.ascontiguousarray(np.array(cases, np.int32).reshape(-1, 10))
    kn = np.array([k[f] for f in KNOBS], np.int32)
    out = np.empty((q.shape[0], 6), np.int32)
    hx.hx_conv_route(q.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(q.shape[0]), kn.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    return [tuple(int(v) for v in row) for row in out]


def test_knob_defaults(hx):
    kn = np.empty(7, np.int32)
    hx.hx_conv_knob_defaults(kn.ctypes.data_as(ctypes.c_void_p))
    assert dict(zip(KNOBS, kn.tolist())) == knobs_of({})


def _cases():
    """M x Cout x Kpad x residual x second input x epi x (fp32, split, split stem, fp32 stem).  Without a second input Cin = Kpad (a 1x1
    convolution; 144 = nine k-tiles, no 32-channel runs), with one the two inputs share K evenly (Kpad 32 / 96 / 144: no 32-channel runs).
    The stem (Cin = 4) comes through ssg_conv2d_nhwc_xt alone: no second input, convolution epilogue."""
    out = []
    for M, Cout, Kpad, res, in2, epi, (split, cin4) in itertools.product(
            (1, 127, 128, 129, 255 * 128, 256 * 128, 299 * 128, 300 * 128, 128000), (64, 128, 256, 1024), (32, 64, 96, 128, 144, 1024, 2304),
            (0, 1), (0, 1), (0, 1, 3), ((0, 0), (1, 0), (1, 1), (0, 1))):
        if cin4 and (in2 or epi):
            continue
        Cin, Cin2 = (4, 0) if cin4 else ((Kpad // 2, Kpad // 2) if in2 else (Kpad, 0))
        out.append((M, Cout, Kpad, Cin, Cin2, res, in2, epi, split, cin4))
    return out


def test_route_equals_the_rules_it_replaced(hx):
    cases = _cases()
    assert len(cases) == 9 * 4 * 7 * 2 * (2 * 2 * 3 + 2)
    nsets = 0
    for base, dma, line in itertools.product(({}, WIDE, TALL), (None, "0", "1", "2"), (None, "0", "1")):
        env = dict(base)
        if dma is not None:
            env["SSG_CONV_DMA"] = dma
        if line is not None:
            env["SSG_CONV_LINE"] = line
        k = knobs_of(env)
        got = route(hx, cases, k)
        for c, g in zip(cases, got):
            want = parent_route(*c, k)
            assert g == want, (env, dict(zip(("M", "Cout", "Kpad", "Cin", "Cin2", "res", "in2", "epi", "split", "cin4"), c)), g, want)
        nsets += 1
    assert nsets == 36


def test_weight_resource_guard_falls_back_to_the_register_staged_kernel(hx):
    """weights of 2 GiB or more do not fit conv_dma_kernel's buffer resource: 128x256 launches take conv_igemm_kernel"""
    k = knobs_of({})
    M = 128000
    for Cout, Kpad, fam in ((1024, 524288 - 32, DMA), (1024, 524288, IGEMM), (2048, 262144, IGEMM)):
        c = (M, Cout, Kpad, Kpad, 0, 0, 0, 0, 1, 0)
        (g,) = route(hx, [c], k)
        assert g == parent_route(*c, k) and g[0] == fam and g[2] == 256, (Cout, Kpad, g)


def test_resnet50_launches_by_name(hx):
    """The launches of a ResNet-50 forward on 256 x 128 images that carry the embedder (layer3: a 16 x 8 map), default knobs, split-half
    operands: at B = 1000 the LDS-DMA kernel in line order on the tiles the measurements chose, at B = 8 the register-staged 128x64 kernel."""
    k = knobs_of({})
    layer3 = {  # name: (Cout, Kpad, Cin, Cin2, residual, second input)
        "3x3": (256, 2304, 256, 0, 0, 0),
        "conv1": (256, 1024, 1024, 0, 0, 0),
        "conv3+residual": (1024, 256, 256, 0, 1, 0),
        "conv3|downsample": (1024, 768, 256, 512, 0, 1),
    }
    want1000 = {"3x3": (DMA, 256, 256, 16, 0, 1), "conv1": (DMA, 256, 256, 16, 0, 1), "conv3+residual": (DMA, 128, 256, 16, 0, 1),
                "conv3|downsample": (DMA, 128, 256, 16, 1, 1)}
    for name, (Cout, Kpad, Cin, Cin2, res, in2) in layer3.items():
        big = (1000 * 16 * 8, Cout, Kpad, Cin, Cin2, res, in2, 0, 1, 0)
        small = (8 * 16 * 8, Cout, Kpad, Cin, Cin2, res, in2, 0, 1, 0)
        g_big, g_small = route(hx, [big, small], k)
        assert g_big == want1000[name] == parent_route(*big, k), (name, g_big)
        assert g_small == (IGEMM, 128, 64, 32, in2, 0) == parent_route(*small, k), (name, g_small)
    # the stem (7x7 on RGB0 pixels, Kpad = 32 * ceil(49 / 8)) and the float32 distance GEMM of the evaluator
    (stem,) = route(hx, [(1000 * 128 * 64, 64, 224, 4, 0, 0, 0, 0, 1, 1)], k)
    assert stem == (IGEMM, 128, 64, 16, 0, 0)
    (dist,) = route(hx, [(3368, 15872, 2048, 2048, 0, 0, 0, 1, 0, 0)], k)
    assert dist == (IGEMM, 128, 128, 16, 0, 0)
