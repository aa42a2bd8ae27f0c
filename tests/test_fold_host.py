"""CPU half of the embedder-refresh tests: the scalar rules of csrc/fold.hip (float64 BatchNorm scale / weight / bias, the row-scale
exponent taken from the bits of the row maximum, the hi / lo half split, the packed index of both layouts), cut out of the .hip file
and compiled as the SAME SOURCE TEXT for x86 (tools/hostexec/fold_rules.cpp, ROCm's clang, host only), held bit for bit to `_fold`,
`_row_scales`, `_h8l8`, `_h4l4` and `pack_weight_khwc` of ssg_amd/resnet.py; and what needs no device at all: the public surface
(`ResNet.refresh`, the entry points of include/ssg_hip.h) and the refusals that come before any launch.  No GPU.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import fold_ref
from ssg_amd import _lib, resnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def hx(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang++ not present")
    d = tmp_path_factory.mktemp("hx_fold")
    out, on = [], False
    for line in open(os.path.join(ROOT, "self-similarity-grouping_amd", "csrc", "fold.hip")):
        if line.startswith("__device__ __forceinline__ double fold_scale"):
            on = True
        if "end of the scalar rules" in line:
            break
        if on:
            out.append(line)
    text = "".join(out)
    for name in ("fold_scale", "fold_weight", "fold_bias", "fold_row_exponent", "fold_pow2", "fold_split", "fold_packed_index", "fold_stem_index"):
        assert "__device__ __forceinline__" in text and name + "(" in text, name
    (d / "fold_cut.inc").write_text(text)
    so = str(d / "libhx_fold.so")
    r = subprocess.run([CLANG, "-x", "hip", "--offload-host-only", "-O2", "-shared", "-fPIC", "-I/opt/rocm/include", "-I" + str(d), "-o", so,
                        os.path.join(ROOT, "tools", "hostexec", "fold_rules.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _i32(t):
    return t.contiguous().view(torch.int32)


def _row_scale(hx, mx):
    """(e, 2^e, 2^-e) of the compiled rule for float32 row maxima"""
    mx = np.ascontiguousarray(mx, np.float32)
    e = np.empty(mx.size, np.int32); sc = np.empty(mx.size, np.float32); inv = np.empty(mx.size, np.float32)
    hx.hx_fold_row_scale(_p(mx), ctypes.c_long(mx.size), _p(e), _p(sc), _p(inv))
    return e, sc, inv


def _emulate(hx, case, split):
    """the kernel's steps with the compiled rules, the data movement in numpy -> (w, bias, cscale) as torch tensors"""
    w = case["w"]
    cout, cin, kh, kw = w.shape
    taps = kh * kw
    f32 = lambda t: np.ascontiguousarray(t.numpy(), np.float32)                        # noqa: E731
    scale = np.empty(cout, np.float64); bias = np.empty(cout, np.float32)
    hx.hx_fold_channel(_p(f32(case["gamma"])), _p(f32(case["beta"])), _p(f32(case["mean"])), _p(f32(case["var"])), ctypes.c_double(fold_ref.EPS),
                       ctypes.c_long(cout), _p(scale), _p(bias))
    src = f32(w.reshape(cout, cin * taps)); wf = np.empty_like(src)
    hx.hx_fold_weight(_p(src), _p(scale), ctypes.c_long(cout), ctypes.c_long(cin * taps), _p(wf))
    idx = np.empty(cin * taps, np.int32)
    hx.hx_fold_index(cin, taps, _p(idx))
    kp = 32 * ((taps + 7) // 8) if cin == 3 else cin * taps
    packed = np.zeros((cout, kp), np.float32)
    packed[:, idx] = wf
    if not split:
        return torch.from_numpy(packed), torch.from_numpy(bias), None
    _, sc, inv = _row_scale(hx, np.abs(packed).max(axis=1))
    hi = np.empty((cout, kp), np.uint16); lo = np.empty((cout, kp), np.uint16)
    hx.hx_fold_split(_p(packed), _p(sc), ctypes.c_long(cout), ctypes.c_long(kp), _p(hi), _p(lo))
    grp = 4 if cin == 3 else 8
    halves = np.stack([hi.reshape(cout, kp // grp, grp), lo.reshape(cout, kp // grp, grp)], axis=2).reshape(cout, 2 * kp)
    return torch.from_numpy(np.ascontiguousarray(halves).view(np.float32)), torch.from_numpy(bias), torch.from_numpy(inv)


# ------------------------------------------------------------------ the surface (fails without the feature)
def test_refresh_and_fold_entry_points_are_declared():
    assert callable(getattr(resnet.ResNet, "refresh", None))
    protos = _lib.parse_header()
    for name in ("ssg_fold_conv_bn_f32", "ssg_fold_conv_bn_dual_f32", "ssg_fold_max_k"):
        assert name in protos, name
    assert _lib.lib().ssg_fold_max_k() >= 512 * 3 * 3                                   # the longest ResNet row fits


def _single(L, cout, cin, kh, kw, split=1, w=1, out=1):
    """ssg_fold_conv_bn_f32 with made-up (never dereferenced) pointers"""
    p = ctypes.c_void_p
    return L.ssg_fold_conv_bn_f32(p(w * 4096), cin * kh * kw, kh * kw, kw, 1, cout, cin, kh, kw, p(4096), p(4096), p(4096), p(4096), 1e-5, split,
                                  p(out * 4096), p(4096), p(4096), None)


def _dual(L, cout, cin1, cin2, k1=1, k2=1):
    p = ctypes.c_void_p
    a = [p(4096), cin1 * k1 * k1, k1 * k1, k1, 1, cin1, k1, k1, p(4096), p(4096), p(4096), p(4096)]
    b = [p(4096), cin2 * k2 * k2, k2 * k2, k2, 1, cin2, k2, k2, p(4096), p(4096), p(4096), p(4096)]
    return L.ssg_fold_conv_bn_dual_f32(*a, *b, 1e-5, cout, 1, p(4096), p(4096), p(4096), None)


def test_refusals_come_before_any_launch():
    """everything outside the rules returns -1 and names the entry point in ssg_last_error -- no device is touched (this box has none)"""
    L = _lib.lib()
    cap = L.ssg_fold_max_k()
    for what, call in (("Cin % 32", lambda: _single(L, 64, 48, 1, 1)), ("Cout % 64", lambda: _single(L, 96, 64, 1, 1)),
                       ("Cin = 4", lambda: _single(L, 64, 4, 7, 7)), ("Cout = 0", lambda: _single(L, 0, 64, 1, 1)),
                       ("row beyond LDS", lambda: _single(L, 64, (cap // 9 // 32 + 1) * 32, 3, 3)),
                       ("NULL weight", lambda: _single(L, 64, 64, 1, 1, w=0)), ("NULL output", lambda: _single(L, 64, 64, 1, 1, out=0)),
                       ("NULL ch_scale in split mode", lambda: L.ssg_fold_conv_bn_f32(ctypes.c_void_p(4096), 64, 1, 1, 1, 64, 64, 1, 1, *([ctypes.c_void_p(4096)] * 4),
                                                                                        1e-5, 1, ctypes.c_void_p(4096), ctypes.c_void_p(4096), None, None)),
                       ("negative stride", lambda: L.ssg_fold_conv_bn_f32(ctypes.c_void_p(4096), 64, -1, 1, 1, 64, 64, 1, 1, *([ctypes.c_void_p(4096)] * 4),
                                                                            1e-5, 0, ctypes.c_void_p(4096), ctypes.c_void_p(4096), None, None)),
                       ("unaligned output", lambda: L.ssg_fold_conv_bn_f32(ctypes.c_void_p(4096), 64, 1, 1, 1, 64, 64, 1, 1, *([ctypes.c_void_p(4096)] * 4),
                                                                             1e-5, 0, ctypes.c_void_p(4100), ctypes.c_void_p(4096), None, None))):
        assert call() == -1, what
        assert b"ssg_fold_conv_bn_f32" in L.ssg_last_error(), what
    for what, call in (("3x3 second source", lambda: _dual(L, 64, 64, 64, k2=3)), ("3x3 first source", lambda: _dual(L, 64, 64, 64, k1=3)),
                       ("Cin2 % 32", lambda: _dual(L, 64, 64, 48)), ("stem in the dual form", lambda: _dual(L, 64, 3, 64)),
                       ("Cout % 64", lambda: _dual(L, 96, 64, 64)), ("row beyond LDS", lambda: _dual(L, 64, cap // 2, cap // 2 + 32))):
        assert call() == -1, what
        assert b"ssg_fold_conv_bn_dual_f32" in L.ssg_last_error(), what
    with pytest.raises(ValueError, match="ssg_fold_conv_bn_f32"):
        _lib.check(_single(L, 64, 48, 1, 1), "ssg_fold_conv_bn_f32")


def test_refresh_needs_a_gpu_resident_model():
    m = resnet.ResNet(18, pretrained=False)
    with pytest.raises(_lib.SSGError):
        m.refresh(m.state_dict())


# ------------------------------------------------------------------ the compiled rules against resnet.py
def test_row_scale_from_bits_is_row_scales(hx):
    """e from the bits of the maximum == floor(log2(16384 / mx)) clamped to +-40 as `_row_scales` evaluates it in float64: every float32
    power of two from 2^-149 to 2^127 with both neighbours, 0, the crafted maxima, and random magnitudes over 24 decades"""
    p2 = np.ldexp(1.0, np.arange(-149, 128)).astype(np.float32)
    rng = np.random.default_rng(5)
    mx = np.concatenate([p2, np.nextafter(p2, np.float32(np.inf)), np.nextafter(p2, np.float32(0)), [0.0, 16384.0, 8192.0, 3.4028235e38, 1e-45],
                         np.exp(rng.uniform(np.log(1e-12), np.log(1e12), 20000))]).astype(np.float32)
    mx = mx[np.isfinite(mx)]
    e, sc, inv = _row_scale(hx, mx)
    ref = resnet._row_scales(torch.from_numpy(mx).view(-1, 1))
    assert np.array_equal(sc.view(np.uint32), ref.numpy().view(np.uint32))
    assert np.array_equal(inv.view(np.uint32), (1.0 / ref).numpy().view(np.uint32))
    assert np.array_equal(np.ldexp(1.0, e).astype(np.float32), sc) and e.min() == -40 and e.max() == 40 and (mx == 0).any() and not e[mx == 0].any()
    live = (mx > 0) & (np.abs(e) < 40)
    scaled = mx[live].astype(np.float64) * sc[live]
    assert np.all((scaled > 8192) & (scaled <= 16384))


def test_split_rule_is_h8l8_and_h4l4(hx):
    """hi = half(w * sc), lo = half(w * sc - hi) with torch's roundings: random rows over the whole half range and below it, exact halves
    (lo = 0), values whose lo half is subnormal, values that overflow the half range"""
    g = torch.Generator().manual_seed(7)
    rows, k = 16, 64
    v = torch.randn(rows, k, generator=g) * torch.exp(torch.rand(rows, 1, generator=g) * 30 - 20)
    v[0, :8] = torch.tensor([1.0, 1.0 + 2.0 ** -20, 0.5 + 2.0 ** -11, 3e-6, 2.0 ** -24, 1.5 * 2.0 ** -25, 0.0, -0.0])
    v[1, :4] = torch.tensor([65504.0, 65519.9, 65520.0, -1e6])
    sc = torch.pow(2.0, torch.randint(-6, 7, (rows,), generator=g).float())
    hi = np.empty((rows, k), np.uint16); lo = np.empty((rows, k), np.uint16)
    vn = np.ascontiguousarray(v.numpy()); sn = np.ascontiguousarray(sc.numpy())
    hx.hx_fold_split(_p(vn), _p(sn), ctypes.c_long(rows), ctypes.c_long(k), _p(hi), _p(lo))
    scaled = v * sc.view(-1, 1)
    for grp, enc in ((8, resnet._h8l8), (4, resnet._h4l4)):
        halves = np.stack([hi.reshape(rows, k // grp, grp), lo.reshape(rows, k // grp, grp)], axis=2).reshape(rows, 2 * k)
        got = torch.from_numpy(np.ascontiguousarray(halves).view(np.int32))
        assert torch.equal(got, _i32(enc(scaled))), grp


def test_packed_index_is_pack_weight_khwc_and_the_stem_order(hx):
    for cin, kh, kw in ((32, 1, 1), (64, 3, 3), (96, 3, 1), (512, 3, 3), (3, 7, 7)):
        taps = kh * kw
        idx = np.empty(cin * taps, np.int32)
        hx.hx_fold_index(cin, taps, _p(idx))
        w = torch.arange(1, cin * taps + 1, dtype=torch.float32).view(1, cin, kh, kw)             # value = 1 + (c * taps + tap)
        if cin == 3:
            ref = torch.nn.functional.pad(w.permute(0, 2, 3, 1), (0, 1)).reshape(-1)                # [KH, KW, 4]: what `_fold` builds for the stem
        else:
            ref = resnet.pack_weight_khwc(w.permute(0, 2, 3, 1).contiguous()).reshape(-1)
        assert len(set(idx.tolist())) == idx.size and idx.min() >= 0 and idx.max() < ref.numel()
        assert torch.equal(ref[torch.from_numpy(idx).long()], w.reshape(-1)), (cin, kh, kw)


CASES = {"stem": (64, 3, 7, 7), "one_chunk": (64, 32, 1, 1), "chunk_major": (64, 64, 3, 3), "linear": (64, 512, 1, 1)}


def test_crafted_rows_hold_what_they_claim():
    for i, shape in enumerate(CASES.values()):
        fold_ref.check_crafted(fold_ref.crafted(*shape, seed=100 + i))


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("split", (False, True))
def test_compiled_rules_reproduce_fold(hx, name, split):
    """the kernel's steps, run with the compiled rules on the crafted rows and on random rows, give `_fold`'s w, bias and ch_scale"""
    case = fold_ref.crafted(*CASES[name], seed=100 + list(CASES).index(name))
    w, bias, cs = _emulate(hx, case, split)
    rw, rb, rcs = fold_ref.host_fold(case, split)
    assert torch.equal(_i32(bias), _i32(rb))
    assert torch.equal(_i32(w), _i32(rw))
    assert (cs is None and rcs is None) or torch.equal(_i32(cs), _i32(rcs))
