"""GPU suite (-m gpu): the embedder's non-GEMM kernels (csrc/conv.hip: layout change, split-half encode / decode, max-pool, global + stripe
average pool, flip-sum-L2) and the fp32 dual 1x1 GEMM, each called through its C entry point (include/ssg_hip.h) and compared with a plain
torch statement of the same operation on the CPU -- at sizes the 256 x 128 forward never gives them (1 x 1 maps, odd maps, rows that
belong to no stripe, channel counts that are not a multiple of 64, grids that wrap) and on inputs made for the mistakes a per-set L2
normalisation divides out: maps whose rows differ in magnitude (row r scaled by 1 + r) and a map of ones, on which every pooled set is
exactly 1.0f -- a wrong divisor or row range is then an exact failure.

Data movement, max and the hi / lo split are exact operations: those assertions are bit equality.  NaN: IEEE 754 fixes neither the sign
nor the payload of the NaN that inf - inf produces (the lo half of an infinite value; hosts and the GPU may differ), so `_same_bits` counts
any NaN as equal to any NaN and compares every other value, +-0 and +-inf included, bit for bit.

Derived bounds (u = 2^-24, nothing measured on the kernel):
  average pool   the kernel adds n = rows * W fp32 terms in sequence and divides once: |got - ref| <= (n + 1) * u * mean|x| over the
                 summed window, per output, from the float64 reference;
  flip-sum-L2    one rounding for a + b; per lane ceil(C / 64) squared terms added in sequence, 6 levels of the cross-lane tree, sqrt,
                 divide: relative error per element <= (ceil(C / 64) + 6 + 4) * u, applied as |got - ref| <= that * |ref| + u * |ref|max.
                 (Counting more tightly -- the sum of squares (k + 8) u with k = ceil(C / 64), halved by the root, plus one rounding each
                 for a + b, the root and the quotient -- gives (k / 2 + 7) u, below the constant used for every k.)
Each prints the worst observed error / bound (pytest -s).  ssg_flip_sum_l2norm's `out` may alias neither input: a wave reads its row
of a and b twice, before and after the norm (not tested: undefined by contract).
"""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional

U = 2.0 ** -24
INVALID = -1            # SSG_ERR_INVALID


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    from ssg_amd import _lib
    return _lib.lib()


def _call(fn, *args):
    """check(fn(..., stream)) with device pointers for tensors"""
    from ssg_amd._lib import check, ptr, stream
    check(fn(*[ptr(a) if torch.is_tensor(a) else a for a in args], stream()), fn.__name__)


def _canon(t):
    """integer view of a float32 / float16 tensor with every NaN mapped to one pattern"""
    if t.dtype == torch.float16:
        b = t.contiguous().view(torch.int16).to(torch.int32) & 0xffff
        return torch.where((b & 0x7fff) > 0x7c00, torch.full_like(b, 0x7e00), b)
    b = t.contiguous().view(torch.int32)
    return torch.where((b & 0x7fffffff) > 0x7f800000, torch.full_like(b, 0x7fc00000), b)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_canon(a.cpu()), _canon(b.cpu()))


def _split(v):
    """the two-line split of the header: hi = half(v), lo = half(v - hi)"""
    hi = v.half()
    return hi, (v - hi.float()).half()


def _grouped(v, g):
    """[..., n] fp32 -> halves in layout [h0..h(g-1) | l0..l(g-1)] per g values (h8l8: g = 8, the stem's h4l4: g = 4), as float16 [..., 2n]"""
    hi, lo = _split(v)
    shp = v.shape[:-1]
    return torch.stack([hi.reshape(*shp, -1, g), lo.reshape(*shp, -1, g)], dim=-2).reshape(*shp, -1)


def _decoded(v):
    """what a split-half container of v holds: hi + lo in fp32 (exact: |lo| <= ulp(hi) / 2, 11 + 11 significant bits)"""
    hi, lo = _split(v)
    return hi.float() + lo.float()


SALT = [0.0, -0.0, 1e-6, -1e-6, 6.0e-8, 1e-3 * (1 + 2.0 ** -12), -3e-2 * (1 + 2.0 ** -11), 2.0 ** -14, 2.0 ** -24, 65504.0, 65519.9, 65520.0, -65520.0, 1e5,
        float("inf"), float("-inf"), float("nan"), 1.0, -1.0 - 2.0 ** -12, 0.1]


def _salted(shape, seed):
    """randn over decades with the edge values of the split-half format strewn in"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 10.0 ** torch.randint(-3, 4, shape, generator=g).float()
    flat = x.view(-1)
    pos = torch.randperm(flat.numel(), generator=g)[:min(flat.numel(), 8 * len(SALT))]
    flat[pos] = torch.tensor(SALT).repeat(8)[:pos.numel()]
    return x


def _row_scaled(B, H, W, C, seed, negative=False):
    """NHWC map whose row r is scaled by 1 + r (a wrong row range changes a pooled value by far more than any tolerance)"""
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(seed)) * (1.0 + torch.arange(H).float()).view(1, H, 1, 1)
    return -x.abs() - 0.5 if negative else x


# ------------------------------------------------------------------ layout change
LAYOUT_SHAPES = [(1, 1, 1), (2, 7, 5), (3, 250, 100), (2, 256, 128), (1, 64, 33), (40, 256, 128)]       # the last: B*H*W > 4096 * 256 threads, the loop wraps


@pytest.mark.parametrize("B,H,W", LAYOUT_SHAPES)
def test_nchw_to_nhwc4(B, H, W, L, dev):
    x = _salted((B, 3, H, W), 100 * H + W)
    xd = x.to(dev)
    for flip in (0, 1):
        src = x.flip(3) if flip else x
        ref = torch.cat([src, torch.zeros(B, 1, H, W)], 1).permute(0, 2, 3, 1).contiguous()
        out = torch.full((B, H, W, 4), 7.0, device=dev)
        _call(L.ssg_nchw_to_nhwc4, xd, out, B, H, W, flip)
        assert _same_bits(out, ref), (B, H, W, flip)
        assert bool((out[..., 3].view(torch.int32) == 0).all())                    # +0.0, not -0.0
        # split-half pixels [h0 h1 h2 h3 | l0 l1 l2 l3]
        out4 = torch.full((B, H, W, 4), 7.0, device=dev)
        _call(L.ssg_nchw_to_nhwc4_h4l4, xd, out4, B, H, W, flip)
        got = out4.cpu().view(torch.float16)
        assert _same_bits(got, _grouped(ref, 4)), (B, H, W, flip)
        assert bool((got.view(torch.int16).view(B, H, W, 2, 4)[..., 3] == 0).all())   # hi and lo of the 4th channel: +0
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert L.ssg_nchw_to_nhwc4(None, None, *bad, 0, None) == INVALID and L.ssg_nchw_to_nhwc4_h4l4(None, None, *bad, 0, None) == INVALID


def test_h4l4_layout_is_the_host_encoders(L, dev):
    """the device pixel layout equals ssg_amd.resnet._h4l4 (what the stem weights are packed with; tests/test_abi.py states its format)"""
    from ssg_amd.resnet import _h4l4
    x = _salted((2, 3, 9, 6), 5)
    out = torch.empty(2, 9, 6, 4, device=dev)
    _call(L.ssg_nchw_to_nhwc4_h4l4, x.to(dev), out, 2, 9, 6, 0)
    nhwc4 = torch.cat([x, torch.zeros(2, 1, 9, 6)], 1).permute(0, 2, 3, 1).reshape(-1, 4)
    assert _same_bits(out.cpu().view(-1, 4).view(torch.float16), _h4l4(nhwc4).view(torch.float16))


# ------------------------------------------------------------------ split-half encode / decode
@pytest.mark.parametrize("n", [8, 4096, 8 * 4096 * 256 + 8])          # the last: one group more than the grid has threads
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -3, 2.0 ** 5])
def test_h8l8_encode_decode(n, scale, L, dev):
    from ssg_amd.resnet import _h8l8
    v = _salted((n,), 7) if n > 8 else torch.tensor(SALT[9:17])
    vd = v.to(dev)
    enc = torch.full((n,), 7.0, device=dev)
    _call(L.ssg_h8l8_encode, vd, enc, n, scale)
    want = _grouped(v * scale, 8)
    assert _same_bits(enc.cpu().view(torch.float16), want), (n, scale)
    assert torch.equal(_h8l8((v * scale).view(1, n)).view(torch.float16).view(torch.int16), want.view(1, -1).view(torch.int16))     # the host encoder of the weights: one format
    dec = torch.full((n,), 7.0, device=dev)
    _call(L.ssg_h8l8_decode, enc, dec, n, scale)
    hi, lo = _split(v * scale)
    assert _same_bits(dec, (hi.float() + lo.float()) * scale), (n, scale)


def test_h8l8_round_trip_is_exact_on_22_bit_values(L, dev):
    """decode(encode(v)) == v bit for bit for fp32 v of at most 22 significant bits, 2^-3 <= |v| < 65504; below 2^-3 the lo half is a
    half subnormal (step 2^-24) whenever v has bits under 2^-24: there the round trip is exact for the multiples of 2^-24 and within
    2^-25 otherwise, down to |v| = 2^-14 (the header's "22 significand bits, absolute floor 2^-24", tests/test_abi.py)."""
    g = torch.Generator().manual_seed(3)
    n = 1 << 20
    e = torch.randint(-3, 16, (n,), generator=g)                                    # binades 2^-3 .. 2^15
    m = (torch.randint(0, 1 << 21, (n,), generator=g).double() / (1 << 21) + 1.0)   # 1.xxx with 21 fraction bits: 22 significant bits
    v = (m * torch.pow(2.0, e.double()) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)).float()
    v = v[v.abs() < 65504.0]
    v = torch.cat([v, torch.tensor([2.0 ** -3, -(2.0 ** -3), 65503.984375, 65472.0, 2047.9990234375, 1.0 + 2.0 ** -21, 2.0 - 2.0 ** -21])])
    v = v[: v.numel() // 8 * 8].contiguous()
    small_e = torch.randint(-14, -3, (n,), generator=g)
    small = (m * torch.pow(2.0, small_e.double())).float()
    on_grid = torch.round(small.double() * 2 ** 24) == small.double() * 2 ** 24
    for x, exact in ((v, None), (small, on_grid)):
        xd = x.to(dev)
        enc, dec = torch.empty_like(xd), torch.empty_like(xd)
        _call(L.ssg_h8l8_encode, xd, enc, x.numel(), 1.0)
        _call(L.ssg_h8l8_decode, enc, dec, x.numel(), 1.0)
        dec = dec.cpu()
        assert _same_bits(dec, _decoded(x))
        if exact is None:
            assert torch.equal(dec.view(torch.int32), x.view(torch.int32))
        else:
            assert int(exact.sum()) > 1000 and torch.equal(dec[exact].view(torch.int32), x[exact].view(torch.int32))
            assert float((dec.double() - x.double()).abs().max()) <= 2.0 ** -25


def test_h8l8_encode_decode_refuse_bad_lengths(L):
    for n in (12, 7, 0, -8):
        for fn in (L.ssg_h8l8_encode, L.ssg_h8l8_decode):
            assert fn(None, None, n, 1.0, None) == INVALID
            assert b"multiple of 8" in L.ssg_last_error() and fn.__name__.encode() in L.ssg_last_error()


# ------------------------------------------------------------------ max-pool 3x3 stride 2 padding 1
POOL_MAPS = [(1, 1), (2, 2), (5, 3), (125, 50), (128, 64), (63, 25)]


def _pool_ref(x):
    return F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("C", [4, 64, 68])
@pytest.mark.parametrize("H,W", POOL_MAPS)
def test_maxpool3x3s2_nhwc(H, W, C, L, dev):
    B = 2
    OH, OW = (H + 1) // 2, (W + 1) // 2
    cases = {"rows": _row_scaled(B, H, W, C, H + C), "negative": _row_scaled(B, H, W, C, H + C + 1, negative=True)}     # padding must not contribute a 0
    inf = _row_scaled(B, H, W, C, H + C + 2)
    inf[0, :2, :2, :] = float("-inf")                                                # the window of output (0, 0) holds nothing else
    cases["-inf window"] = inf
    for name, x in cases.items():
        out = torch.full((B, OH, OW, C), 7.0, device=dev)
        _call(L.ssg_maxpool3x3s2_nhwc, x.to(dev), out, B, H, W, C)
        ref = _pool_ref(x)
        assert ref.shape == out.shape and _same_bits(out, ref), (name, H, W, C)
    assert bool((ref[0, 0, 0] == float("-inf")).all()) and bool((_pool_ref(cases["negative"]) < 0).all())
    assert L.ssg_maxpool3x3s2_nhwc(None, None, B, H, W, C + 2, None) == INVALID and b"C % 4" in L.ssg_last_error()


@pytest.mark.parametrize("C", [8, 64, 72])
@pytest.mark.parametrize("H,W", POOL_MAPS)
def test_maxpool3x3s2_h8l8(H, W, C, L, dev):
    """decode -> max_pool2d -> encode on the CPU; the kernel's output must be those bits (so its decode is the pooled decode).  The format
    holds no -inf (|v| < 65504), so the edge here is the all-negative map."""
    from ssg_amd.resnet import _h8l8
    B = 2
    OH, OW = (H + 1) // 2, (W + 1) // 2
    for name, x in (("rows", _row_scaled(B, H, W, C, H + C)), ("negative", _row_scaled(B, H, W, C, H + C + 1, negative=True)),
                    ("tiny", _row_scaled(B, H, W, C, H + C + 2) * 1e-4)):            # half-subnormal lo parts
        xs = _h8l8(x.view(-1, C)).view(B, H, W, C)
        out = torch.full((B, OH, OW, C), 7.0, device=dev)
        _call(L.ssg_maxpool3x3s2_h8l8, xs.to(dev), out, B, H, W, C)
        ref = _pool_ref(_decoded(x))
        assert _same_bits(out.cpu().view(-1, C).view(torch.float16), _h8l8(ref.view(-1, C)).view(torch.float16)), (name, H, W, C)
        assert torch.equal(_h8l8(ref.view(-1, C)).view(torch.float16), _grouped(ref.view(-1, C), 8))
        dec = torch.empty_like(out)
        _call(L.ssg_h8l8_decode, out, dec, out.numel(), 1.0)
        assert _same_bits(dec, ref), (name, H, W, C)
    assert L.ssg_maxpool3x3s2_h8l8(None, None, B, H, W, C + 4, None) == INVALID and b"C % 8" in L.ssg_last_error()


# ------------------------------------------------------------------ global + stripe average pool
GAP_CASES = [  # H, W, C, S, batches
    (8, 4, 2048, 1, (1, 3)), (8, 4, 2048, 2, (1, 3, 129)),      # 3 * 129 * 2048 outputs: more than the 2048 * 256 threads of the grid
    (12, 4, 2048, 3, (1, 3)),
    (7, 3, 2048, 2, (1, 3)),                                     # the last row belongs to no stripe
    (8, 4, 2048, 3, (1, 3, 129)),                                # two rows dropped
    (8, 4, 2048, 8, (1, 3)),                                     # one-row stripes
    (2, 1, 64, 2, (1, 3)), (1, 1, 8, 1, (1, 3)), (1, 1, 4, 1, (1,)), (8, 4, 2048, 0, (3,)),
]


def _gap_ref(x64, S):
    """oracle/embed_oracle.pooled on the NCHW float64 map -> [nsets, B, C], and mean|x| over the same windows"""
    from oracle import embed_oracle
    p = embed_oracle.pooled(x64.permute(0, 3, 1, 2), S)
    a = embed_oracle.pooled(x64.abs().permute(0, 3, 1, 2), S)
    return (torch.stack(p), torch.stack(a)) if isinstance(p, list) else (p[None], a[None])


@pytest.mark.parametrize("H,W,C,S,batches", GAP_CASES)
def test_gap_stripes(H, W, C, S, batches, L, dev):
    from ssg_amd.resnet import _h8l8
    nsets = S + 1 if S > 1 else 1
    worst = 0.0
    for B in batches:
        for name in ("rows", "ones"):
            if name == "rows":
                x = _row_scaled(B, H, W, C, 10 * H + S + B)
                x[0, 0, 0, :] *= 1e-4
            else:
                x = torch.ones(B, H, W, C)
            x = _decoded(x)                                                          # the same values for the fp32 and the split-half kernel
            ref, mean_abs = _gap_ref(x.double(), S)
            assert ref.shape == (nsets, B, C)
            n = torch.tensor([H * W] + ([H // S * W] * S if S > 1 else []), dtype=torch.float64).view(nsets, 1, 1)
            bound = (n + 1) * U * mean_abs
            out = torch.full((nsets + 1, B, C), 7.0, device=dev)                     # one set more: nothing may be written behind the last
            _call(L.ssg_gap_stripes, x.to(dev), out, B, H, W, C, S)
            assert bool((out[nsets] == 7.0).all())
            got = out[:nsets].cpu()
            ratio = float(((got.double() - ref).abs() / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, B, ratio)
            if name == "ones":
                assert bool((got == 1.0).all()), "a map of ones must pool to exactly 1.0f in every set"
            if C % 8 == 0:
                outs = torch.full((nsets + 1, B, C), 7.0, device=dev)
                _call(L.ssg_gap_stripes_h8l8, _h8l8(x.view(-1, C)).to(dev), outs, B, H, W, C, S)
                assert bool((outs[nsets] == 7.0).all())
                assert _same_bits(outs[:nsets], out[:nsets]), "the split-half pool sums hi + lo in the fp32 pool's order: same bits"
    print("gap-stripes-error: H %2d W %d C %4d S %d  worst |got - ref| / ((n + 1) u mean|x|) = %.3f" % (H, W, C, S, worst))


def test_gap_stripes_refuses_more_stripes_than_rows(L):
    for fn in (L.ssg_gap_stripes, L.ssg_gap_stripes_h8l8):
        assert fn(None, None, 2, 2, 1, 64, 3, None) == INVALID and b"bad shape" in L.ssg_last_error()
        assert fn(None, None, 2, 7, 3, 64, 8, None) == INVALID
        assert fn(None, None, 0, 8, 4, 64, 2, None) == INVALID
    assert L.ssg_gap_stripes_h8l8(None, None, 2, 8, 4, 68, 2, None) == INVALID       # C % 8


# ------------------------------------------------------------------ (a + b) / ||a + b||
@pytest.mark.parametrize("rows,C", [(1, 1), (3, 63), (3, 64), (5, 100), (7, 2048), (4, 6144), (1000, 2048)])
def test_flip_sum_l2norm(rows, C, L, dev):
    g = torch.Generator().manual_seed(rows + C)
    a = torch.randn(rows, C, generator=g) * (1.0 + torch.arange(rows).float()).view(rows, 1)
    b = a + 0.3 * torch.randn(rows, C, generator=g)
    zero_row = cancel_row = None
    if rows >= 3:
        zero_row, cancel_row = 1, 2
        a[zero_row] = 0.0; b[zero_row] = 0.0                                         # x / x.norm() of a zero row: NaN everywhere
        b[cancel_row] = -a[cancel_row]; b[cancel_row, C // 2] = a[cancel_row, C // 2] + 0.75     # a + b exactly zero in all but one column
    out = torch.full((rows + 1, C), 7.0, device=dev)
    _call(L.ssg_flip_sum_l2norm, a.to(dev), b.to(dev), out, rows, C)
    assert bool((out[rows] == 7.0).all())
    got = out[:rows].cpu()
    s = a.double() + b.double()
    ref = s / s.norm(dim=1, keepdim=True)
    keep = torch.ones(rows, dtype=torch.bool)
    if zero_row is not None:
        assert bool(torch.isnan(got[zero_row]).all()) and bool(torch.isnan(ref[zero_row]).all())
        keep[zero_row] = False
        want = torch.zeros(C); want[C // 2] = 1.0 if float(s[cancel_row, C // 2]) > 0 else -1.0
        assert torch.equal(got[cancel_row], want)
    got, ref = got[keep].double(), ref[keep]
    assert bool(torch.isfinite(got).all())
    rel = ((C + 63) // 64 + 6 + 4) * U
    bound = rel * ref.abs() + U * ref.abs().amax(dim=1, keepdim=True)
    ratio = float(((got - ref).abs() / bound).max())
    print("flip-sum-l2norm-error: rows %4d C %4d  worst |got - ref| / bound = %.3f  (relative constant %d u)" % (rows, C, ratio, (C + 63) // 64 + 10))
    assert ratio <= 1.0
    assert L.ssg_flip_sum_l2norm(None, None, None, 0, 8, None) == INVALID and L.ssg_flip_sum_l2norm(None, None, None, 4, 0, None) == INVALID


# ------------------------------------------------------------------ conv3 | downsample as one fp32 GEMM
@pytest.mark.parametrize("H2,W2,s2,H,W", [(63, 25, 2, 32, 13), (7, 3, 2, 4, 2)])
@pytest.mark.parametrize("Cin,Cin2,Cout,stride1", [(128, 256, 512, False), (256, 512, 1024, False), (512, 1024, 2048, False), (64, 64, 256, True)])
def test_conv1x1_dual_nhwc_f32_on_odd_maps(Cin, Cin2, Cout, stride1, H2, W2, s2, H, W, L, dev):
    """relu(o @ w3^T + x[:, ::s, ::s] @ wd^T + bias) on the fp32 matrix cores: the channel layouts of
    test_conv_dual_tile_shapes_agree_bitwise (tests/test_gpu_parity.py) at B = 2 with the odd maps a 250 x 100 or 200 x 72 input gives
    the stride-2 blocks (the last sampled row / column is the map's last); the stride-1 layout (layer1's first block) samples every
    pixel of an H x W map.  Tolerance: test_conv_vs_torch's for this path."""
    B = 2
    if stride1:
        H2, W2, s2 = H, W, 1
    g = torch.Generator().manual_seed(Cin + Cout + H2)
    o = torch.randn(B, H, W, Cin, generator=g)
    x = torch.randn(B, H2, W2, Cin2, generator=g) * (1.0 + torch.arange(H2).float()).view(1, H2, 1, 1) / H2     # a wrong sampled row is not a tolerance question
    w3 = torch.randn(Cout, Cin, generator=g) * (1.0 / Cin) ** 0.5
    wd = torch.randn(Cout, Cin2, generator=g) * (1.0 / Cin2) ** 0.5
    bias = torch.randn(Cout, generator=g)
    out = torch.full((B + 1, H, W, Cout), 7.0, device=dev)
    _call(L.ssg_conv1x1_dual_nhwc_f32, o.to(dev), x.to(dev), torch.cat([w3, wd], 1).contiguous().to(dev), bias.to(dev), out, B, H, W, Cin, H2, W2, Cin2, s2, Cout, 1)
    assert bool((out[B] == 7.0).all())
    xs = x[:, ::s2, ::s2]
    assert xs.shape[1:3] == (H, W)
    ref = torch.relu(torch.einsum("bhwc,oc->bhwo", o.double(), w3.double()) + torch.einsum("bhwc,oc->bhwo", xs.double(), wd.double()) + bias.double())
    err = float((out[:B].cpu().double() - ref).abs().max())
    assert err < 2e-5 * max(1.0, float(ref.abs().max())), err
    # a sampling grid that leaves the second map is refused
    assert L.ssg_conv1x1_dual_nhwc_f32(None, None, None, None, None, B, H + 1, W, Cin, H2, W2, Cin2, s2, Cout, 1, None) == INVALID
