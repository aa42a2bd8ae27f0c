"""GPU suite (-m gpu): the split-half codec of csrc/ssg_common.h (split_encode4 / split_decode4) through ssg_h8l8_encode and
ssg_h8l8_decode, against its numpy statement

    hi = float16(v)      lo = float16(v - float32(hi))      decode = float32(float32(hi) + float32(lo))

with a power-of-two scale of 1 and 2^-3 (encode: v = in * scale; decode: out = (hi + lo) * scale).  Every comparison is equality of
the uint16 / uint32 patterns.  The inputs are the ones on which a codec built from packed or mixed-precision instructions could differ
from one built from scalar conversions: every finite half as hi with its float32 neighbours and the ties half an ulp away, +-0, float32
denormals, lo halves that are subnormal or round to zero (40 % of the lo halves of |N(0, 1)| activations are subnormal halves), the
edge of the half range, inf and NaN, and 2^20 random magnitudes over 36 binades.

NaN: IEEE 754 fixes neither the sign nor the payload of the NaN that inf - inf gives (the lo half of an infinite value) and hosts differ
from the GPU there, so as in test_gpu_embed_layers.py any NaN equals any NaN; everything else, +-0 and +-inf included, is bit for bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SCALES = [1.0, 0.125]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    from ssg_amd import _lib
    return _lib.lib()


def _pad8(a, fill):
    return np.concatenate([a, np.full((-a.size) % 8, fill, a.dtype)])


@pytest.fixture(scope="module")
def values():
    """float32 inputs of the encoder (a multiple of 8 of them)"""
    rng = np.random.default_rng(20240817)
    allh = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    fin = allh[(allh & 0x7c00) != 0x7c00]
    assert fin.size == 63488
    h = fin.view(np.float16)
    v = h.astype(np.float32)
    with np.errstate(over="ignore"):                                           # (the spacing above 65504 is infinite: v +- inf is tested too)
        half_ulp = np.abs(np.spacing(h)).astype(np.float32) * np.float32(0.5)  # exact: at least 2^-25
    inf = np.float32(np.inf)
    parts = [v, np.nextafter(v, inf), np.nextafter(v, -inf), v + half_ulp, v - half_ulp]
    parts.append(np.array([0.0, -0.0, 65504.0, 65519.99, 65520.0, 65536.0, np.inf, np.nan], np.float32))
    parts.append(-parts[-1])
    den = np.concatenate([np.arange(1, 65, dtype=np.uint32), np.arange(0x7fffc0, 0x800040, dtype=np.uint32),
                          rng.integers(1, 0x800000, 4096).astype(np.uint32)])
    parts += [den.view(np.float32), (den | 0x80000000).view(np.float32)]
    # lo a subnormal half, or rounding to 0: t around 2^-24 (the smallest half) and 2^-25 (its tie with 0), alone and on top of a hi
    t = np.concatenate([(np.float32(c).view(np.uint32) + np.arange(-64, 65)).astype(np.uint32).view(np.float32)
                        for c in (2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.0 ** -14, 2.0 ** -15)])
    t = np.concatenate([t, -t])
    parts.append(t)
    for c in (2.0 ** -14, 2.0 ** -12, 2.0 ** -10, 3.0 * 2.0 ** -11, -(2.0 ** -10)):
        parts.append(np.float32(c) + t)
    k = rng.integers(-20, 16, 1 << 20)
    parts.append(np.ldexp(np.abs(rng.standard_normal(1 << 20)), k).astype(np.float32))
    return _pad8(np.concatenate(parts).astype(np.float32), np.float32(0))


@pytest.fixture(scope="module")
def pairs():
    """(hi, lo) half patterns of the decoder: 4096 random hi x the lo patterns around 0, the subnormal / normal boundary and the top"""
    rng = np.random.default_rng(5)
    hi = rng.integers(0, 65536, 4096).astype(np.uint16)
    lo = np.concatenate([np.arange(0, 64), np.arange(0x0400 - 32, 0x0400 + 32), np.arange(0x7c00 - 32, 0x7c00 + 32)])
    lo = np.concatenate([lo, lo | 0x8000]).astype(np.uint16)
    H, Lo = np.meshgrid(hi, lo, indexing="ij")
    return _pad8(H.ravel(), np.uint16(0)), _pad8(Lo.ravel(), np.uint16(0))


def _canon16(b):
    b = b.astype(np.uint16)
    return np.where((b & 0x7fff) > 0x7c00, np.uint16(0x7e00), b)


def _canon32(b):
    b = b.astype(np.uint32)
    return np.where((b & 0x7fffffff) > 0x7f800000, np.uint32(0x7fc00000), b)


def _report(what, got, ref):
    bad = np.flatnonzero(got != ref)
    if bad.size:
        print("%s: %d of %d differ; first at %d: got %#x ref %#x" % (what, bad.size, got.size, bad[0], got[bad[0]], ref[bad[0]]))
    return bad.size == 0


@pytest.mark.parametrize("scale", SCALES)
def test_encode_bits(scale, values, L, dev):
    from ssg_amd._lib import check, ptr, stream
    with np.errstate(invalid="ignore", over="ignore"):
        v = values * np.float32(scale)
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    x = torch.from_numpy(values).to(dev)
    enc = torch.empty_like(x)
    check(L.ssg_h8l8_encode(ptr(x), ptr(enc), x.numel(), float(scale), stream()), "ssg_h8l8_encode")
    got = enc.cpu().numpy().view(np.uint16).reshape(-1, 16)
    assert int(np.count_nonzero((lo.view(np.uint16) & 0x7c00) == 0)) > values.size // 4, "few subnormal lo halves in the inputs"
    ok_hi = _report("hi", _canon16(got[:, :8].ravel()), _canon16(hi.view(np.uint16)))
    ok_lo = _report("lo", _canon16(got[:, 8:].ravel()), _canon16(lo.view(np.uint16)))
    assert ok_hi and ok_lo


@pytest.mark.parametrize("scale", SCALES)
def test_decode_bits(scale, pairs, L, dev):
    from ssg_amd._lib import check, ptr, stream
    hi, lo = pairs
    with np.errstate(invalid="ignore", over="ignore"):
        ref = (hi.view(np.float16).astype(np.float32) + lo.view(np.float16).astype(np.float32)) * np.float32(scale)
    cont = np.concatenate([hi.reshape(-1, 8), lo.reshape(-1, 8)], axis=1)
    enc = torch.from_numpy(cont.view(np.float32).reshape(-1).copy()).to(dev)
    out = torch.empty_like(enc)
    check(L.ssg_h8l8_decode(ptr(enc), ptr(out), enc.numel(), float(scale), stream()), "ssg_h8l8_decode")
    assert _report("decode", _canon32(out.cpu().numpy().view(np.uint32)), _canon32(ref.view(np.uint32)))


def test_round_trip_of_the_encoder_inputs(values, L, dev):
    """decode(encode(v)) against the numpy statement of both, on the encoder's inputs (the decoder then sees the lo halves real
    values have, next to the synthetic pairs above)"""
    from ssg_amd._lib import check, ptr, stream
    with np.errstate(invalid="ignore", over="ignore"):
        hi = values.astype(np.float16)
        lo = (values - hi.astype(np.float32)).astype(np.float16)
        ref = hi.astype(np.float32) + lo.astype(np.float32)
    x = torch.from_numpy(values).to(dev)
    enc, out = torch.empty_like(x), torch.empty_like(x)
    check(L.ssg_h8l8_encode(ptr(x), ptr(enc), x.numel(), 1.0, stream()), "ssg_h8l8_encode")
    check(L.ssg_h8l8_decode(ptr(enc), ptr(out), x.numel(), 1.0, stream()), "ssg_h8l8_decode")
    assert _report("round trip", _canon32(out.cpu().numpy().view(np.uint32)), _canon32(ref.view(np.uint32)))
