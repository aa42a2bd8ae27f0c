"""GPU suite (-m gpu): the float32 distance GEMMs (csrc/conv.hip: the non-DMA fp32 instantiation of the convolution GEMM with the epilogues
epi == 1, `ssg_pairwise_sqdist_f32`, and epi == 2, `ssg_cosine_dist_f32`) through their C entry points, at the sizes an evaluation and
the SSG++ label step run them at: 3368 x 15 936 at d = 2048 / 8192 (128 x 64 tile), the stacked 19 281 -> 19 328 self and cosine forms
(128 x 128 tile), an output above 4 GiB, a y operand above 4 GiB, every m % 128 in {1, 127, 0, 1}, operands that are views into a
NaN-filled allocation.  `out` and `ws` are NaN before every call; every element of out[:m, :n] must be finite afterwards.

Reference: the same formula (|x|^2 + |y|^2 - 2 x.y, 2 |x|^2 - 2 x.y, 2 - 2 x.y) in float64 on the CPU from the same float32 inputs
(oracle.ssg_oracle.sqdist_f64) -- on whole matrices for the small shapes, on sampled rows x columns for the large ones.  A sample
holds row 0, row m - 1 and the first and last row of the first, a middle and the last 128-row tile, a seeded draw, and the same for the
columns with the tile width actually launched (128 if n % 128 == 0, else 64); the zero rows that pad y are columns like any other
(expected: the row term, or 2).

Tolerance (the rule of test_gpu_fused_blocks.py):  err <= 4 * e32 + 2^-21 * max(1, |ref|max), with e32 the largest error, against that
float64 reference and on the same elements, of the reference project's own arithmetic -- torch float32 on the CPU, the expressions of
reid/evaluators.py:63-85 and rerank.py:182 (oracle.ssg_oracle.sqdist_f32_reference).  e32 is computed per case inside the test; nothing in the
bound comes from the kernel.  Every case prints one `dist-f32-error` line (pytest -s); profiles/dist_f32_errors.txt is such a log.
The squared forms run on rows of individually varying norm (_varied: a seeded factor in [0.5, 2] per row, around 1 and around the scale
of the embedder's un-normalised outputs), so that every row term and column term is a number of its own: a term read at the wrong row,
column or tile is an error of the size of the value.  Measured on an MI355X over the 167 whole-matrix / sampled lines: err / bound at
most 0.96 (the stacked self form on varied norms at the embedder's scale; err / e32 7.6 there, carried by the 2^-21 |ref|max term).

One check needs more than the factor 4: the elements whose x row IS the y row (unit norm), judged alone -- reference 0, so |ref|max grants
nothing beyond 2^-21 and the whole value is summation-order noise of a sum of d squares.  The GEMM gives ONE accumulator all d / 2
v_mfma_f32_32x32x2 steps in sequence: at d = 2048 a chain of 1024 additions of positive terms whose running sum grows to 1, against the
lane-split, blocked sums of a CPU BLAS (chains of d / 16 = 128 or shorter); a rounding random walk 8 times as long is sqrt(8) = 2.8
times as wide, and |x|^2 + |y|^2 - 2 x.y adds the norm kernel's own order (64 lanes x d / 64 terms, then a tree) on top.  The maximum
over a few hundred such elements has no headroom left in a factor 4 that was set for values with a |ref|max to lean on, so these
elements get twice the factor: DUP_FACTOR = 8.  Measured on an MI355X with the factor 4, 257 elements at d = 2048: squared form err
3.815e-06 (16 ulp of 2.0), e32 5.215e-07, err / e32 7.31, factor needed 6.4; cosine form err 3.765e-06, e32 8.097e-07, err / e32 4.65, factor
needed 4.06.  The same elements inside their whole matrix (|ref|max 2.2) hold the factor 4 (err / bound 0.78), as do the 30 sampled
diagonal elements of the stacked 19 281-row case (err / bound 0.75 and 0.67).

Bit identity: a row's result depends neither on the number of rows of the call nor on the tile the row falls in, and a repeated call
returns the same bits.  `pairwise_distance_device` returns the direct call's bits; ssg_amd.ranking on that device matrix equals
oracle/eval_oracle.py on its host copy for all 3368 queries (the Python oracle takes about half a minute for them).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NAN = float("nan")
FORMS = {0: "sqdist", 1: "sqdist-self", 2: "cosine"}
DUP_FACTOR = 8.0             # x rows that are y rows, judged alone against 0: see the module docstring
EMBED_SCALE = 0.3            # element std of the un-normalised embedder outputs of tests/golden/pairwise.npz, tag r (row norm 13.6 at d = 2048)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    from ssg_amd import _lib
    return _lib.lib()


def _run(L, form, x, y, m=None, out=None):
    """one direct call on x [m, d], y [n, d] (n % 64 == 0): NaN-filled out [m, n] and ws, then the entry point of `form`"""
    from ssg_amd._lib import check, ptr, stream
    m = x.shape[0] if m is None else m
    n, d = y.shape
    assert x.is_contiguous() and y.is_contiguous() and x.shape[1] == d
    if out is None:
        out = torch.full((m, n), NAN, dtype=torch.float32, device=x.device)
    if form == 2:
        zeros = torch.zeros(n, dtype=torch.float32, device=x.device)
        check(L.ssg_cosine_dist_f32(ptr(x), ptr(y), m, n, d, ptr(zeros), ptr(out), stream()), "ssg_cosine_dist_f32")
    else:
        ws = torch.full((m + n,), NAN, dtype=torch.float32, device=x.device)
        check(L.ssg_pairwise_sqdist_f32(ptr(x), ptr(y), m, n, d, form, ptr(ws), ptr(out), stream()), "ssg_pairwise_sqdist_f32")
    torch.cuda.synchronize()
    return out


def _sample(count, tile, extra, seed, tail=0):
    """0, count - 1, the first and last index of the first, a middle and the last tile, `extra` seeded draws, the last `tail` indices"""
    nt = (count + tile - 1) // tile
    s = {0, count - 1}
    for t in (0, nt // 2, nt - 1):
        s.add(min(t * tile, count - 1)); s.add(min(t * tile + tile - 1, count - 1))
    s.update(int(v) for v in np.random.default_rng(seed).integers(0, count, extra))
    s.update(range(max(count - tail, 0), count))
    return np.array(sorted(s), dtype=np.int64)


def _bound(got, ref64, ref32, factor=4.0):
    err = float(np.abs(got - ref64).max())
    e32 = float(np.abs(ref32.astype(np.float64) - ref64).max())
    scale = max(1.0, float(np.abs(ref64).max()))
    return err, e32, scale, factor * e32 + 2.0 ** -21 * scale


def _report(tag, form, shape, got, ref64, ref32, factor=4.0):
    """print the case's `dist-f32-error` line, then assert the bound of the module docstring -> max(1, |ref|max)"""
    err, e32, scale, bound = _bound(got, ref64, ref32, factor)
    print("dist-f32-error: %-34s %-11s m %6d n %6d d %5d  elements %9d  err %.3e  e32 %.3e  err/e32 %6.2f  |ref|max %9.3e  bound %.3e  err/bound %.3f"
          % ((tag, FORMS[form]) + tuple(shape) + (got.size, err, e32, err / e32 if e32 else float("inf"), scale, bound, err / bound)))
    assert np.isfinite(got).all() and err <= bound, (tag, FORMS[form], err, e32, bound)
    return scale


def _judge(tag, form, out, x, y, rows=None, cols=None):
    """all of out finite, the (sampled) elements within the bound of the module docstring"""
    from oracle import ssg_oracle as ora
    m, n = out.shape
    assert bool(torch.isfinite(out).all()), (tag, "non-finite output")
    if rows is None:
        got = out.cpu().numpy().astype(np.float64); xs = x[:m].cpu().numpy(); ys = y.cpu().numpy()
    else:
        r = torch.from_numpy(rows).to(out.device); c = torch.from_numpy(cols).to(out.device)
        got = out[r][:, c].cpu().numpy().astype(np.float64); xs = x[r].cpu().numpy(); ys = y[c].cpu().numpy()
    ref64 = ora.sqdist_f64(xs, ys, form); ref32 = ora.sqdist_f32_reference(xs, ys, form)
    _report(tag, form, (m, n, x.shape[1]), got, ref64, ref32)
    return got, ref64, ref32


def _unit(rows, d, seed, dev, scale=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn((rows, d), generator=g, device=dev, dtype=torch.float32)
    x /= x.norm(dim=1, keepdim=True)
    return x * scale if scale != 1.0 else x


def _varied(rows, d, seed, dev, scale=1.0):
    """rows of individually different norm: unit rows times a seeded factor in [0.5, 2] (log-uniform) times `scale` -- |x_i|^2 spans 16 x
    within every tile, so a row or column term taken from the wrong row, column or tile is an error of the order of the value itself"""
    g = torch.Generator(device=dev).manual_seed(seed + 500000)
    f = torch.exp2(2.0 * torch.rand((rows, 1), generator=g, device=dev, dtype=torch.float32) - 1.0)
    return (_unit(rows, d, seed, dev) * (f * scale)).contiguous()


def _padded(y, n):
    """y followed by zero rows up to n (what the Python wrappers hand the entry points)"""
    return torch.nn.functional.pad(y, (0, 0, 0, n - y.shape[0])).contiguous()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------ small shapes, whole matrices
@pytest.mark.parametrize("d", [32, 224, 2048])
def test_small_shapes_whole_matrix(L, dev, d):
    """m in {1, 127, 128, 129} x n in {64, 128, 192, 1152} (both tile widths, one and several column tiles, the row remainders 1 / 127 / 0 / 1)
    x the three forms, d / 16 = 2, 14, 128.  The last three rows of y are zero padding.  The squared forms run on rows of individually
    varying norm (_varied), alternately around 1 and around the embedder's scale; the cosine form runs on unit rows."""
    case = 0
    for n in (64, 128, 192, 1152):
        for m in (1, 127, 128, 129):
            for form in (0, 1, 2):
                case += 1
                scale = 1.0 if (form == 2 or case % 2) else EMBED_SCALE * d ** 0.5
                make = _unit if form == 2 else _varied
                x = make(m, d, 1000 + case, dev, scale)
                y = _padded(make(n - 3, d, 2000 + case, dev, scale), n)
                out = _run(L, form, x, y)
                got, _, _ = _judge("small", form, out, x, y)
                pad = got[:, n - 3:]                       # the padded columns: the row term (|x|^2 or 2 |x|^2), or 2, in every column alike
                assert np.array_equal(pad, np.repeat(pad[:, :1], 3, axis=1)), (m, n, d, form)


# ------------------------------------------------------------------ evaluation sizes
@pytest.fixture(scope="module")
def market(dev):
    """3368 queries x 15 913 gallery rows (padded to 15 936 = 64 * 249: the 128 x 64 tile), d = 2048, unit norm; ids and cameras of a
    Market-1501-like split (751 identities, 6 cameras), features clustered by identity so that the ranking means something"""
    rng = np.random.default_rng(77)
    m, n, d, nid = 3368, 15913, 2048, 751
    gid = rng.integers(0, nid, n).astype(np.int32); gcam = rng.integers(0, 6, n).astype(np.int32)
    qid = rng.integers(0, nid, m).astype(np.int32); qcam = rng.integers(0, 6, m).astype(np.int32)
    g = torch.Generator(device=dev).manual_seed(78)
    c = torch.randn((nid, d), generator=g, device=dev); c /= c.norm(dim=1, keepdim=True)

    def feats(ids):
        f = c[torch.from_numpy(ids.astype(np.int64)).to(dev)] + 1.2 / d ** 0.5 * torch.randn((len(ids), d), generator=g, device=dev)
        return (f / f.norm(dim=1, keepdim=True)).contiguous()
    return dict(x=feats(qid), y=feats(gid), qid=qid, gid=gid, qcam=qcam, gcam=gcam, n=n, npad=15936)


def test_market_evaluation_block(L, dev, market):
    """the query x gallery block of a Market-1501 evaluation: d = 2048 twice (bit-identical), and the same rows un-normalised: at the
    embedder's scale, every row with a norm of its own (a factor in [0.5, 2])"""
    x, y = market["x"], _padded(market["y"], market["npad"])
    m, n = x.shape[0], y.shape[0]
    rows, cols = _sample(m, 128, 24, 1), _sample(n, 64, 192, 2, tail=64)
    out = _run(L, 0, x, y)
    _judge("market unit", 0, out, x, y, rows, cols)
    assert _same_bits(out, _run(L, 0, x, y)), "two runs of the same call differ"
    del out
    g = torch.Generator(device=dev).manual_seed(79)
    xs = x * (EMBED_SCALE * 2048 ** 0.5 * torch.exp2(2.0 * torch.rand((m, 1), generator=g, device=dev) - 1.0))
    ys = y * (EMBED_SCALE * 2048 ** 0.5 * torch.exp2(2.0 * torch.rand((n, 1), generator=g, device=dev) - 1.0))     # (its zero rows stay zero)
    _judge("market embedder-scale", 0, _run(L, 0, xs, ys), xs, ys, rows, cols)


def test_market_evaluation_block_stripes(L, dev):
    """3368 x 15 936 at d = 8192 (global + stripe features): 512 k-tiles of 16; rows of varying norm"""
    x = _varied(3368, 8192, 5, dev); y = _padded(_varied(15913, 8192, 6, dev), 15936)
    _judge("market stripes", 0, _run(L, 0, x, y), x, y, _sample(3368, 128, 24, 3), _sample(15936, 64, 192, 4, tail=64))


def test_stacked_self_and_cosine_forms(L, dev):
    """[query; gallery] stacked: N = 19 281 rows against themselves padded to 19 328 = 128 * 151 (the 128 x 128 tile); self_form = 1 and
    the cosine form.  The diagonal holds duplicate rows (x_i = y_i): both forms must stay within the bound of 0 there, never NaN."""
    from oracle import ssg_oracle as ora
    N, npad, d = 19281, 19328, 2048
    x = _unit(N, d, 9, dev); y = _padded(x, npad)
    rows, cols = _sample(N, 128, 24, 5), _sample(npad, 128, 192, 6, tail=64)
    for form in (1, 2):
        out = _run(L, form, x, y)
        _judge("stacked", form, out, x, y, rows, cols)
        diag = out.diagonal()[:N][torch.from_numpy(rows).to(dev)].cpu().numpy().astype(np.float64)
        xs = x[torch.from_numpy(rows).to(dev)].cpu().numpy()
        ref64 = np.diagonal(ora.sqdist_f64(xs, xs, form)); ref32 = np.diagonal(ora.sqdist_f32_reference(xs, xs, form))
        assert _report("stacked diagonal (duplicates)", form, (N, npad, d), diag, ref64, ref32) == 1.0
        del out
    # the self form again on rows of varying norm: 151 row tiles x 151 column tiles, each row with a row term of its own
    x = _varied(N, d, 10, dev, EMBED_SCALE * d ** 0.5); y = _padded(x, npad)
    _judge("stacked varied norms", 1, _run(L, 1, x, y), x, y, rows, cols)


def test_duplicate_rows_between_x_and_y(L, dev):
    """x rows that are rows of y (a query image that is also in the gallery): |x|^2 + |y|^2 - 2 x.y and 2 - 2 x.y cancel to 0 within the
    bound on unit rows, and are never NaN; rows of the embedder's scale are judged with the whole matrix (|ref|max of the matrix)."""
    from oracle import ssg_oracle as ora
    m, n, d = 257, 1152, 2048
    for scale_in in (1.0, EMBED_SCALE * d ** 0.5):
        y = _padded((_unit if scale_in == 1.0 else _varied)(n - 5, d, 31, dev, scale_in), n)
        idx = torch.from_numpy(np.random.default_rng(32).permutation(n - 5)[:m]).to(dev)
        x = y[idx].contiguous()
        for form in ((0, 2) if scale_in == 1.0 else (0,)):
            out = _run(L, form, x, y)
            _judge("duplicates scale %.3g" % scale_in, form, out, x, y)
            dup = out[torch.arange(m, device=dev), idx].cpu().numpy().astype(np.float64)
            assert np.isfinite(dup).all()
            if scale_in == 1.0:
                xs = x.cpu().numpy()
                ref64 = np.diagonal(ora.sqdist_f64(xs, xs, form)); ref32 = np.diagonal(ora.sqdist_f32_reference(xs, xs, form))
                assert _report("duplicate elements alone", form, (m, n, d), dup, ref64, ref32, factor=DUP_FACTOR) == 1.0


# ------------------------------------------------------------------ 64-bit offsets
@pytest.mark.parametrize("m,n", [(33000, 33024), (46400, 46464)])
def test_output_above_4gib(L, dev, m, n):
    """33 000 x 33 024 floats = 4.36 GB of output at d = 32: byte offsets above 2^32; 46 400 x 46 464 = 2.156e9 elements: element offsets above
    2^31 as well (a 32-bit m * n).  The sample holds the last row and the last column, and every element must have been written."""
    d = 32
    x = _varied(m, d, 41, dev, 3.0); y = _padded(_varied(n - 7, d, 42, dev, 3.0), n)
    rows, cols = _sample(m, 128, 40, 7), _sample(n, 128, 192, 8, tail=64)
    assert rows[-1] == m - 1 and cols[-1] == n - 1 and (m - 1) * n * 4 > 2 ** 32 and (m * n > 2 ** 31 or m < 40000)
    for form in (0, 2):
        xx, yy = (x, y) if form == 0 else (x / x.norm(dim=1, keepdim=True), _padded(y[:n - 7] / y[:n - 7].norm(dim=1, keepdim=True), n))
        out = _run(L, form, xx, yy)
        _judge("output > 4 GiB", form, out, xx, yy, rows, cols)
        del out


def test_y_above_4gib(L, dev):
    """y = 140 096 x 8192 floats = 4.59 GB (only m * d * 4 is limited): the 64-bit pointer arithmetic of the y tile loads.  n = 140 096 =
    64 * 2189 runs on the 128 x 64 tile, its first 140 032 = 128 * 1094 rows on the 128 x 128 tile; the sample holds the last 64 columns."""
    m, d, n = 128, 8192, 140096
    x = _unit(m, d, 51, dev)
    y = _unit(n, d, 52, dev)
    y[n - 9:] = 0
    xv = x * torch.exp2(torch.linspace(-1.0, 1.0, m, device=dev)).view(m, 1)            # the squared form: norms that differ from row to row
    y[1::2] *= 1.5; y[::3] *= 0.5                                                        # and from column to column (also the cosine form's y)
    assert y.numel() * 4 > 2 ** 32
    rows = _sample(m, 128, 30, 9)
    for nn, tile in ((n, 64), (140032, 128)):
        yy = y[:nn]
        cols = _sample(nn, tile, 256, 10, tail=64)
        assert set(range(nn - 64, nn)) <= set(cols.tolist())
        for form in (0, 2):
            xx = xv if form == 0 else x
            out = _run(L, form, xx, yy)
            _judge("y > 4 GiB", form, out, xx, yy, rows, cols)
            del out


def test_views_inside_a_nan_allocation(L, dev):
    """x, y, ws-free out: views that start at a non-zero, 16-byte aligned offset inside one allocation whose every other float is NaN.  A read
    outside x or y would bring a NaN into the result; a write outside out would remove one from the surroundings."""
    m, n, d = 129, 192, 224
    for form in (0, 1, 2):
        buf = torch.full((4 + m * d + 12 + n * d + 8,), NAN, dtype=torch.float32, device=dev)
        x = buf[4:4 + m * d].view(m, d); y = buf[4 + m * d + 12:4 + m * d + 12 + n * d].view(n, d)
        assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0 and x.data_ptr() != buf.data_ptr()
        make = _varied if form < 2 else _unit
        x.copy_(make(m, d, 61 + form, dev)); y.copy_(_padded(make(n - 2, d, 71 + form, dev), n))
        obuf = torch.full((8 + m * n + 8,), NAN, dtype=torch.float32, device=dev)
        out = obuf[8:8 + m * n].view(m, n)
        _run(L, form, x, y, out=out)
        _judge("views", form, out, x, y)
        assert bool(torch.isnan(obuf[:8]).all()) and bool(torch.isnan(obuf[8 + m * n:]).all()), "wrote outside out"
        assert bool(torch.isnan(buf[:4]).all()) and bool(torch.isnan(buf[4 + m * d:4 + m * d + 12]).all()) and bool(torch.isnan(buf[-8:]).all())


# ------------------------------------------------------------------ bit identity
def test_rows_do_not_depend_on_the_call_shape(L, dev, market):
    """a call at 3368 rows equals, bit for bit on its first rows, the call at 1000 rows, and equals two stacked calls split at row 1531
    (neither a multiple of 128): a row's result may not depend on the tile or the call it falls in"""
    xu, yu = market["x"], _padded(market["y"], market["npad"])
    g = torch.Generator(device=dev).manual_seed(80)
    xv = xu * torch.exp2(2.0 * torch.rand((xu.shape[0], 1), generator=g, device=dev) - 1.0)
    yv = yu * torch.exp2(2.0 * torch.rand((yu.shape[0], 1), generator=g, device=dev) - 1.0)
    for form in (0, 1, 2):
        x, y = (xu, yu) if form == 2 else (xv, yv)
        full = _run(L, form, x, y)
        assert _same_bits(full[:1000], _run(L, form, x[:1000], y)), FORMS[form]
        assert _same_bits(full[:1], _run(L, form, x[:1], y)), FORMS[form]
        top, bottom = _run(L, form, x[:1531], y), _run(L, form, x[1531:], y)
        assert _same_bits(full, torch.cat([top, bottom], 0)), FORMS[form]
        del full, top, bottom


# ------------------------------------------------------------------ the Python surface
def test_pairwise_distance_device_and_ranking_at_market_size(L, dev, market):
    """`pairwise_distance_device` on the Market case returns the direct call's bits; `ssg_amd.ranking.per_query` / `cmc` on that device
    matrix (ssg_rank_metrics, ssg_rank_metrics_all at 3368 x 15 913, row pitch 15 936) equal oracle/eval_oracle.py on the host copy of the same
    matrix: first ranks and both CMC curves exactly, AP within 1e-12.  All 3368 queries."""
    from collections import OrderedDict
    import ssg_amd
    from ssg_amd import ranking
    from ssg_amd._lib import check, ptr, stream
    from oracle import eval_oracle
    x, y, n = market["x"], market["y"], market["n"]
    qid, gid, qcam, gcam = market["qid"], market["gid"], market["qcam"], market["gcam"]
    m = x.shape[0]
    feats = OrderedDict(("q%05d" % i, t) for i, t in enumerate(x.unbind(0)))
    feats.update(("g%05d" % i, t) for i, t in enumerate(y.unbind(0)))
    query = [("q%05d" % i, int(qid[i]), int(qcam[i])) for i in range(m)]
    gallery = [("g%05d" % i, int(gid[i]), int(gcam[i])) for i in range(n)]
    from ssg_amd.evaluators import pairwise_distance_device
    dist = pairwise_distance_device(feats, query, gallery)
    direct = _run(L, 0, x, _padded(y, market["npad"]))
    assert dist.shape == (m, n) and dist.is_cuda and _same_bits(dist, direct[:, :n])
    host = dist.cpu().numpy()
    first, ap = ranking.per_query(dist, qid, gid, qcam, gcam)
    ofirst, oap = eval_oracle.per_query(host, qid, gid, qcam, gcam)
    assert np.array_equal(first.cpu().numpy(), ofirst) and (ofirst >= 0).sum() > 3000
    assert np.array_equal(np.isnan(ap.cpu().numpy()), np.isnan(oap)) and np.nanmax(np.abs(ap.cpu().numpy() - oap)) < 1e-12
    assert np.array_equal(ranking.cmc(dist, qid, gid, qcam, gcam, first_match_break=True), eval_oracle.cmc(host, qid, gid, qcam, gcam, first_match_break=True))
    assert np.array_equal(ranking.cmc(dist, qid, gid, qcam, gcam), eval_oracle.cmc(host, qid, gid, qcam, gcam))       # all-shots: ssg_rank_metrics_all
    # the all-shots entry point by name, on the strided device matrix: its first ranks / AP are those of the plain entry point
    tq, tqc, tg, tgc = (torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev) for a in (qid, qcam, gid, gcam))
    cap = int(np.bincount(gid).max())
    f2 = torch.empty(m, dtype=torch.int32, device=dev); ap2 = torch.empty(m, dtype=torch.float64, device=dev); ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    nmb = torch.zeros((m, cap), dtype=torch.int32, device=dev); nm = torch.zeros(m, dtype=torch.int32, device=dev)
    check(L.ssg_rank_metrics_all(ptr(dist), m, n, dist.stride(0), ptr(tq), ptr(tqc), ptr(tg), ptr(tgc), 0, ptr(f2), ptr(ap2), ptr(ovf),
                                 ptr(nmb), ptr(nm), cap, stream()), "ssg_rank_metrics_all")
    assert int(ovf.item()) == 0 and np.array_equal(f2.cpu().numpy(), ofirst)
    assert np.array_equal(np.isnan(ap2.cpu().numpy()), np.isnan(oap)) and np.nanmax(np.abs(ap2.cpu().numpy() - oap)) < 1e-12
    valid = (gid[None, :] != qid[:, None]) | (gcam[None, :] != qcam[:, None])
    assert np.array_equal(nm.cpu().numpy(), ((gid[None, :] == qid[:, None]) & valid).sum(1))
    assert np.array_equal(nmb.cpu().numpy()[ofirst >= 0, 0], ofirst[ofirst >= 0])


def test_clamp_sqrt_bit_for_bit(L, dev):
    """`ssg_clamp_sqrt_f32` (triplet.pairwise_dist: dist = sqrt(clamp(sq, min))) against torch.clamp(min=lo).sqrt() on the CPU, bit for bit, on
    values below, at and above the clamp, denormals, +-0, +inf and NaN (any NaN equals any NaN), strewn over a length that wraps the grid.

    The reference expression is evaluated in float64 and rounded once to float32: the IEEE float32 square root (53 >= 2 * 24 + 2 bits, no
    double rounding).  torch 2.10's own float32 CPU sqrt is 1 ulp off that value on 4314 of the 2 097 255 values used here; numpy's on none."""
    from ssg_amd._lib import check, ptr, stream
    for lo in (1e-12, 0.0, 2.0 ** -140, 0.25):
        lo32 = float(np.float32(lo))
        nxt = float(np.nextafter(np.float32(lo32), np.float32(np.inf))); prv = float(np.nextafter(np.float32(lo32), np.float32(-np.inf)))
        crafted = torch.tensor([lo32, nxt, prv, 0.0, -0.0, -1.0, -1e-30, 1e-45, 2.0 ** -149, 2.0 ** -127, 1.1754942e-38, 1.17549435e-38, 1e-13, 1e-12, 1e-11, 0.1,
                                1.0, 2.0, 3.0, 4.0, 1e30, 3.4028235e38, float("inf"), float("-inf"), NAN, -NAN], dtype=torch.float32)
        g = torch.Generator().manual_seed(3)
        n = 8192 * 256 + 77
        v = torch.cat([crafted, torch.randn(n, generator=g) * 10.0 ** torch.randint(-20, 5, (n,), generator=g).float()])
        v[1000::997] = crafted.repeat(100)[: v[1000::997].numel()]
        ref = v.double().clamp(min=lo32).sqrt().float()
        ref32 = v.clamp(min=lo32).sqrt()
        got = v.to(dev)
        check(L.ssg_clamp_sqrt_f32(ptr(got), got.numel(), lo32, stream()), "ssg_clamp_sqrt_f32")
        got = got.cpu()
        same = (got.view(torch.int32) == ref.view(torch.int32)) | (torch.isnan(got) & torch.isnan(ref))
        same32 = (ref32.view(torch.int32) == ref.view(torch.int32)) | (torch.isnan(ref32) & torch.isnan(ref))
        print("clamp-sqrt: lo %.3e  kernel differs from the IEEE value on %d of %d, torch's float32 sqrt on %d" % (lo32, int((~same).sum()), same.numel(), int((~same32).sum())))
        assert bool(same.all()), (lo, v[~same][:8], got[~same][:8], ref[~same][:8])
        assert bool(same[: crafted.numel()].all()) and bool(torch.isnan(got[crafted.numel() - 2: crafted.numel()]).all())


def test_wrappers_surface_the_2gib_refusal_as_ssgerror(L, dev):
    """an x operand of more than 2^31 - 1 bytes is refused by both GEMM entry points (their buffer resource covers 2 GiB); `_sqdist` and
    `re_ranking_init_device` raise SSGError with the entry point's own message before they allocate or copy anything (the operands here
    are expanded views of one row: 65 537 x 8192 floats = 2 GiB + 32 KiB that are never materialised)"""
    import ssg_amd
    from ssg_amd.evaluators import _sqdist
    from ssg_amd.rerank import re_ranking_init_device
    x = torch.zeros((1, 8192), dtype=torch.float32, device=dev).expand(65537, 8192)
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(ssg_amd.SSGError, match="ssg_pairwise_sqdist_f32.*2 GiB"):
        _sqdist(x, x[:64])
    with pytest.raises(ssg_amd.SSGError, match="ssg_cosine_dist_f32.*2 GiB"):
        re_ranking_init_device(x[:64], x[64:])
    assert free0 - torch.cuda.mem_get_info()[0] < 2 ** 28
