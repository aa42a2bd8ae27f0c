"""GPU suite of the JPEG decoder (csrc/jpeg.hip through ssg_amd.jpeg.decode_batch) on the files of tests/jpeg_cases_ref.py.
The reference is Pillow at run time; every image is at most 80 pixels a side.

    edge battery     well-formed files at the edges of the format, in three mixed batches: Pillow's bytes, all decoded on the device,
                     none handed to Pillow
    damaged corpora  one flipped bit in the entropy-coded data (the two corpora of tests/test_jpeg_damage_host.py), in batches of 64 with
                     undamaged files among them: every output equals Pillow's, the device flags exactly the files oracle/jpeg_oracle.py
                     calls Damaged (the same rule, stated in numpy), and at least half of each corpus is decoded on the device
    launch shapes    more than 64 restart segments (a second workgroup of the Huffman grid); a 1 x 1 next to an 80 x 80 image (most
                     threads of the block and pixel grids leave early); packed=True clean and with one flagged file
    byte stuffing    a batch assembled so that stuffed FF 00 pairs start at all eight residues mod 8 of the pool (7: the pair straddles
                     two 8-byte chunks of BitReader) and segments start at every residue 1..7
"""
import numpy as np
import pytest

import jpeg_cases_ref as jc
from oracle import jpeg_oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CORPORA = ((1, 400, 25, 98), (7, 400, 1, 29))


@pytest.fixture(scope="module")
def pj():
    from ssg_amd import jpeg
    return jpeg


def _decode(pj, files, **kw):
    """decode_batch + the movement of the counters -> (outputs, rise of gpu, pillow, damaged)"""
    before = dict(pj.stats)
    out = pj.decode_batch(files, **kw)
    return out, tuple(pj.stats.get(k, 0) - before.get(k, 0) for k in ("gpu", "pillow", "damaged"))


def _oracle_damaged(data):
    try:
        jpeg_oracle.decode(data)
    except jpeg_oracle.Damaged:
        return True
    return False


def test_edge_battery_in_mixed_batches(pj):
    files = jc.edge_files()
    for part in range(3):                       # every third file: each batch mixes sizes, layouts, qualities and restart intervals
        batch = files[part::3]
        out, (gpu, pillow, damaged) = _decode(pj, [d for _, d in batch])
        for (tag, data), o in zip(batch, out):
            assert o.dtype == torch.uint8 and o.is_cuda
            assert np.array_equal(o.cpu().numpy(), jc.reference(data)), tag
        assert (gpu, pillow, damaged) == (len(batch), 0, 0)


@pytest.mark.parametrize("corpus", CORPORA, ids=lambda c: "seed%d_q%d-%d" % (c[0], c[2], c[3]))
def test_damaged_corpus_in_batches_of_64(pj, corpus):
    files = jc.damaged_files(*corpus)
    clean = jc.clean_files(100 + corpus[0], 16)
    on_gpu = 0
    for start in range(0, len(files), 48):      # 48 damaged files + 16 undamaged ones, every fourth position
        part = list(files[start:start + 48])
        batch, is_clean = [], []
        for k, f in enumerate(part):
            batch.append(f); is_clean.append(False)
            if k % 3 == 2:
                batch.append(clean[k // 3]); is_clean.append(True)
        assert len(batch) == 64 or start + 48 >= len(files)
        expect = sum(_oracle_damaged(d) for (_, d), c in zip(batch, is_clean) if not c)
        out, (gpu, pillow, damaged) = _decode(pj, [d for _, d in batch])
        for (tag, data), o in zip(batch, out):
            assert np.array_equal(o.cpu().numpy(), jc.reference(data)), tag
        assert damaged == pillow == expect and gpu == len(batch) - expect, (start, gpu, pillow, damaged, expect)
        on_gpu += gpu - sum(is_clean)
    print("corpus %r: %d files, %d decoded on the device, %d flagged" % (corpus, len(files), on_gpu, len(files) - on_gpu))
    assert 2 * on_gpu >= len(files)


def test_more_than_64_restart_segments(pj):
    """80 x 80 at 4:4:4 with a restart marker behind every block: 100 segments per file, 301 in the batch = 5 workgroups of the Huffman
    grid, the last one with 45 of 64 threads at work"""
    rng = np.random.default_rng(31)
    files = [jc.encode(jc.gradient_noise(rng, 80, 80, 25.0), lay, quality=88, restart_marker_blocks=1) for lay in ("444", "444", "gray")]
    files.append(jc.encode(jc.gradient_noise(rng, 1, 1, 0.0), "420", quality=50))
    P = pj.parse_batch_python(files)
    assert P.segs.shape[0] == 301
    out, (gpu, pillow, damaged) = _decode(pj, files)
    assert (gpu, pillow, damaged) == (4, 0, 0)
    for k, (data, o) in enumerate(zip(files, out)):
        assert np.array_equal(o.cpu().numpy(), jc.reference(data)), k


@pytest.mark.parametrize("order", ((0, 1), (1, 0)), ids=("small_first", "large_first"))
def test_one_pixel_next_to_80x80(pj, order):
    rng = np.random.default_rng(32)
    pair = [jc.encode(jc.gradient_noise(rng, 1, 1, 0.0), "444", quality=90), jc.encode(jc.gradient_noise(rng, 80, 80, 30.0), "420", quality=70)]
    files = [pair[k] for k in order]
    P = pj.parse_batch_python(files)
    assert (P.max_blocks, P.max_pixels) == (100, 6400) and sorted(P.dims) == [(1, 1), (80, 80)]
    out, (gpu, pillow, damaged) = _decode(pj, files)
    assert (gpu, pillow, damaged) == (2, 0, 0)
    for data, o in zip(files, out):
        assert np.array_equal(o.cpu().numpy(), jc.reference(data))


def test_packed_clean_and_with_one_flagged_file(pj):
    rng = np.random.default_rng(33)
    files = [jc.encode(jc.gradient_noise(rng, 37, 22, 20.0), ("444", "422", "420", "420", "444")[k], quality=60 + 5 * k) for k in range(5)]
    out, (gpu, pillow, damaged) = _decode(pj, files, packed=True)
    assert torch.is_tensor(out) and tuple(out.shape) == (5, 37, 22, 3) and out.dtype == torch.uint8 and out.is_cuda
    assert (gpu, pillow, damaged) == (5, 0, 0)
    for k in range(5):
        assert np.array_equal(out[k].cpu().numpy(), jc.reference(files[k])), k
    # one file of the same size that the device flags: the first single-bit flip the oracle calls Damaged and Pillow still decodes
    bad = None
    for _ in range(200):
        cand = jc.flip_one_bit(rng, files[2])[0]
        if _oracle_damaged(cand):
            try:
                jc.reference(cand)
            except Exception:       # noqa: BLE001  (Pillow raises: no pixels to compare, draw again)
                continue
            bad = cand
            break
    assert bad is not None
    mixed = files[:2] + [bad] + files[3:]
    out, (gpu, pillow, damaged) = _decode(pj, mixed, packed=True)
    assert isinstance(out, list) and len(out) == 5
    assert (gpu, pillow, damaged) == (4, 1, 1)
    for k in range(5):
        assert tuple(out[k].shape) == (37, 22, 3) and np.array_equal(out[k].cpu().numpy(), jc.reference(mixed[k])), k


def test_stuffed_bytes_and_segment_starts_at_every_residue(pj):
    """The pool offsets come from parse_batch_python (the native parser, which the product uses, is held to the same pool): files are
    added until stuffed FF 00 pairs start at all eight residues mod 8 and restart segments at all eight too."""
    rng = np.random.default_rng(34)
    files = []

    def residues(P):
        pool = P.pool[:-64]
        ff = np.nonzero((pool[:-1] == 0xFF) & (pool[1:] == 0x00))[0]
        return set((ff % 8).tolist()), set((P.segs[:, 1] % 8).tolist()), len(ff)

    for k in range(12):
        h, w = int(rng.integers(17, 41)), int(rng.integers(17, 41))
        files.append(jc.encode(rng.integers(0, 256, (h, w, 3)).astype(np.uint8), jc.LAYOUTS[k % 4], quality=97, restart_marker_blocks=1 + k % 2))
        P = pj.parse_batch_python(files)
        stuffed, starts, n = residues(P)
        if k >= 2 and stuffed == set(range(8)) and starts == set(range(8)):
            break
    assert stuffed == set(range(8)) and starts == set(range(8)) and n >= 8, (stuffed, starts, n)
    pool = P.pool[:-64]
    lo, hi = P.segs[:, 1], P.segs[:, 1] + P.segs[:, 2]
    ff7 = [q for q in np.nonzero((pool[:-1] == 0xFF) & (pool[1:] == 0x00))[0] if q % 8 == 7]
    assert any(((lo <= q) & (q + 1 < hi)).any() for q in ff7)              # a straddling pair lies INSIDE a segment the kernel reads
    N = pj._parse_batch_native(files)
    assert np.array_equal(N.pool, P.pool) and np.array_equal(N.segs, P.segs)
    out, (gpu, pillow, damaged) = _decode(pj, files)
    assert (gpu, pillow, damaged) == (len(files), 0, 0)
    for k, (data, o) in enumerate(zip(files, out)):
        assert np.array_equal(o.cpu().numpy(), jc.reference(data)), k
