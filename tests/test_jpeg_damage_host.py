"""csrc/jpeg.hip's contract -- every file comes back with the bytes of Image.open(f).convert('RGB'), or is flagged and handed to
Pillow -- on files whose scan is complete but wrong, and on well-formed files at the edges of the format.  No GPU: the kernels'
source text runs as a host program (tools/fuzz/jpeg_device_fuzz.cpp, tests/jpeg_cases_ref.py), next to oracle/jpeg_oracle.py.

Counts of the two damaged corpora (Pillow 12.2.0, libjpeg-turbo with SIMD; profiles/jpeg_damage.txt):
                                      equal  flagged  different
    seed 1, quality 25-98   before     322      62       16        (decode_symbol took 16 bits for an unknown code; the IDCT wrapped
    seed 7, quality  1-29   before     240     143       17         where libjpeg-turbo's SIMD code saturates / works in 16 bits)
    seed 1, quality 25-98   now        328      72        0
    seed 7, quality  1-29   now        250     150        0"""
import numpy as np
import pytest

import jpeg_cases_ref as jc
from oracle import jpeg_oracle

CORPORA = ((1, 400, 25, 98), (7, 400, 1, 29))


@pytest.fixture(scope="module")
def host():
    if jc.host_decoder() is None:
        pytest.skip("ROCm clang++ not present")
    return jc.run_host_many


def test_edge_files_decode_unflagged_and_equal_pillow(host):
    """every well-formed edge file: exit 0 (never flagged, never left to the parser's fallback) and Pillow's bytes"""
    files = jc.edge_files()
    assert len(files) > 300
    for (tag, data), (rc, px) in zip(files, host([d for _, d in files])):
        ref = jc.reference(data)
        assert rc == 0, (tag, rc)
        assert px.size == ref.size and np.array_equal(px.reshape(ref.shape), ref), tag


def test_edge_files_oracle_equals_pillow():
    for tag, data in jc.edge_files():
        assert np.array_equal(jpeg_oracle.decode(data), jc.reference(data)), tag


@pytest.mark.parametrize("corpus", CORPORA, ids=lambda c: "seed%d_q%d-%d" % (c[0], c[2], c[3]))
def test_damaged_files_flagged_or_equal_pillow(host, corpus):
    """one flipped bit in the entropy-coded data: the file is flagged (exit 4) or its bytes are Pillow's -- no exception; and the flag is
    no escape hatch: at least half of the corpus is still decoded"""
    files = jc.damaged_files(*corpus)
    assert len(files) > 0.95 * corpus[1]
    equal, flagged, different = 0, 0, []
    for (tag, data), (rc, px) in zip(files, host([d for _, d in files])):
        assert rc in (0, 4), (tag, rc)                  # (3 would be the parser refusing a file whose headers are intact)
        if rc == 4:
            flagged += 1
            continue
        ref = jc.reference(data)
        if px.size == ref.size and np.array_equal(px.reshape(ref.shape), ref):
            equal += 1
        else:
            different.append(tag)
    print("corpus %r: %d files, %d equal, %d flagged, %d different" % (corpus, len(files), equal, flagged, len(different)))
    assert not different, (len(different), different[:10])
    assert 2 * equal >= len(files), (equal, flagged)


@pytest.mark.parametrize("corpus", CORPORA, ids=lambda c: "seed%d_q%d-%d" % (c[0], c[2], c[3]))
def test_damaged_files_oracle_raises_or_equals_pillow(host, corpus):
    """the oracle follows the kernels' rule: Damaged exactly on the files the kernels flag, Pillow's bytes on every other"""
    files = jc.damaged_files(*corpus)
    for (tag, data), (rc, _) in zip(files, host([d for _, d in files])):
        try:
            px = jpeg_oracle.decode(data)
        except jpeg_oracle.Damaged:
            assert rc == 4, tag
            continue
        assert rc == 0, tag
        assert np.array_equal(px, jc.reference(data)), tag


def test_generator_flips_exactly_one_bit_outside_markers():
    """the property the corpora claim: against the same draw's clean file, one bit differs, inside the entropy-coded data, and every 0xFF
    byte and the byte behind it are untouched"""
    rng = np.random.default_rng(3)
    for lay in jc.LAYOUTS:
        clean = jc.encode(jc.gradient_noise(rng, 33, 41, 30.0), lay, quality=92, restart_marker_blocks=2)
        s, e = jc.ecs_range(clean)
        assert clean[s - 14:s - 12] == b"\xff\xda" or clean[s - 10:s - 8] == b"\xff\xda"
        for _ in range(50):
            bad, q, bit = jc.flip_one_bit(rng, clean)
            diff = [i for i in range(len(clean)) if clean[i] != bad[i]]
            assert diff == [q] and s <= q < e and clean[q] ^ bad[q] == 1 << bit
            assert clean[q] != 0xFF and bad[q] != 0xFF and clean[q - 1] != 0xFF
