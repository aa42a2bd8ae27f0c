"""The record behind profiles/jpeg_damage.txt: the kernels of csrc/jpeg.hip as a host program (tests/jpeg_cases_ref.py) over the edge
battery and the damaged corpora of tests/test_jpeg_damage_host.py -- equal to Pillow / flagged / different per corpus -- and, from
oracle/jpeg_oracle.py, the largest IDCT magnitudes of the well-formed edge battery beside the limits of the flag rule.  No GPU.

    python tools/jpeg_damage_counts.py [seed,n,quality_lo,quality_hi ...]      (more corpora than the two of the suite)"""
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import jpeg_cases_ref as jc  # noqa: E402
from oracle import jpeg_oracle  # noqa: E402


def tally(files):
    c = collections.Counter()
    for (tag, data), (rc, px) in zip(files, jc.run_host_many([d for _, d in files])):
        if rc:
            c["flagged" if rc == 4 else "parser"] += 1
            continue
        ref = jc.reference(data)
        c["equal" if px.size == ref.size and np.array_equal(px.reshape(ref.shape), ref) else "different"] += 1
    return c


def main():
    import PIL
    from PIL import features
    print("Pillow %s, libjpeg-turbo %s (jpeg library version %s)" % (PIL.__version__, features.version("libjpeg_turbo"), features.version("jpg")))
    corpora = [(1, 400, 25, 98), (7, 400, 1, 29)] + [tuple(int(x) for x in a.split(",")) for a in sys.argv[1:]]
    print("%-34s %6s %6s %8s %10s" % ("corpus", "files", "equal", "flagged", "different"))
    edge = jc.edge_files()
    c = tally(edge)
    print("%-34s %6d %6d %8d %10d" % ("edge battery (well-formed)", len(edge), c["equal"], c["flagged"] + c["parser"], c["different"]))
    for args in corpora:
        files = jc.damaged_files(*args)
        c = tally(files)
        print("%-34s %6d %6d %8d %10d" % ("seed %d, %d draws, quality %d-%d" % args, len(files), c["equal"], c["flagged"] + c["parser"], c["different"]))
    m = {}
    for _, data in edge:
        jpeg_oracle.decode(data, m)
    print("edge battery, largest magnitudes:  dequantised coefficient %d (flag outside int16), pass-1 IDCT output %d (flag outside int16), "
          "pass-2 IDCT output %d .. %d (flag outside -512 .. 511)" % (m["dequantised"], m["pass1"], m["pass2_min"], m["pass2_max"]))


if __name__ == "__main__":
    main()
