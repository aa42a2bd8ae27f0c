"""What the JPEG damage / edge suites (tests/test_jpeg_damage_host.py, tests/test_gpu_jpeg_edges.py) and
test_jpeg_kernel_text_executed_on_host_matches_pillow share: the files, and the kernels of csrc/jpeg.hip built as a host program.

    edge_files()                         well-formed files at the edges of the format: every size 1..5 x 1..5 at 4:4:4 / 4:2:2 / 4:2:0,
                                         grayscale with sides 1..33, three kinds of noise at quality 1, 2, 5, 10, 95, 100 (with / without
                                         optimised tables and one restart marker per block), quantisation tables of all 255 / all 1,
                                         COM and ICC payloads that spell SOI / SOF2 / SOS / EOI, streamtype=0
    damaged_files(seed, n, qlo, qhi)     n draws of a Pillow-written file (sides 8..79, any layout, optimize and restart interval drawn)
                                         with exactly ONE bit of its entropy-coded data flipped; no 0xFF byte, and no byte behind one,
                                         is created or touched, so the marker structure of the file is intact
    reference(data)                      np.asarray(Image.open(...).convert('RGB')): Pillow at run time is the reference
    host_decoder() / run_host(...)       tools/fuzz/jpeg_device_fuzz.cpp -DFZ_MAIN over the kernel text cut from csrc/jpeg.hip (with ASan)

Everything is deterministic from its seeds.  A plain module, imported by name: no fixture lives here."""
import functools
import io
import os
import subprocess
import tempfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
LAYOUTS = ("444", "422", "420", "gray")
MARKER_SOUP = b"\xff\xd8\xff\xc2\x00\x0b\x08\x00\x10\x00\x10\x01\x01\x11\x00\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00\xff\xd9" * 3


def encode(a, layout, **kw):
    """uint8 [h, w, 3] -> JPEG bytes; layout 444 / 422 / 420 (chroma subsampling 0 / 1 / 2) or gray (the first channel alone)"""
    buf = io.BytesIO()
    if layout == "gray":
        Image.fromarray(np.ascontiguousarray(a[..., 0])).save(buf, "JPEG", **kw)
    else:
        Image.fromarray(a).save(buf, "JPEG", subsampling=LAYOUTS.index(layout), **kw)
    return buf.getvalue()


_refs = {}


def reference(data):
    """Pillow's pixels of a file (computed once per file, read-only); raises what Pillow raises"""
    if data not in _refs:
        a = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        a.setflags(write=False)
        _refs[data] = a
    return _refs[data]


def gradient_noise(rng, h, w, sigma):
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([xx * 255.0 / max(w - 1, 1), yy * 255.0 / max(h - 1, 1), (xx + yy) * 127.0 / max(h + w - 2, 1)], -1) + rng.normal(0, sigma, (h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def _noise(rng, kind, h, w):
    if kind == "uniform":
        return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "bw":                                          # black / white, the three channels alike
        return np.repeat(rng.integers(0, 2, (h, w, 1)) * 255, 3, axis=2).astype(np.uint8)
    return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)       # "bw3": black / white per channel


@functools.lru_cache(maxsize=None)
def edge_files():
    """-> tuple of (tag, bytes): the well-formed edge battery"""
    rng = np.random.default_rng(2024)
    out = []
    for lay in LAYOUTS[:3]:
        for h in range(1, 6):
            for w in range(1, 6):
                out.append(("tiny_%s_%dx%d" % (lay, h, w), encode(_noise(rng, "uniform", h, w), lay, quality=90)))
    for s in range(1, 34):
        out.append(("gray_%dx%d" % (s, 34 - s), encode(gradient_noise(rng, s, 34 - s, 20), "gray", quality=75)))
    for kind in ("uniform", "bw", "bw3"):
        for q in (1, 2, 5, 10, 95, 100):
            for lay in LAYOUTS[:3]:
                for opt in (False, True):
                    for rst in (0, 1):
                        h, w = int(rng.integers(9, 41)), int(rng.integers(9, 41))
                        kw = dict(quality=q, optimize=opt)
                        if rst:
                            kw["restart_marker_blocks"] = 1
                        out.append(("%s_q%d_%s_opt%d_rst%d_%dx%d" % (kind, q, lay, opt, rst, h, w), encode(_noise(rng, kind, h, w), lay, **kw)))
    for lay in LAYOUTS:
        for v in (255, 1):
            out.append(("qt%d_%s" % (v, lay), encode(_noise(rng, "bw3", 24, 19), lay, qtables=[[v] * 64, [v] * 64])))
    for lay in LAYOUTS:
        a = gradient_noise(rng, 21, 30, 15)
        out.append(("com_%s" % lay, encode(a, lay, quality=80, comment=MARKER_SOUP)))
        out.append(("icc_%s" % lay, encode(a, lay, quality=80, icc_profile=MARKER_SOUP * 40)))
        out.append(("streamtype0_%s" % lay, encode(a, lay, quality=80, streamtype=0)))
    assert len(set(t for t, _ in out)) == len(out)
    return tuple(out)


def ecs_range(data):
    """(first byte, end) of the entropy-coded data of a Pillow-written baseline file: behind the SOS header, up to the EOI marker"""
    p = 2
    while True:
        assert data[p] == 0xFF, p
        m = data[p + 1]
        n = (data[p + 2] << 8) | data[p + 3]
        p += 2 + n
        if m == 0xDA:
            break
    end = len(data) - 2
    assert data[end:] == b"\xff\xd9"
    return p, end


def flip_one_bit(rng, data):
    """one bit of the entropy-coded data flipped; the byte is not 0xFF, does not follow a 0xFF and does not become 0xFF"""
    s, e = ecs_range(data)
    while True:
        q, bit = int(rng.integers(s, e)), int(rng.integers(0, 8))
        nb = data[q] ^ (1 << bit)
        if data[q] != 0xFF and data[q - 1] != 0xFF and nb != 0xFF:
            return data[:q] + bytes([nb]) + data[q + 1:], q, bit


@functools.lru_cache(maxsize=None)
def damaged_files(seed, n, quality_lo, quality_hi):
    """-> tuple of (tag, bytes): n draws, minus the files on which Pillow raises (asserted to be fewer than 5 % of the draws)"""
    rng = np.random.default_rng(seed)
    out, dropped = [], 0
    for k in range(n):
        h, w = int(rng.integers(8, 80)), int(rng.integers(8, 80))
        lay = LAYOUTS[int(rng.integers(0, 4))]
        q = int(rng.integers(quality_lo, quality_hi + 1))
        kw = dict(quality=q, optimize=bool(rng.integers(0, 2)))
        if rng.integers(0, 2):
            kw["restart_marker_blocks"] = int(rng.integers(1, 6))
        sigma = float(rng.choice([4.0, 12.0, 40.0]))
        clean = encode(gradient_noise(rng, h, w, sigma), lay, **kw)
        data, pos, bit = flip_one_bit(rng, clean)
        assert len(data) == len(clean) and sum(bin(x ^ y).count("1") for x, y in zip(data, clean)) == 1
        assert data.count(b"\xff") == clean.count(b"\xff")
        try:
            reference(data)
        except Exception:       # noqa: BLE001  (whatever Pillow raises, the reference raises: such a file has no pixels to compare)
            dropped += 1
            continue
        out.append(("s%d_%03d_%s_q%d_%dx%d_rst%d_opt%d_byte%d_bit%d" % (seed, k, lay, q, h, w, kw.get("restart_marker_blocks", 0), kw["optimize"], pos, bit), data))
    assert dropped * 20 < n, "Pillow raised on %d of %d damaged files" % (dropped, n)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def clean_files(seed, n):
    """-> tuple of (tag, bytes): undamaged neighbours for the batches of the GPU test (sides 8..79, any layout)"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        h, w = int(rng.integers(8, 80)), int(rng.integers(8, 80))
        lay = LAYOUTS[int(rng.integers(0, 4))]
        kw = dict(quality=int(rng.integers(25, 99)), optimize=bool(rng.integers(0, 2)))
        if rng.integers(0, 2):
            kw["restart_marker_blocks"] = int(rng.integers(1, 6))
        out.append(("clean%d_%03d_%s_%dx%d" % (seed, k, lay, h, w), encode(gradient_noise(rng, h, w, 20.0), lay, **kw)))
    return tuple(out)


# ------------------------------------------------------------------ the kernels of csrc/jpeg.hip as a host program
def cut_kernel_text():
    """the device code of csrc/jpeg.hip (namespace ssg { ... } up to the C entry point), as the fuzz harness includes it"""
    src = os.path.join(ROOT, "self-similarity-grouping_amd", "csrc", "jpeg.hip")
    text, on = [], False
    for line in open(src):
        if line.startswith("namespace ssg {"):
            on = True
        if line.startswith("using namespace ssg;"):
            break
        if on:
            text.append(line)
    assert any("colour_kernel" in ln for ln in text) and any("huffman_kernel" in ln for ln in text)
    return "".join(text)


_host = {}


def host_decoder():
    """path of the stand-alone decoder `jpeg_device_host` (built once per process, with AddressSanitizer), or None when the ROCm
    clang++ is not installed.  exit codes: 0 decoded, 3 the parser hands the file to Pillow, 4 the kernels flagged the file."""
    if "exe" not in _host:
        if not os.path.exists(CLANG):
            _host["exe"] = None
            return None
        _host["dir"] = tempfile.TemporaryDirectory(prefix="ssg_jpeg_host_")
        d = _host["dir"].name
        with open(os.path.join(d, "jpeg_kernels_cut.inc"), "w") as f:
            f.write(cut_kernel_text())
        exe = os.path.join(d, "jpeg_device_host")
        r = subprocess.run([CLANG, "-x", "hip", "--offload-host-only", "-O1", "-DFZ_MAIN", "-fsanitize=address", "-Wno-option-ignored", "-I/opt/rocm/include",
                            "-I" + d, "-o", exe, os.path.join(ROOT, "tools", "fuzz", "jpeg_device_fuzz.cpp"), "-lpthread"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        _host["exe"] = exe
    return _host["exe"]


def run_host(data):
    """one file through the host decoder -> (exit code, uint8 pixels flat or None); any exit code but 0 / 3 / 4 is a sanitizer report"""
    return run_host_many([data])[0]


def run_host_many(files):
    """files (bytes each) through ONE run of the host decoder (`--dir`: one process, a fresh parse + decode per file)
    -> list of (code, uint8 pixels flat or None).  A sanitizer report ends the process: that fails here."""
    exe = host_decoder()
    with tempfile.TemporaryDirectory(prefix="ssg_jpeg_run_") as d:
        for i, data in enumerate(files):
            with open(os.path.join(d, "%d.jpg" % i), "wb") as f:
                f.write(data)
        r = subprocess.run([exe, "--dir", d, str(len(files))], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        codes = [int(x) for x in r.stdout.split()]
        assert len(codes) == len(files) and all(c in (0, 3, 4) for c in codes), codes
        return [(c, np.fromfile(os.path.join(d, "%d.rgb" % i), np.uint8) if c == 0 else None) for i, c in enumerate(codes)]
