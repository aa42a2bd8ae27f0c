"""The int8 exact Gram (csrc/gram_i8.hip: ssg_gram_i8_encode + ssg_sqdist_self_i8) against the exact reference of tests/gram_i8_ref.py,
bit for bit, at every kernel variant, pipeline tail, tile order, stripe and edge the case table lists.

One child process per configuration (the knobs are cached per process, tests/gram_i8_child.py):
    default     LDS-DMA kernel for 3 digits and >= 4 k blocks (3 and 4 stages), register-staged otherwise; super-blocks of 6 x 6 tiles
    nodma       the register-staged kernel everywhere, panel-major digits        (SSG_I8_DMA=0)
    nodma_kb2   the same with two k blocks per stage where the count is even     (SSG_I8_DMA=0 SSG_I8_KB2=2)
    sb0         the plain upper triangle                                          (SSG_I8_SB=0)
    sb2         super-blocks of 2 x 2 tiles                                       (SSG_I8_SB=2)
The d = 8192 and d = 16384 cases (the kernels with the modulo-2^64 epilogue) run in the first two only, one of them in nodma_kb2 as well.
Every assertion is an equality of bits:
    a  D equals the reference for every case, stripe and stage count, and no 0xFFFF of the pre-fill is left
    b  rowmax equals the reference's row maxima of the stored rows
    c  a stripe equals the rows of the same child's whole matrix; the whole matrix is symmetric with a zero diagonal and zeros at the
       duplicate rows
    d  every configuration and stage count gives the same D
    e  the encoder: exact int64 norms, the reference's digits in the documented layout, zeros in the padding of the last k block, no flag
    f  inputs that do not fit raise the flag; the multiply then returns SSG_OK and leaves D alone; the Python layer raises SSGError
    g  re_ranking_device(no_rerank=True).euclid, with and without memory_save, equals the reference"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gram_i8_ref as ref  # noqa: E402

FLAG_CASES = ("half_3dig", "nan_3dig", "inf_3dig", "over1_4dig")
PUBLIC = ("unit_n385_d160_3dig", "antipodal_n66_d8192_4dig", "antipodal_n66_d16384_4dig")
_POP = ("SSG_I8_DMA", "SSG_I8_SB", "SSG_I8_KB2", "SSG_I8_DMA_STAGES", "SSG_SELF_GRAM", "SSG_SELF_GRAM_DIGITS")
_RESULTS = {}
CONFIG_CASES = [(cfg, name) for cfg in ref.CONFIGS for name in ref.cases_of(cfg)]


def _child(config, tmp):
    """arrays of one configuration; a child that failed is not started again, and no other child after it"""
    if config not in _RESULTS:
        assert not any(isinstance(v, str) for v in _RESULTS.values()), "an earlier child failed: no further child is started"
        env = {k: v for k, v in os.environ.items() if k not in _POP}
        env.update(ref.CONFIGS[config])
        out = os.path.join(str(tmp), config + ".npz")
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gram_i8_child.py"), out, config], capture_output=True, text=True, timeout=240,
                               env=env, cwd=ROOT)
            if r.returncode != 0:
                _RESULTS[config] = "child %s: exit %d\n%s%s" % (config, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
            else:
                with np.load(out) as z:
                    _RESULTS[config] = (json.loads(r.stdout.strip().splitlines()[-1]), {k: z[k] for k in z.files})
        except subprocess.TimeoutExpired:
            _RESULTS[config] = "child %s: timed out" % config
    res = _RESULTS[config]
    assert not isinstance(res, str), res
    return res[1]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("gram_i8")


def _stages(config, name):
    c = ref.CASES[name]
    return (3, 4) if ref.use_dma(c.N, c.d, c.nd, ref.CONFIGS[config]) else (0,)


def _calls(config, name):
    """(key prefix, row0, nrows) of every ssg_sqdist_self_i8 call of a case"""
    c = ref.CASES[name]
    return [("%s/s%d/%d_%d/" % (name, ns, row0, nrows), row0, nrows) for ns in _stages(config, name) for row0, nrows in ((0, c.N),) + c.stripes]


def _first(got, want, row0=0):
    w = np.argwhere(got != want)
    return "%d entries differ; first (row, col): got, reference = %s" % (
        len(w), ", ".join("(%d, %d): %#06x, %#06x" % (i + row0, j, got[i, j], want[i, j]) for i, j in w[:6]))


@pytest.mark.parametrize("config,name", CONFIG_CASES)
def test_D_and_rowmax_equal_the_reference(config, name, tmp):
    """a, b"""
    z = _child(config, tmp)
    t = ref.truth(name)
    for key, row0, nrows in _calls(config, name):
        D, rowmax = z[key + "D"], z[key + "rowmax"]
        want = t["D"][row0:row0 + nrows]
        assert D.shape == want.shape
        assert not (D == ref.SENTINEL).any(), "a: %s: %d entries were never written" % (key, (D == ref.SENTINEL).sum())
        assert np.array_equal(D, want), "a: %s: %s" % (key, _first(D, want, row0))
        assert np.array_equal(rowmax, t["rowmax"][row0:row0 + nrows]), "b: %s: rowmax differs on rows %s" % (
            key, (np.nonzero(rowmax != t["rowmax"][row0:row0 + nrows])[0][:8] + row0).tolist())


@pytest.mark.parametrize("config,name", CONFIG_CASES)
def test_stripes_and_symmetry(config, name, tmp):
    """c: stated on the kernel's own outputs"""
    z = _child(config, tmp)
    c = ref.CASES[name]
    for ns in _stages(config, name):
        W = z["%s/s%d/0_%d/D" % (name, ns, c.N)]
        assert np.array_equal(W, W.T), "c: not symmetric: " + _first(W, W.T)
        assert not np.diag(W).any(), "c: diagonal"
        for i, j in ref.duplicates(name):
            assert W[i, j] == 0 and W[j, i] == 0, "c: duplicate rows"
        for row0, nrows in c.stripes:
            S = z["%s/s%d/%d_%d/D" % (name, ns, row0, nrows)]
            assert np.array_equal(S, W[row0:row0 + nrows]), "c: stripe (%d, %d): %s" % (row0, nrows, _first(S, W[row0:row0 + nrows], row0))
            assert np.array_equal(z["%s/s%d/%d_%d/rowmax" % (name, ns, row0, nrows)], W[row0:row0 + nrows].max(axis=1))


@pytest.mark.parametrize("name", list(ref.CASES))
def test_every_configuration_gives_the_same_bits(name, tmp):
    """d"""
    c = ref.CASES[name]
    first = None
    for config in ref.CONFIGS:
        if name not in ref.cases_of(config):
            continue
        z = _child(config, tmp)
        for key, row0, nrows in _calls(config, name):
            k = (row0, nrows)
            first = first if first is not None else {}
            if k not in first:
                first[k] = (config, key, z[key + "D"], z[key + "rowmax"])
            else:
                assert np.array_equal(z[key + "D"], first[k][2]) and np.array_equal(z[key + "rowmax"], first[k][3]), \
                    "d: %s under %s differs from %s under %s" % (key, config, first[k][1], first[k][0])
    assert first is not None and (0, c.N) in first


@pytest.mark.parametrize("config,name", CONFIG_CASES)
def test_encoder_outputs(config, name, tmp):
    """e"""
    z = _child(config, tmp)
    c = ref.CASES[name]
    t = ref.truth(name)
    assert int(z[name + "/flag"][0]) == 0
    assert np.array_equal(z[name + "/norms"], t["norms"])
    dg = ref.decode_E(z[name + "/E"], c.N, c.d, c.nd, planar=ref.use_dma(c.N, c.d, c.nd, ref.CONFIGS[config]))
    assert np.array_equal(dg[:, :c.d], t["digits"]), "e: digits"
    assert not dg[:, c.d:].any(), "e: the padding of the last k block is not zero"


@pytest.mark.parametrize("config", list(ref.CONFIGS))
@pytest.mark.parametrize("fname", FLAG_CASES)
def test_flagged_input_is_left_to_the_caller(fname, config, tmp):
    """f"""
    z = _child(config, tmp)
    assert int(z["flag/%s/flag" % fname][0]) == 1
    assert int(z["flag/%s/rc" % fname]) == 0
    assert (z["flag/%s/D" % fname] == ref.SENTINEL).all()


@pytest.mark.parametrize("config", list(ref.CONFIGS))
def test_python_layer_raises_when_the_digits_do_not_fit(config, tmp):
    """f"""
    assert int(_child(config, tmp)["pylayer/raised"]) == 1


@pytest.mark.parametrize("ms", [0, 1])
@pytest.mark.parametrize("name", PUBLIC)
@pytest.mark.parametrize("config", ref.BIG_CONFIGS)
def test_public_surface(config, name, ms, tmp):
    """g.  antipodal rows at d = 8192 and d = 16384: distances of 32768 (0x7800) and inf (0x7C00) between rows 0 and 1 -- the sums
    nA + nB - 2 dot = 2^63 and 2^64 that wrapped in int64 before the epilogue combined them modulo 2^64"""
    z = _child(config, tmp)
    want, _, _, exact = ref.dist_bits(ref.inputs(name), bool(ms))
    assert exact
    got = z["public/%s/ms%d" % (name, ms)]
    assert np.array_equal(got, want), "g: " + _first(got, want)
