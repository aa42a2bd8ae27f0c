"""The source term's bound tables and refine pass (csrc/source_term.hip, csrc/source_bound.hip, the epi == 3 epilogues of csrc/conv.hip)
against the float64 restatement of tests/source_bound_ref.py.

The contract (rerank.source_bound_params): every entry of the table the bound pass writes -- one per target row and granule of 4 or 8
sources -- is within tol / 2 of the true minimum of its granule.  Checked for every row and every granule, on every bound path:

    default   source_bound_dma_kernel, 4- or 8-source granules by the workspace rule, encode_sqnorm_kernel
    gran8     the same kernel with 8-source granules everywhere          (SSG_SB_GRAN=8)
    nodma     the register-staged source_bound_kernel                    (SSG_SB_DMA=0)
    unfused   separate norm and conversion launches                      (SSG_SB_FUSED_ENC=0)
    split     three products on split-half operands: conv_dma_kernel<128, 256> when Ns_pad % 256 == 0, conv_igemm_kernel 128 x 128 otherwise
    f32       float32 MFMA, conv_igemm_kernel

The first four are one child process each (the knobs are cached per process, tests/source_bound_child.py); split and f32 are selected by
arguments and run in the default child.  Assertions, by the letters the messages carry:
    a  no NaN (the workspace is pre-filled with NaN) in the nrows x ld table
    b  |table - float64 granule minimum| <= tol / 2 for every granule that holds a real source
    c  fully padded granules and the padded norms are >= 1e38
    d  rowmin equals the float64 restatement bit for bit (and source_vector's full float64 Gram)
    e  rowmin is bit-equal across all paths
    f  {g : t[g] <= min t + tol} contains the true granule and lies inside {g : truth[g] <= m* + 2 tol}; exactly one granule per row
       on the perm cases"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import source_bound_ref as ref  # noqa: E402
from source_bound_child import ROW_BLOCK  # noqa: E402

CONFIGS = {"default": {}, "gran8": {"SSG_SB_GRAN": "8"}, "nodma": {"SSG_SB_DMA": "0"}, "unfused": {"SSG_SB_FUSED_ENC": "0"}}
# path -> (child configuration, bound)
PATHS = {"default": ("default", "half"), "gran8": ("gran8", "half"), "nodma": ("nodma", "half"), "unfused": ("unfused", "half"),
         "split": ("default", "split"), "f32": ("default", "f32")}
_POP = ("SSG_SB_DMA", "SSG_SB_GRAN", "SSG_SB_FUSED_ENC", "SSG_SOURCE_BOUND", "SSG_SOURCE_EXACT_GEMM")
_RESULTS = {}


def _child(config, tmp):
    """metrics and arrays of one configuration; a child that failed is not started again, and no other child after it"""
    if config not in _RESULTS:
        assert not any(isinstance(v, str) for v in _RESULTS.values()), "an earlier child failed: no further child is started"
        env = {k: v for k, v in os.environ.items() if k not in _POP and not k.startswith(("SSG_CONV_", "SSG_SPLIT_"))}
        env.update(CONFIGS[config])
        out = os.path.join(str(tmp), config + ".npz")
        cmd = [sys.executable, os.path.join(ROOT, "tests", "source_bound_child.py"), out, "half,split,f32" if config == "default" else "half"]
        try:
            r = subprocess.run(cmd + (["extras"] if config == "default" else []), capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
            if r.returncode != 0:
                _RESULTS[config] = "child %s: exit %d\n%s%s" % (config, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
            else:
                with np.load(out) as z:
                    _RESULTS[config] = (json.loads(r.stdout.strip().splitlines()[-1]), {k: z[k] for k in z.files})
        except subprocess.TimeoutExpired:
            _RESULTS[config] = "child %s: timed out" % config
    res = _RESULTS[config]
    assert not isinstance(res, str), res
    return res


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("source_bound")


def _tol_G(name, path, metrics):
    bound = PATHS[path][1]
    tol = ref.params(name, bound)[0]
    G = metrics[name + "/" + bound]["G"]
    c = ref.case(name)
    assert G == (ref.granule_of(c.tgt.shape[0], c.Ns_pad, c.tgt.shape[1], CONFIGS[PATHS[path][0]]) if bound == "half" else 8)
    return bound, tol, G


def table_errors(name, path, metrics, arrays):
    """-> (failed assertions, max |table - truth| / (tol / 2), refined share)"""
    bound, tol, G = _tol_G(name, path, metrics)
    c = ref.case(name); t = ref.truth(name)
    gm, padded = t[G]
    key = "%s/%s/" % (name, bound)
    table = arrays[key + "table"].astype(np.float64)
    nrows = c.tgt.shape[0]; Ns = c.src.shape[0]
    bad = []
    assert table.shape == gm.shape == (nrows, c.Ns_pad // G)
    if np.isnan(table).any():
        bad.append("a: %d NaN left in the table (first at %s)" % (np.isnan(table).sum(), np.argwhere(np.isnan(table))[0]))
    with np.errstate(invalid="ignore"):
        err = np.abs(table[:, ~padded] - gm[:, ~padded])
    err = np.where(np.isnan(err), np.inf, err)
    worst = float(err.max() / (tol / 2))
    print("%s %s G=%d tol=%.4g max|table - truth| / (tol / 2) = %.4g refined share %.4g" % (name, path, G, tol, worst, metrics[name + "/" + bound]["share"]))
    if not worst <= 1.0:
        r, g = np.unravel_index(err.argmax(), err.shape)
        bad.append("b: |table - granule_min| = %.6g > tol / 2 = %.6g at row %d, granule %d (%d rows / %d entries beyond)"
                   % (err[r, g], tol / 2, r, g, (err > tol / 2).any(axis=1).sum(), (err > tol / 2).sum()))
    colterm = arrays[key + "colterm"]
    if not (np.all(table[:, padded] >= 1e38) and np.all(colterm[Ns:] >= 1e38)):
        bad.append("c: a fully padded granule or a padded norm below 1e38 (min %.6g, %.6g)"
                   % (np.nanmin(table[:, padded], initial=np.inf), np.nanmin(colterm[Ns:], initial=np.inf)))
    S = ref.refine_set(np.nan_to_num(arrays[key + "table"], nan=np.inf), tol, padded)
    rows = np.arange(nrows)
    best = gm.argmin(axis=1)
    if not S[rows, best].all():
        bad.append("f: the true granule is not re-evaluated on %d rows (first %d)" % ((~S[rows, best]).sum(), np.nonzero(~S[rows, best])[0][0]))
    if (S & ~(gm <= gm.min(axis=1, keepdims=True) + 2 * tol)).any():
        bad.append("f: a granule more than 2 tol above the row minimum is re-evaluated")
    if c.kind == "perm" and not np.all(S.sum(axis=1) == 1):
        bad.append("f: %d rows of a perm case re-evaluate more than one granule" % (S.sum(axis=1) != 1).sum())
    return bad, worst, float(S.sum()) / (nrows * int((~padded).sum()))


@pytest.mark.parametrize("name", ref.CASES)
@pytest.mark.parametrize("path", list(PATHS))
def test_bound_table_keeps_the_contract(path, name, tmp):
    metrics, arrays = _child(PATHS[path][0], tmp)
    bad, worst, share = table_errors(name, path, metrics, arrays)
    assert not bad, "\n".join(bad)
    assert metrics[name + "/" + PATHS[path][1]]["nan"] == 0 and abs(metrics[name + "/" + PATHS[path][1]]["share"] - share) < 1e-12


@pytest.mark.parametrize("name", ref.CASES)
@pytest.mark.parametrize("path", list(PATHS))
def test_rowmin_equals_float64(path, name, tmp):
    """d"""
    _, arrays = _child(PATHS[path][0], tmp)
    want = ref.truth(name)["bits"].astype(np.int64)
    got = arrays["%s/%s/rowmin" % (name, PATHS[path][1])].astype(np.int64)
    wrong = np.nonzero(got != want)[0]
    assert wrong.size == 0, "d: rowmin differs from float64 on %d rows, first %d: %#x, float64 %#x" % (wrong.size, wrong[0], got[wrong[0]], want[wrong[0]])


@pytest.mark.parametrize("name", ref.CASES)
def test_rowmin_is_the_same_on_every_path(name, tmp):
    """e, and d against the library's own full float64 Gram and its own caller (range_stats for the tolerance, padding to 256)"""
    first = None
    for path, (config, bound) in PATHS.items():
        got = _child(config, tmp)[1]["%s/%s/rowmin" % (name, bound)]
        first = got if first is None else first
        assert np.array_equal(got, first), "e: rowmin of %s differs from the default path" % path
    extras = _child("default", tmp)[1]
    assert np.array_equal(extras[name + "/exact_gemm"], first), "d: source_vector(exact_gemm=True) differs"
    assert np.array_equal(extras[name + "/exact_gemm"].astype(np.int64), ref.truth(name)["bits"].astype(np.int64)), "d: the float64 Gram differs from float64"
    if ref.case(name).Ns_pad % 256 == 0:
        assert np.array_equal(extras[name + "/source_vector"], first), "d: source_vector differs"


def test_row_block(tmp):
    name, row0, nrows = ROW_BLOCK
    extras = _child("default", tmp)[1]
    assert np.array_equal(extras[name + "/row_block"], extras[name + "/source_vector"][row0:row0 + nrows])
    assert np.array_equal(extras[name + "/row_block"].astype(np.int64), ref.truth(name)["bits"][row0:row0 + nrows].astype(np.int64))


@pytest.mark.parametrize("name", [n for n in ref.CASES if n.startswith("ranges")])
def test_stats_are_upper_bounds(name, tmp):
    """rerank.range_stats (what source_vector derives tol and the scales from) is >= the float64 values"""
    got = _child("default", tmp)[1][name + "/range_stats"]
    c = ref.case(name)
    t = c.tgt.astype(np.float64); s = c.src.astype(np.float64)
    exact = (np.abs(t).max(), np.abs(s).max(), np.sqrt((t * t).sum(1)).max(), np.sqrt((s * s).sum(1)).max())
    for g, e in zip(got, exact):
        assert np.isfinite(g) and g >= e


def measure(tmp):
    """(case, path, granule size, max |table - truth| / (tol / 2), refined share) for tools/source_bound_errors.py"""
    for path, (config, bound) in PATHS.items():
        metrics, arrays = _child(config, tmp)
        for name in ref.CASES:
            bad, worst, share = table_errors(name, path, metrics, arrays)
            yield name, path, metrics[name + "/" + bound]["G"], worst, share, bad
