"""GPU suite (-m gpu): `rerank.re_ranking_device` over the whole k1 / k2 / lambda / N range it accepts -- the case table of
tests/rerank_grid_ref.py -- against tests/golden/rerank_kgrid.npz (the UNTOUCHED reference's outputs) and the C oracle (checked
against the reference on these very inputs by tools/make_golden.py and tests/test_rerank_grid_host.py), bit for bit at every stage
boundary; the guess / redo protocol of the query expansion where the first guess misses; the first-generation Jaccard kernel and
the dense passes against the defaults; the limits of the range.

Run as a script (`python tests/test_gpu_rerank_grid.py <case> ...`) it prints one JSON line per case: sha256 of J', eps and labels at
both rho under the environment it was started with -- the child process of `test_jaccard_generation_1_equals_the_default`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rerank_grid_ref as grid
from conftest import bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ALL = [c.name for c in grid.CASES]
NUM = {int(c.name[1:3]): c for c in grid.CASES}
MISSES = [NUM[n].name for n in (9, 13, 14, 15)]           # query expansion runs and the longest V row exceeds the first guess of 64
SETTINGS = [NUM[n].name for n in (1, 10, 20, 21)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def g(golden):
    return golden(grid.FIXTURE)


@pytest.fixture()
def empty_guess_table():
    """the query expansion's remembered guesses, emptied for the test and put back after it"""
    from ssg_amd import rerank
    old = dict(rerank._QE_GUESS)
    rerank._QE_GUESS.clear()
    yield rerank._QE_GUESS
    rerank._QE_GUESS.clear(); rerank._QE_GUESS.update(old)


def _run(c, dev, **kw):
    from ssg_amd import rerank
    src, tgt = grid.inputs(c)
    return rerank.re_ranking_device(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), k1=c.k1, k2=c.k2, lambda_value=c.lam, **kw)


def _eps_and_labels(h):
    """[(eps, count, top_num, labels | None)] at both rho through the handle"""
    from ssg_amd import cluster
    out = []
    for rho in grid.RHOS:
        eps, cnt, top = cluster.eps_rule(h, rho)
        lab = cluster.DBSCAN(eps=eps, min_samples=4, metric="precomputed").fit_predict(h).tolist() if top > 0 else None
        out.append([eps, cnt, top, lab])
    return out


def _summary(h):
    return dict(jp=grid.sha(h.M.cpu().numpy()), eps=_eps_and_labels(h))


_DEFAULTS = {}


def _default_summary(c, dev):
    """J', eps and labels of the default run of a case (second-generation Jaccard kernel, sparse copy where there is one): once per process"""
    if c.name not in _DEFAULTS:
        _DEFAULTS[c.name] = _summary(_run(c, dev))
    return _DEFAULTS[c.name]


# ------------------------------------------------------------------ every case, every stage boundary
@pytest.mark.parametrize("name", ALL)
def test_grid_case_vs_reference(name, g, dev, ora, empty_guess_table):
    from ssg_amd import cluster
    c = grid.BY_NAME[name]
    N = c.N
    src, tgt, oe, of, ost = grid.oracle_run(ora, c)
    st = {}
    h = _run(c, dev, stages=st)
    grid.check_stage(g, c, "euclid", st["D"].cpu().numpy(), oe)
    assert np.array_equal(bits(st["v"].cpu().numpy()), bits(ost["v"])), "source vector"
    rank = st["rank"].cpu().numpy()
    assert np.array_equal(rank, ost["rank"]), "initial rank (oracle, all %d columns)" % ost["rank"].shape[1]
    assert np.array_equal(rank[:, :g[name + "__rank"].shape[1]], g[name + "__rank"]), "initial rank (reference)"
    V = grid.sparse_to_dense(st["v_idx"], st["v_val"], st["v_nnz"], N)
    grid.check_stage(g, c, "V", V, ost["V"])
    assert int(st["v_nnz"].max().item()) == int(g[name + "__vmax"])
    Vq = grid.sparse_to_dense(st["q_idx"], st["q_val"], st["q_nnz"], N)
    grid.check_stage(g, c, "V_qe", Vq, ost["V_qe"])
    Jp = bits(st["Jp"].cpu().numpy())
    assert np.array_equal(Jp, bits(ost["jaccard_scaled"])), "J': %s" % grid.first_difference(Jp, bits(ost["jaccard_scaled"]))
    if c.lam == 0.0:
        grid.check_stage(g, c, "jaccard", Jp, ost["jaccard"])                   # half(1 - lambda) = 1: J' is the reference's jaccard_dist itself
    final = h.final_dist().cpu().numpy()
    grid.check_stage(g, c, "final", final, of)
    assert (h.sparse is None) == bool(grid.derived(c)["om_bits"] & 0x8000)      # negative J': first-generation kernel, no sparse copy
    # eps rule and DBSCAN through the handle, then through the materialised float64 matrix (the sklearn drop-in path)
    grid.check_eps_and_labels(g, c, lambda rho: cluster.eps_rule(h, rho),
                              lambda eps: cluster.DBSCAN(eps=eps, min_samples=4, metric="precomputed", n_jobs=8).fit_predict(h), "handle")
    grid.check_eps_and_labels(g, c, lambda rho: cluster.eps_rule(final, rho),
                              lambda eps: cluster.DBSCAN(eps=eps, min_samples=4, metric="precomputed").fit_predict(final), "float64 matrix")


# ------------------------------------------------------------------ guess / redo protocol of the query expansion
@pytest.mark.parametrize("name", MISSES)
def test_first_guess_misses_and_is_redone(name, g, dev, ora, empty_guess_table, monkeypatch):
    """from an empty guess table the query expansion runs on 64 entries per V row; the longest row of these cases is longer: the call
    reports the miss through the status words, `validate` redoes the tail sized by the reported length and the guess for this k1 grows
    to at least that length; a second call is not redone; the exact-bound path (SSG_QE_GUESS=0) gives the same bits"""
    c = grid.BY_NAME[name]
    vmax = int(g[name + "__vmax"])
    want = bits(grid.oracle_run(ora, c)[4]["jaccard_scaled"])
    assert vmax > grid.QE_FIRST_GUESS and not empty_guess_table
    h = _run(c, dev, validate=False)
    assert h._pending is not None and h._redo is not None
    stale = h.M.clone()
    h.validate()
    assert h._pending is None and h._redo is None and not torch.equal(stale, h.M), "the truncated matrix was not rebuilt"
    assert empty_guess_table[(c.k1, None)] >= vmax
    first = bits(h.M.cpu().numpy())
    assert np.array_equal(first, want), grid.first_difference(first, want)
    h2 = _run(c, dev, validate=False)
    before = h2.M.clone()
    h2.validate()
    assert torch.equal(before, h2.M) and np.array_equal(bits(h2.M.cpu().numpy()), first), "a sufficient guess was redone, or gave other bits"
    monkeypatch.setenv("SSG_QE_GUESS", "0")
    h3 = _run(c, dev)
    assert h3._redo is None and np.array_equal(bits(h3.M.cpu().numpy()), first)


def test_k2_1_has_no_guess(dev, empty_guess_table):
    """k2 == 1 (here with V rows of up to 129 entries): no query expansion, nothing is guessed, nothing is redone, nothing is remembered"""
    c = NUM[10]
    h = _run(c, dev, validate=False)
    assert h._redo is None
    before = h.M.clone()
    h.validate()
    assert torch.equal(before, h.M) and not empty_guess_table


# ------------------------------------------------------------------ Jaccard kernel generations, dense passes, sparse copy
@pytest.mark.parametrize("name", SETTINGS)
def test_dense_passes_equal_the_default(name, dev, monkeypatch):
    """SSG_SPARSE=0 (no sparse copy: the eps rule and the region query stream the N x N matrix): J', eps and labels of the default run"""
    c = grid.BY_NAME[name]
    ref = _default_summary(c, dev)
    monkeypatch.setenv("SSG_SPARSE", "0")
    h = _run(c, dev)
    assert h.sparse is None
    assert _summary(h) == ref


def test_jaccard_generation_1_equals_the_default(dev):
    """SSG_JACCARD_GEN=1 (the first-generation row kernel; the library reads the variable once per process: a child process runs the
    four cases): J', eps and labels of the default run"""
    here = os.path.abspath(__file__)
    env = dict(os.environ, SSG_JACCARD_GEN="1")
    r = subprocess.run([sys.executable, here] + SETTINGS, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            rec = json.loads(line)
            got[rec.pop("name")] = rec
    assert sorted(got) == sorted(SETTINGS)
    for name in SETTINGS:
        assert got[name].pop("sparse") is False, name
        assert got[name] == json.loads(json.dumps(_default_summary(grid.BY_NAME[name], dev))), name


@pytest.mark.parametrize("n", [20, 21])
def test_sparse_copy_at_lambda_0_and_1(n, dev):
    """lambda = 0: the sparse copy's constant is half(1.0) and J' holds exact zeros; lambda = 1: the constant and every entry are 0.
    The copy is complete and consistent with the dense rows (the eps rule through it is compared with the dense passes above)."""
    from test_gpu_parity import _check_sparse_copy
    c = NUM[n]
    h = _run(c, dev)
    assert h.sparse_complete() and h.sparse["jp0"] == grid.derived(c)["om_bits"] == (0x3C00 if c.lam == 0.0 else 0)
    _check_sparse_copy(h, c.N)
    if c.lam == 1.0:
        assert not h.M.view(torch.int16).any()


# ------------------------------------------------------------------ the limits of the range
def test_limits_are_refused_before_any_launch(dev, ora, monkeypatch):
    from ssg_amd import rerank, _lib
    c = NUM[1]
    src, tgt = (torch.from_numpy(x).to(dev) for x in grid.inputs(c))
    for kw in (dict(k1=64, k2=6), dict(k1=20, k2=65), dict(k1=0, k2=6), dict(k1=20, k2=0)):
        with pytest.raises(ValueError, match="1 <= k1 <= 63 and 1 <= k2 <= 64"):
            rerank.re_ranking_device(src, tgt, lambda_value=0.3, **kw)
    assert rerank.re_ranking_device(src, tgt, k1=63, k2=64, lambda_value=0.3) is not None          # the corner itself works on this input
    # a combination whose staged rows do not fit the LDS (here: the library's answer replaced by "does not fit"): a ValueError that names
    # k1, k2 and the longest row, raised before the expansion is launched; the side stream is joined -- the next call is sound
    L = _lib.lib()
    monkeypatch.setattr(L, "ssg_query_expand_rows_per_group", lambda *a: 0)
    with pytest.raises(ValueError, match=r"k1=20, k2=6 with a longest k-reciprocal row of 64 entries"):
        rerank.re_ranking_device(src, tgt, k1=20, k2=6, lambda_value=0.3)
    monkeypatch.undo()
    c6 = NUM[6]
    h = _run(c6, dev)
    assert np.array_equal(bits(h.M.cpu().numpy()), bits(grid.oracle_run(ora, c6)[4]["jaccard_scaled"]))


if __name__ == "__main__":
    device = torch.device("cuda", 0)
    for case_name in sys.argv[1:]:
        handle = _run(grid.BY_NAME[case_name], device)
        print(json.dumps(dict(name=case_name, sparse=handle.sparse is not None, **_summary(handle))), flush=True)
