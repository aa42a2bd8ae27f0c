"""GPU suite (-m gpu): the eps rule and DBSCAN above the oracle's sizes, against the independent reference of tests/grouping_ref.py
(torch element-wise final_dist rows, numpy's mean of the sorted exact candidates, sklearn's DBSCAN on the sparse neighbour graph).

* N = 30 000 (BASELINE configs[3], one split): rows go both through the sparse copy S and through the dense passes; every entry point
  (eps_rule, eps_rule_dbscan, DBSCAN.fit, compute_dist -> generate_selflabel) under every call-time switch of the eps rule;
* N = 128 000 (configs[4]): every row is dense; both eps paths, every row's neighbour count, the labels;
* N = 8 000 / 8 003: mixed rows at a size the oracle also checks; N % 8 == 0 runs the dense region query's float16 pre-filter, N = 8 003
  its exact generic path; lambda = 0.9 pushes on the pre-filter's band.

Every comparison is an equality: each quantity is defined exactly by the reference.  Besides the eps rule's own radius, each size is also
queried at `_floor_radius`, a radius at which the region query must split its rows between S and the dense pass, and which equals the
exact value of many entries (hits with d == eps)."""
import os
import time

import numpy as np
import pytest

from conftest import clustered, hard_clustered

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import grouping_ref as gr  # noqa: E402

SWITCHES = [{}, {"SSG_EPS_PATH": "radix"}, {"SSG_EPS_FUSED": "0"}, {"SSG_EPS_SORT": "bitonic"}]
SWITCH_IDS = ["default", "radix", "unfused", "bitonic"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda", 0)


def _pin_helper(h, rows):
    """the reference's final_dist rows == the numpy restatement of tests/test_gpu_fullsize.py::_check_sampled_rows == ssg_final_dist_f64"""
    from ssg_amd._lib import check, lib, ptr, stream
    v = h.v.cpu().numpy()
    for r in rows:
        ours = gr.final_rows(h.M, h.v, h.lambda_value, r, r + 1).cpu().numpy()[0]
        ref = h.M[r].cpu().numpy().astype(np.float64) + (v + v[r]).astype(np.float64) * h.lambda_value
        out = torch.empty((1, h.N), dtype=torch.float64, device=h.device)
        check(lib().ssg_final_dist_f64(ptr(h.M[r:r + 1]), ptr(h.v), h.N, int(r), 1, h.lambda_value, ptr(out), stream()), "final")
        assert np.array_equal(ours, ref), "row %d: reference vs numpy" % r
        assert np.array_equal(ours, out.cpu().numpy()[0]), "row %d: reference vs ssg_final_dist_f64" % r


def _floor_radius(h):
    """a radius at which about 1 % of the rows must take the dense region query: row i is walked through S only when its floor
    f64(J'(0)) + f64(half(v_i + min v)) * lambda exceeds eps.  The radius is the floor of one row, so it is the exact value of the
    entries outside S that share that row's source term: hits with d == eps."""
    jp0 = float(np.uint16(h.sparse["jp0"]).view(np.float16))
    v = h.v.float()
    floors = jp0 + (v + v.min()).half().double() * h.lambda_value
    return float(torch.sort(floors).values[h.N // 100])


def _device_region(h, eps, cap):
    """per-row neighbour counts and the sorted hit keys i * N + k straight from the region query kernels DBSCAN.fit launches"""
    from ssg_amd._lib import check, lib, ptr, stream
    L, st, dev, N = lib(), stream(), h.device, h.N
    cnt = torch.zeros(h.nrows, dtype=torch.int32, device=dev)
    edges = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    cursor = torch.zeros(2, dtype=torch.int64, device=dev)
    sp = h.sparse
    check(L.ssg_region_query_s(ptr(h.M), ptr(h.v), N, h.row0, h.nrows, h.lambda_value, float(eps), ptr(sp["pool"]), ptr(sp["seg_off"]), ptr(sp["seg_len"]),
                               sp["nseg"], ptr(sp["cursor"]), ptr(sp["vmin"]), sp["jp0"], ptr(sp["rowmask"]), ptr(cnt), ptr(edges), cap, ptr(cursor), st),
          "ssg_region_query_s")
    ne = int(cursor[0].item())
    assert ne <= cap, "the region query found %d hits, the reference %d" % (ne, cap)
    e = edges[:ne].cpu().numpy().astype(np.int64)
    return cnt.cpu().numpy().astype(np.int64), np.sort(e[:, 0] * N + e[:, 1])


class Ref:
    """the reference's answers for one handle: eps rule at rho, region graph + labels at its eps and at `_floor_radius`"""

    def __init__(self, h, rho, hint, name, floor=True):
        t0 = time.time()
        mat = gr.FinalDist(h.M, h.v, h.lambda_value)
        self.rule = gr.eps_rule(mat, rho, hint=hint)
        t1 = time.time()
        self.eps = self.rule.eps
        self.graph = gr.region_graph(mat, self.eps)
        self.keys = gr.hit_keys(self.graph, self.eps)
        self.labels, self.core = gr.dbscan(self.graph, self.eps, 4)
        t2 = time.time()
        self.radii = [(self.eps, self.graph, self.keys, self.labels, self.core)]
        msg = ""
        if floor:
            self.eps_x = _floor_radius(h)
            self.graph_x = gr.region_graph(mat, self.eps_x)
            self.keys_x = gr.hit_keys(self.graph_x, self.eps_x)
            self.labels_x, self.core_x = gr.dbscan(self.graph_x, self.eps_x, 4)
            self.radii.append((self.eps_x, self.graph_x, self.keys_x, self.labels_x, self.core_x))
            msg = "; floor radius %.6f: %d hits, %.1f s" % (self.eps_x, self.graph_x.nhits, time.time() - t2)
        print("%s: reference %.1f s (eps rule %.1f s: count %d, top %d, %d candidates at cap %.6g; region + sklearn %.1f s: %d hits%s)" % (
            name, time.time() - t0, t1 - t0, self.rule.count, self.rule.top, self.rule.ncand, self.rule.cap, t2 - t1, self.graph.nhits, msg), flush=True)

    def rule3(self):
        return (self.eps, self.rule.count, self.rule.top)


def _check_region(h, ref, which=""):
    """the kernels' per-row neighbour counts and hit pairs, and DBSCAN.fit's labels and core set, at each radius of the reference"""
    from ssg_amd import cluster
    for eps, g, keys, lab, core in ref.radii:
        cnt, dkeys = _device_region(h, eps, max(g.nhits, 1 << 16))
        bad = np.nonzero(cnt != g.counts)[0]
        assert bad.size == 0, "%s eps %.17g: %d rows with a wrong neighbour count, first %s: device %s, reference %s" % (
            which, eps, bad.size, bad[:8], cnt[bad[:8]], g.counts[bad[:8]])
        assert np.array_equal(dkeys, keys), "%s eps %.17g: hit pairs" % (which, eps)
        est = cluster.DBSCAN(eps=eps, min_samples=4, metric="precomputed").fit(h)
        assert np.array_equal(est.core_sample_indices_, core), "%s eps %.17g: core samples" % (which, eps)
        assert np.array_equal(est.core_sample_indices_, np.nonzero(g.counts >= 4)[0])
        assert np.array_equal(est.labels_, lab), "%s eps %.17g: labels" % (which, eps)


def _check_chain(h, ref, rho, which):
    """eps_rule and the one-read chain eps_rule_dbscan against the reference"""
    from ssg_amd import cluster
    assert cluster.eps_rule(h, rho) == ref.rule3(), "%s: eps_rule" % which
    e, c, t, lab, core = cluster.eps_rule_dbscan(h, rho, min_samples=4)
    assert (e, c, t) == ref.rule3(), "%s: eps_rule_dbscan eps" % which
    assert np.array_equal(core, ref.core), "%s: eps_rule_dbscan core samples" % which
    assert np.array_equal(lab, ref.labels), "%s: eps_rule_dbscan labels" % which


def _split(h, rho, eps):
    from ssg_amd import cluster
    s = cluster.sparse_row_split(h, rho, eps)
    assert s is not None, "the handle has a sparse copy"
    return s


# ---------------------------------------------------------------------------------------------------- N = 30 000 (configs[3])
N3, NS3, D3, LAM3, RHO3 = 30000, 12936, 2048, 0.1, 1.6e-3


@pytest.fixture(scope="module")
def n30k(dev):
    from ssg_amd import cluster, rerank
    tgt = torch.from_numpy(hard_clustered(N3, D3, 100)).to(dev)
    src = torch.from_numpy(hard_clustered(NS3, D3, 200, intra=0.7)).to(dev)
    h = rerank.re_ranking_device(src, tgt, lambda_value=LAM3)
    hint = cluster.eps_rule(h, RHO3)[0]
    ref = Ref(h, RHO3, hint, "N=%d" % N3)
    yield src, tgt, h, ref
    del h


def test_n30k_rows_mixed_and_reference_pinned(n30k):
    """the region query splits the rows between S and the dense pass; the reference's rows are the kernel's.  (At rho = 1.6e-3 the eps
    rule's threshold lies below every row's floor here: its pass walks every row through S -- the mix of that pass is asserted at
    rho = 0.01 below and at the mid sizes.)"""
    src, tgt, h, ref = n30k
    s = _split(h, RHO3, ref.eps)
    sx = _split(h, RHO3, ref.eps_x)
    print("N=%d: rows (sparse, dense): eps rule %s, region query at eps %s, at the floor radius %s" % (N3, s["eps"], s["region"], sx["region"]))
    assert sx["region"][0] > 0 and sx["region"][1] > 0, "region query at the floor radius: mixed rows"
    _pin_helper(h, [0, 1, 7777, 15000, 29998, 29999])
    _check_region(h, ref, "N=30000")


def test_n30k_eps_rule_with_mixed_rows(n30k):
    """rho = 0.01: the threshold of the eps rule's one pass cuts through the rows' floors -- rows through S and through the dense
    compaction in the same pass -- and (eps, count, top), the neighbour counts and the labels still equal the reference's"""
    from ssg_amd import cluster
    src, tgt, h, _ = n30k
    rho = 0.01
    ref = Ref(h, rho, cluster.eps_rule(h, rho)[0], "N=%d rho=%g" % (N3, rho), floor=False)
    s = _split(h, rho, ref.eps)
    print("N=%d rho=%g: rows (sparse, dense): eps rule %s, region query %s" % (N3, rho, s["eps"], s["region"]))
    assert s["eps"][0] > 0 and s["eps"][1] > 0, "eps rule: mixed rows"
    _check_chain(h, ref, rho, "N=30000 rho=0.01")
    _check_region(h, ref, "N=30000 rho=0.01")


@pytest.mark.parametrize("env", SWITCHES, ids=SWITCH_IDS)
def test_n30k_every_entry_point_vs_reference(env, n30k, monkeypatch):
    """eps_rule, eps_rule_dbscan, DBSCAN.fit and compute_dist -> generate_selflabel == the reference, under each call-time switch"""
    from types import SimpleNamespace
    from ssg_amd import compute_dist, generate_selflabel
    src, tgt, h, ref = n30k
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    which = "N=30000 %s" % (env or "default")
    _check_chain(h, ref, RHO3, which)
    from ssg_amd import cluster
    est = cluster.DBSCAN(eps=ref.eps, min_samples=4, metric="precomputed").fit(h)
    assert np.array_equal(est.labels_, ref.labels) and np.array_equal(est.core_sample_indices_, ref.core), "%s: DBSCAN.fit" % which
    e_list, r_list = compute_dist([src], [tgt], lambda_value=LAM3, no_rerank=False)
    assert torch.equal(r_list[0].M, h.M) and torch.equal(r_list[0].v, h.v), "the pipeline is deterministic"
    args = SimpleNamespace(no_rerank=False, rho=RHO3)
    labels, clusters = generate_selflabel(e_list, r_list, 0, args, [])
    assert clusters[0].eps == ref.eps, "%s: generate_selflabel eps" % which
    assert np.array_equal(labels[0], ref.labels) and np.array_equal(clusters[0].core_sample_indices_, ref.core), "%s: generate_selflabel" % which
    labels1, _ = generate_selflabel(e_list, r_list, 1, args, clusters)
    assert np.array_equal(labels1[0], ref.labels), "%s: generate_selflabel, later iteration" % which


# ---------------------------------------------------------------------------------------------------- N = 128 000 (configs[4])
def test_n128k_eps_counts_labels_vs_reference(dev, monkeypatch):
    """configs[4] with only J' resident (no stages, no euclidean matrix): both eps paths, every row's neighbour count and the hit pairs,
    the labels of DBSCAN.fit and of the one-read chain -- against the reference and sklearn on a graph of ~10^7 stored pairs"""
    from ssg_amd import cluster, rerank
    N, Ns, d, lam, rho = 128000, 12936, 2048, 0.1, 1.6e-3
    tgt = torch.from_numpy(clustered(N, d, 1)).to(dev); src = torch.from_numpy(clustered(Ns, d, 2, intra=0.7)).to(dev)
    h = rerank.re_ranking_device(src, tgt, lambda_value=lam, keep_euclid=False)
    del src, tgt
    dev_rule = cluster.eps_rule(h, rho)
    ref = Ref(h, rho, dev_rule[0], "N=%d" % N, floor=False)     # (every row is dense here: the floor radius would add no mix)
    s = _split(h, rho, ref.eps)
    print("N=%d: rows (sparse, dense): eps rule %s, region query %s" % (N, s["eps"], s["region"]))
    assert dev_rule == ref.rule3(), "eps_rule (sampled path)"
    monkeypatch.setenv("SSG_EPS_PATH", "radix")
    assert cluster.eps_rule(h, rho) == ref.rule3(), "eps_rule (radix select)"
    monkeypatch.delenv("SSG_EPS_PATH")
    _pin_helper(h, [0, 63999, 64000, 127999])
    _check_region(h, ref, "N=128000")
    _check_chain(h, ref, rho, "N=128000")


# ---------------------------------------------------------------------------------------------------- mid-size, also against the oracle
@pytest.mark.parametrize("N,lam,rho", [(8000, 0.3, 0.01), (8003, 0.3, 0.01), (8000, 0.9, 0.01)])
def test_midsize_mixed_rows_vs_reference_and_oracle(N, lam, rho, dev, ora):
    """rows split between S and the dense passes at a size the oracle holds: the reference, the oracle and every device path agree.
    N = 8 000 runs the dense region query's float16 pre-filter, N = 8 003 its generic path; lambda = 0.9 is the top of the range the
    product uses, where the pre-filter's band is widest -- every row's neighbour count is compared"""
    from ssg_amd import cluster, rerank
    ora.set_num_threads(min(os.cpu_count() or 8, 16))
    tgt = torch.from_numpy(hard_clustered(N, 2048, 31)).to(dev); src = torch.from_numpy(hard_clustered(4000, 2048, 32, intra=0.7)).to(dev)
    h = rerank.re_ranking_device(src, tgt, lambda_value=lam)
    ref = Ref(h, rho, cluster.eps_rule(h, rho)[0], "N=%d lambda=%g rho=%g" % (N, lam, rho))
    s = _split(h, rho, ref.eps)
    sx = _split(h, rho, ref.eps_x)
    print("N=%d lambda=%g: rows (sparse, dense): eps rule %s, region query at eps %s, at the floor radius %s" % (N, lam, s["eps"], s["region"], sx["region"]))
    assert s["eps"][0] > 0 and s["eps"][1] > 0, "eps rule: mixed rows"
    assert sx["region"][0] > 0 and sx["region"][1] > 0, "region query at the floor radius: mixed rows"
    _pin_helper(h, [0, N // 2, N - 1])
    final = h.final_dist().cpu().numpy()
    assert ora.eps_rule(final, rho) == ref.rule3(), "reference vs oracle: eps rule"
    assert np.array_equal(ora.dbscan(final, ref.eps, 4), ref.labels), "reference vs oracle: labels"
    assert np.array_equal(ora.dbscan(final, ref.eps_x, 4), ref.labels_x), "reference vs oracle: labels at the floor radius"
    assert np.array_equal(ref.graph_x.counts, (final <= ref.eps_x).sum(axis=1))
    del final
    _check_region(h, ref, "N=%d lambda=%g" % (N, lam))
    _check_chain(h, ref, rho, "N=%d lambda=%g" % (N, lam))


# ---------------------------------------------------------------------------------------------------- the mean above numpy's buffer
@pytest.mark.parametrize("top", [8192, 8193, 16385, 100000])
def test_eps_mean_above_numpy_reduction_buffer(top, dev):
    """np.mean sums in chunks of numpy's buffer size (8192 elements), pairwise inside each chunk: every eps path (re-rank handle, half
    no-rerank matrix, uploaded float64 matrix; sampled, radix, one-read chain) == numpy's own code for more than 8192 summands"""
    from ssg_amd import cluster, rerank
    N = 2048
    tgt = torch.from_numpy(hard_clustered(N, 256, 41)).to(dev); src = torch.from_numpy(hard_clustered(1500, 256, 42, intra=0.7)).to(dev)
    h = rerank.re_ranking_device(src, tgt, lambda_value=0.3)
    final = h.final_dist().cpu().numpy()
    rho = top / (N * (N - 1) // 2)
    ref = gr.numpy_eps_rule(final, rho)
    assert ref[2] == top
    assert cluster.eps_rule(h, rho) == ref, "re-rank handle, sampled path"
    assert cluster.eps_rule_dbscan(h, rho)[:3] == ref, "re-rank handle, one-read chain"
    assert cluster.eps_rule(final, rho) == ref, "uploaded float64 matrix"
    os.environ["SSG_EPS_PATH"] = "radix"
    try:
        assert cluster.eps_rule(h, rho) == ref, "re-rank handle, radix select"
    finally:
        del os.environ["SSG_EPS_PATH"]
    hn = rerank.re_ranking_device(src, tgt, no_rerank=True)
    E = hn.M.cpu().numpy()
    href = gr.numpy_eps_rule(E, rho)
    he, hc, ht = cluster.eps_rule(hn, rho)
    assert (hc, ht) == href[1:] and np.float16(he).view(np.uint16) == np.float16(href[0]).view(np.uint16), "half no-rerank matrix"
