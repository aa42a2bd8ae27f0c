"""Records tests/golden/cmc_sgs_cases.npz: the reference's own single-gallery-shot CMC (reid/evaluation_metrics/ranking.py, cmc with
single_gallery_shot=True) on the cases of tests/cmc_sgs_ref.py.

    python tools/make_golden_cmc_sgs.py /path/to/reference

The reference file is imported by path under a stub `reid.utils.to_numpy` (its relative import).  Its _unique_sample uses np.bool, gone
from numpy 2: np.bool = np.bool_ is set only after sklearn is imported (np.bool = bool breaks numpy.ma).  Tie-free cases run the
reference untouched; cases with equal distances run it with argsort(kind='stable') through a proxy of the module's `np` (numpy's default
argsort leaves the order of ties unspecified; (distance, index) is the order this project documents).  Data only: nothing of the
reference's text is copied.

Per case and (separate_camera_set, first_match_break) setting the file holds the curve (or that the call raised "No valid query"), the
32-bit words the call consumed from the global stream, and the next standard_normal() and random_sample() of that stream; inputs are
stored when small, otherwise their seed and a digest (np.random.RandomState streams are frozen).  The tool asserts that the restatement
agrees and that the case set covers every edge listed in main()."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cmc_sgs_ref as ref  # noqa: E402


class _StableNp(object):
    """numpy with argsort(kind='stable')"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def argsort(a, axis=-1):
        return np.argsort(a, axis=axis, kind="stable")


def load_reference(ref_root):
    import sklearn.metrics  # noqa: F401  (before np.bool exists again)
    np.bool = np.bool_
    for name in ("reid", "reid.evaluation_metrics"):
        pkg = types.ModuleType(name); pkg.__path__ = []
        sys.modules[name] = pkg
    utils = types.ModuleType("reid.utils"); utils.to_numpy = np.asarray
    sys.modules["reid.utils"] = utils
    path = os.path.join(ref_root, "reid", "evaluation_metrics", "ranking.py")
    spec = importlib.util.spec_from_file_location("reid.evaluation_metrics.ranking", path)
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    return mod


def words_between(before, after_rs_state):
    """how many 32-bit words lie between two states of one MT19937 stream"""
    bg = np.random.MT19937()
    bg.state = {"bit_generator": "MT19937", "state": dict(before["state"])}
    target = after_rs_state["state"]
    n = 0
    for _ in range(1 << 26):
        s = bg.state["state"]
        if s["pos"] == target["pos"] and np.array_equal(s["key"], target["key"]):
            return n
        bg.random_raw(1); n += 1
    raise AssertionError("the stream did not reach the state after the call")


def run_reference(mod, case, sep, fmb, seed, tied, gauss=False):
    """-> (curve or None when the call raised 'No valid query', words consumed, next standard_normal, next random_sample)"""
    mod.np = _StableNp() if tied else np
    np.random.seed(seed)
    if gauss:
        np.random.standard_normal()
    before = np.random.get_state(legacy=False)
    try:
        out = mod.cmc(case["dist"], case["qid"], case["gid"], case["qcam"], case["gcam"], topk=case["topk"], separate_camera_set=sep,
                      single_gallery_shot=True, first_match_break=fmb)
    except RuntimeError as e:
        assert str(e) == "No valid query"
        out = None
    after = np.random.get_state(legacy=False)
    assert after["has_gauss"] == before["has_gauss"] and after["gauss"] == before["gauss"]
    consumed = words_between(before, after)
    return out, consumed, np.random.standard_normal(), np.random.random_sample()


def main():
    mod = load_reference(sys.argv[1])
    out = {"cases": np.array(list(ref.CASES))}
    seen_sizes, cover = set(), dict(novalid=False, absent=False, rejections=False, over_topk=False, ties_in=False, ties_across=False,
                                    junk=False, sparse=False, odd_n=False, onecam=False, G1=False, m1=False, big=False)
    for name, c in ref.CASES.items():
        case = ref.make_case(name)
        dist, qid, gid, qcam, gcam = case["dist"], case["qid"], case["gid"], case["qcam"], case["gcam"]
        m, n = dist.shape
        p = name + "_"
        if not c["tied"]:
            assert all(len(np.unique(row)) == n for row in dist), "case %s is meant to be tie-free" % name
        out[p + "seed"] = np.int64(c["seed"]); out[p + "stream"] = np.int64(c["stream"]); out[p + "topk"] = np.int64(c["topk"])
        out[p + "sha256"] = np.array([ref.sha(dist), ref.sha(qid), ref.sha(gid), ref.sha(qcam), ref.sha(gcam)])
        if dist.nbytes <= 48 * 1024:
            out.update({p + "dist": dist, p + "qid": qid, p + "gid": gid, p + "qcam": qcam, p + "gcam": gcam})
        raised = []
        for sep, fmb in ref.SETTINGS:
            tag = p + "s%d_f%d_" % (sep, fmb)
            curve, consumed, nxt_n, nxt_u = run_reference(mod, case, sep, fmb, c["stream"], c["tied"])
            mine = ref.run_case(name, sep)
            assert mine["consumed"] == consumed, (name, sep, fmb, mine["consumed"], consumed)
            rs = np.random.RandomState(0); rs.set_state(mine["state"])
            assert rs.standard_normal() == nxt_n and rs.random_sample() == nxt_u, (name, sep, fmb)
            if curve is None:
                assert (mine["k"] < 0).all()
                raised.append(True)
                curve = np.zeros(0)
            else:
                assert np.array_equal(ref.curve(mine["k"], c["topk"], fmb), curve), (name, sep, fmb)
                raised.append(False)
            out[tag + "curve"] = curve; out[tag + "consumed"] = np.int64(consumed)
            out[tag + "next_normal"] = np.float64(nxt_n); out[tag + "next_uniform"] = np.float64(nxt_u)
            out[p + "s%d_k" % sep] = mine["k"]; out[p + "s%d_draws" % sep] = np.int64(mine["stats"]["draws"])
            # coverage
            k, stats = mine["k"], mine["stats"]
            seen_sizes |= stats["sizes"]
            cover["rejections"] |= consumed > stats["draws"] > 0
            cover["over_topk"] |= bool((k >= c["topk"]).any())
            cover["big"] |= max(stats["sizes"] or [0]) > 256
        out[p + "raised"] = np.array(raised)
        present = np.isin(qid, gid)
        cover["absent"] |= bool((~present).any())
        cover["novalid"] |= any(present[i] and not ((gid == qid[i]) & (gcam != qcam[i])).any() for i in range(m)) and not all(raised)
        cover["junk"] |= bool((gid == -1).any()); cover["sparse"] |= bool((gid > 10 ** 9).any())
        cover["odd_n"] |= n % 64 != 0
        cover["onecam"] |= all(raised) and len(set(gcam.tolist()) | set(qcam.tolist())) == 1
        cover["G1"] |= len(np.unique(gid)) == 1; cover["m1"] |= m == 1
        if c["tied"] and n <= 2000:
            for i in range(m):
                same = dist[i][:, None] == dist[i][None, :]
                np.fill_diagonal(same, False)
                sid = gid[:, None] == gid[None, :]
                cover["ties_in"] |= bool((same & sid).any()); cover["ties_across"] |= bool((same & ~sid).any())
        print("case %-10s m=%d n=%d G=%d raised=%s" % (name, m, n, len(np.unique(gid)), raised))
    # the cached Gaussian: one case once more with standard_normal() called before the protocol
    name = ref.GAUSS_CASE
    c = ref.CASES[name]
    curve, consumed, nxt_n, nxt_u = run_reference(mod, ref.make_case(name), True, False, c["stream"], c["tied"], gauss=True)
    mine = ref.run_case(name, True, gauss=True)
    rs = np.random.RandomState(0); rs.set_state(mine["state"])
    assert mine["consumed"] == consumed and rs.standard_normal() == nxt_n and rs.random_sample() == nxt_u
    assert np.array_equal(ref.curve(mine["k"], c["topk"], False), curve)
    out.update({"gauss_curve": curve, "gauss_consumed": np.int64(consumed), "gauss_next_normal": np.float64(nxt_n), "gauss_next_uniform": np.float64(nxt_u)})
    # the edges no test may miss
    need = {1, 2, 3, 5, 4, 8, 16, 32, 9, 17, 33}
    assert need <= seen_sizes, "group sizes never met: %s" % sorted(need - seen_sizes)
    assert all(cover.values()), "not covered: %s" % [k for k, v in cover.items() if not v]
    path = os.path.join(ROOT, "tests", "golden", "cmc_sgs_cases.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1000000
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
