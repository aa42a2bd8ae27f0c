#!/usr/bin/env python3
"""Generate tests/golden/hausdorff_cases.npz by running the reference's reid/rerank_hausdorff.py (loaded by path, as
tools/make_golden.py loads rerank.py; needs numpy + scipy and the reference tree, so it runs in the development container only --
no test reads this script).  Per case: the two feature matrices, the parameters and the reference's two returns (of the exactly symmetric final_dist the
upper triangle, to keep the file under the size limit of a committed file).  The numpy
restatement tests/hausdorff_ref.py is held against every case while generating; a disagreement fails the run.

Usage: python tools/make_golden_hausdorff.py [reference root, default /root/reference]
"""
import importlib.util
import os
import sys
import time

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "hausdorff_cases.npz")

import hausdorff_ref  # noqa: E402


def load_ref():
    spec = importlib.util.spec_from_file_location("ref_rerank_hausdorff", os.path.join(REF, "reid", "rerank_hausdorff.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.print = lambda *a, **k: None
    return m


def track_g(N, Ns, d, seed):
    """clustered unit-norm rows (SURVEY.md 8d Track G): N/16 identities (at least 2), x = c_p + sigma n with sigma^2 d = 1/3;
    the source rows come from centres of their own"""
    rng = np.random.default_rng(seed)
    P = max(2, N // 16)
    sigma = (1.0 / (3.0 * d)) ** 0.5

    def draw(n, P):
        c = rng.standard_normal((P, d)); c /= np.linalg.norm(c, axis=1, keepdims=True)
        x = c[np.arange(n) % P] + sigma * rng.standard_normal((n, d))
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return draw(Ns, max(1, Ns // 16)), draw(N, P)


def cases():
    yield "a", track_g(48, 16, 2048, 11), dict(k=6, lambda_value=0.1)
    yield "b", track_g(160, 64, 256, 12), dict(k=20, lambda_value=0.3)
    yield "c", track_g(33, 1, 7, 13), dict(k=2, lambda_value=0.1)
    # 16 rows present two or three times: zero distances, ties at the k-th distance (sets larger than k)
    src, base = track_g(64, 20, 40, 14)
    tgt = base.copy()
    tgt[16:32] = base[:16]
    tgt[32:40] = base[:8]
    yield "d", (src, tgt[np.random.default_rng(15).permutation(64)]), dict(k=4, lambda_value=0.1)
    yield "e", track_g(120, 30, 64, 16), dict(k=8, lambda_value=0.2, MemorySave=True, Minibatch=50)


def main():
    ref = load_ref()
    out = {"names": []}
    for name, (src, tgt), kw in cases():
        t0 = time.time()
        e, f = ref.re_ranking(src, tgt, **kw)
        dt = time.time() - t0
        assert e.dtype == np.float16 and f.dtype == np.float64 and not np.isnan(f).any()
        r = hausdorff_ref.re_ranking(src, tgt, kw["k"], kw["lambda_value"], kw.get("MemorySave", False))
        assert np.array_equal(r["euclidean_dist"].view(np.uint16), e.view(np.uint16)), "restatement: euclidean_dist differs in case " + name
        assert np.array_equal(r["final_dist"], f), "restatement: final_dist differs in case " + name
        sizes = [len(s) for s in r["sets"]]
        print("case %s: N=%d Ns=%d d=%d k=%d  reference %.2f s (%.3f ms per pair)  set sizes %d..%d" %
              (name, tgt.shape[0], src.shape[0], tgt.shape[1], kw["k"], dt, 2e3 * dt / (tgt.shape[0] * (tgt.shape[0] - 1)), min(sizes), max(sizes)))
        out["names"].append(name)
        out[name + "_src"], out[name + "_tgt"] = src, tgt
        out[name + "_params"] = np.array([kw["k"], kw["lambda_value"], float(kw.get("MemorySave", False)), kw.get("Minibatch", 2000)], dtype=np.float64)
        # final_dist is exactly symmetric (checked here): its upper triangle is stored, hausdorff_ref.load_cases mirrors it back
        assert np.array_equal(f, f.T)
        out[name + "_euclidean_dist"], out[name + "_final_dist_triu"] = e, f[np.triu_indices(f.shape[0])]
    out["names"] = np.array(out["names"])
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
