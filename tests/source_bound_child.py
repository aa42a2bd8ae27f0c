"""Child process of tests/test_gpu_source_bound.py (the SSG_SB_* knobs of csrc/source_term.hip are cached per process: one child per
configuration).  `source_bound_child.py OUT.npz half[,split,f32] [extras]`: every case of tests/source_bound_ref.py through the C entry
points (ssg_source_rowmin_filtered1 for "half", ssg_source_rowmin_filtered with scales > 0 for "split" and scales 0 for "f32") on a
workspace the test owns, pre-filled with NaN; tol and scales from rerank.source_bound_params on the float64 stats.  OUT.npz gets, per
case and bound, the bound table [nrows, ld], the two norm vectors and rowmin; with `extras` also what rerank.source_vector returns
(filter-and-refine, full float64 Gram, a row block) and rerank.range_stats.  Prints one JSON line: case/bound -> granule size, table
width, NaNs left in the table, share of the granules the refine pass re-evaluates."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import source_bound_ref as ref               # noqa: E402
from ssg_amd import _lib, rerank            # noqa: E402
from ssg_amd._lib import check, ptr, stream  # noqa: E402

ROW_BLOCK = ("perm_d96", 37, 200)


def run(L, dev, name, bound, knobs):
    c = ref.case(name)
    nrows, d = c.tgt.shape; Ns = c.src.shape[0]
    tol, st, ss, nws = rerank.source_bound_params(ref.stats64(c.tgt, c.src), d, bound, nrows, c.Ns_pad)
    G = ref.granule_of(nrows, c.Ns_pad, d, knobs) if bound == "half" else 8
    ld = c.Ns_pad // G
    assert nrows + c.Ns_pad + nrows * ld <= nws
    tgt = torch.from_numpy(c.tgt).to(dev); src = torch.from_numpy(ref.pad_rows(c.src, c.Ns_pad)).to(dev)
    ws = torch.full((nws,), float("nan"), dtype=torch.float32, device=dev)
    rowmin = torch.full((nrows,), -1, dtype=torch.int32, device=dev)
    fn = L.ssg_source_rowmin_filtered1 if bound == "half" else L.ssg_source_rowmin_filtered
    check(fn(ptr(tgt), ptr(src), nrows, Ns, c.Ns_pad, d, tol, st, ss, ptr(ws), ptr(rowmin), stream()), "ssg_source_rowmin_filtered")
    torch.cuda.synchronize()
    w = ws.cpu().numpy()
    t0 = nrows + c.Ns_pad
    table = w[t0:t0 + nrows * ld].reshape(nrows, ld)
    padded = (np.arange(ld) * G) >= Ns
    share = float(ref.refine_set(np.nan_to_num(table, nan=np.inf), tol, padded).sum()) / (nrows * int((~padded).sum()))
    arrays = {"table": table, "rowterm": w[:nrows], "colterm": w[nrows:t0], "rowmin": rowmin.cpu().numpy()}
    return arrays, {"G": G, "ld": ld, "nan": int(np.isnan(table).sum()), "share": share}


def extras(dev, out):
    for name in ref.CASES:
        c = ref.case(name)
        tgt = torch.from_numpy(c.tgt).to(dev); src = torch.from_numpy(c.src).to(dev)
        out[name + "/exact_gemm"] = rerank.source_vector(src, tgt, exact_gemm=True).cpu().numpy()
        if c.Ns_pad % 256 == 0:                       # (source_vector pads the sources to 256 itself: half_tile has no such call)
            out[name + "/source_vector"] = rerank.source_vector(src, tgt, exact_gemm=False).cpu().numpy()
        if name.startswith("ranges"):
            out[name + "/range_stats"] = np.asarray(rerank.range_stats(tgt, src), np.float64)
        if name == ROW_BLOCK[0]:
            out[name + "/row_block"] = rerank.source_vector(src, tgt, row0=ROW_BLOCK[1], nrows=ROW_BLOCK[2], exact_gemm=False).cpu().numpy()


def main():
    path, bounds = sys.argv[1], sys.argv[2].split(",")
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    knobs = {k: os.environ[k] for k in ("SSG_SB_DMA", "SSG_SB_GRAN") if k in os.environ}
    out, metrics = {}, {}
    for name in ref.CASES:
        for bound in bounds:
            arrays, metrics[name + "/" + bound] = run(L, dev, name, bound, knobs)
            for k, v in arrays.items():
                out["%s/%s/%s" % (name, bound, k)] = v
    if sys.argv[3:] == ["extras"]:
        extras(dev, out)
    np.savez(path, **out)
    print(json.dumps(metrics))


if __name__ == "__main__":
    main()
