"""Records tests/golden/verify_cases.npz: what the reference's verification protocol (reid/evaluation_metrics/eval_far_gar.py,
findMetricThreshold_MPI) prints and computes on the cases of tests/verify_ref.py.

    python tools/make_golden_verify.py /path/to/reference

The reference file imports mpi4py; a stub that models ONE rank stands in for it (below: rank 0 of 1, identity allreduce, copying
Allgather / Allgatherv, allgather(x) -> [x]).  The reference returns nothing, so the values of its local variables are read from the
frame when the function returns.  It only survives its own np.hstack (:156-157) when every query has equally many gallery matches:
all recorded cases are built that way.  Data only: nothing of the reference's text is copied.

For every case the `exact` restatement must print the reference's lines; a case whose %.4f fields differ between float32 and float64
sums is refused (pick another seed in tests/verify_ref.py)."""
import contextlib
import hashlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import verify_ref  # noqa: E402


class _OneRankComm(object):
    def Get_rank(self):
        return 0

    def Get_size(self):
        return 1

    def allreduce(self, x, op=None):
        return x

    def allgather(self, x):
        return [x]

    def Allgather(self, send, recv):
        np.asarray(recv).reshape(-1)[:] = np.asarray(send).reshape(-1)

    def Allgatherv(self, send, recv):
        np.asarray(recv[0]).reshape(-1)[:] = np.asarray(send).reshape(-1)


def _stub_mpi4py():
    pkg = types.ModuleType("mpi4py"); mpi = types.ModuleType("mpi4py.MPI")
    mpi.COMM_WORLD = _OneRankComm()
    mpi.SUM, mpi.MAX, mpi.MIN = "sum", "max", "min"
    pkg.MPI = mpi
    sys.modules["mpi4py"] = pkg; sys.modules["mpi4py.MPI"] = mpi


def _load_reference(ref_root):
    _stub_mpi4py()
    path = os.path.join(ref_root, "reid", "evaluation_metrics", "eval_far_gar.py")
    spec = importlib.util.spec_from_file_location("ref_eval_far_gar", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run_reference(mod, case):
    """-> (printed text, locals of findMetricThreshold_MPI at return, return value of CalClassificationError_MPI or None)"""
    grabbed = {}

    def prof(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "findMetricThreshold_MPI":
            grabbed["locals"] = dict(frame.f_locals)
        if event == "return" and frame.f_code.co_name == "CalClassificationError_MPI":
            grabbed["cls"] = arg

    n = case["n"]
    dist = case["dist"][:, :n].copy()                       # the reference overwrites it
    buf = io.StringIO()
    sys.setprofile(prof)
    try:
        with contextlib.redirect_stdout(buf):
            mod.findMetricThreshold_MPI(case["x"], case["ql"], case["y"], case["rl"], dist=dist)
    finally:
        sys.setprofile(None)
    return buf.getvalue(), grabbed["locals"], grabbed.get("cls")


def main():
    ref_root = sys.argv[1]
    mod = _load_reference(ref_root)
    out = {"cases": np.array(verify_ref.CASES)}
    for name in verify_ref.CASES:
        case = verify_ref.make_case(name)
        assert case["balanced"]
        n = case["n"]
        text, loc, cls = _run_reference(mod, case)
        lines = text.split("\n")[:-1]
        exact = verify_ref.find_metric_threshold(case["ql"], case["rl"], case["dist"][:, :n], mode="exact")
        r32 = verify_ref.find_metric_threshold(case["ql"], case["rl"], case["dist"][:, :n], mode="ref32")
        assert exact["lines"] == lines, "case %s: the exact restatement prints other lines than the reference (pick another seed)\n%s\n%s" % (
            name, "\n".join(lines), "\n".join(exact["lines"]))
        assert r32["lines"] == lines, name
        if name == "b":                                     # every selected rank inside a run of equal values
            srt = exact["inter_sorted"]
            for k in exact["num"]:
                assert (k > 0 and srt[k - 1] == srt[k]) or srt[k + 1] == srt[k], "case b: rank %d is not inside a run of ties" % k
        if name == "e":
            assert exact["too_bad"]
        if name == "c":
            d = case["dist"][:, :n]
            assert (d < 0).any() and (d == 0).any()
        p = "%s_" % name
        out[p + "seed"] = np.int64(verify_ref.SEEDS[name])
        out[p + "sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(case["dist"]).tobytes()).digest(), dtype=np.uint8)
        if case["dist"].nbytes <= 100 * 1024:
            out[p + "dist"] = case["dist"]
        out[p + "ql"] = case["ql"]; out[p + "rl"] = case["rl"]
        out[p + "lines"] = np.array(lines)
        out[p + "intra_num"] = np.int64(loc["intra_num"]); out[p + "inter_num"] = np.int64(loc["inter_num"])
        for k in ("intra_sum", "intra_sum2", "inter_sum", "inter_sum2", "intra_avg", "inter_avg", "intra_std", "inter_std"):
            assert np.asarray(loc[k]).dtype == np.float32, (k, np.asarray(loc[k]).dtype)
            out[p + k] = np.float32(loc[k])
        out[p + "intra_min"] = np.float32(loc["local_intra_min"]); out[p + "intra_max"] = np.float32(loc["local_intra_max"])
        out[p + "inter_min"] = np.float32(loc["local_inter_min"]); out[p + "inter_max"] = np.float32(loc["local_inter_max"])
        srt = np.asarray(loc["inter_v"], dtype=np.float32)
        far = [0.01, 0.001, 0.0001, 0.00001]
        num = [int(f * int(loc["inter_num"])) for f in far]
        out[p + "num"] = np.array(num, dtype=np.int64)
        out[p + "thr"] = srt[num]
        pos = np.asarray(loc["intra_v"], dtype=np.float32)
        out[p + "cnt"] = np.array([int((pos < t).sum()) for t in srt[num]], dtype=np.int64)
        out[p + "too_bad"] = np.bool_(cls is None)
        if cls is not None:
            out[p + "thresholds"] = np.asarray(loc["thres"], dtype=np.float64)
            out[p + "pos_err_rate"] = np.asarray(cls[0], dtype=np.float64); out[p + "neg_err_rate"] = np.asarray(cls[1], dtype=np.float64)
        print("case %s: m=%d n=%d\n  %s" % (name, case["dist"].shape[0], n, "\n  ".join(lines)))
    path = os.path.join(ROOT, "tests", "golden", "verify_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
