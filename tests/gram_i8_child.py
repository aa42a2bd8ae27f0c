"""Child process of tests/test_gpu_gram_i8.py (SSG_I8_DMA, SSG_I8_SB and SSG_I8_KB2 of csrc/gram_i8.hip are read once per process: one
child per configuration).  `gram_i8_child.py OUT.npz CONFIG`: every case of tests/gram_i8_ref.py that runs under CONFIG through the C entry
points ssg_gram_i8_encode and ssg_sqdist_self_i8 -- the whole matrix and every listed stripe, D pre-filled with 0xFFFF and rowmax with a
sentinel, the calls that take the LDS-DMA kernel once with SSG_I8_DMA_STAGES=3 and once with 4 (that knob is read per call).  OUT.npz:
    <case>/E, /norms, /flag                          the encoder's outputs (E pre-filled with 0x55)
    <case>/s<3|4|0>/<row0>_<nrows>/D, /rowmax        s0: the register-staged kernel (no stage knob)
    flag/<name>/rc, /flag, /D                        direct calls on inputs that do not fit the digit count
    pylayer/raised                                   1: SSG_SELF_GRAM_DIGITS=3 on max|feat| = 0.6 raised SSGError through rerank
    public/<case>/ms<0|1>                            re_ranking_device(no_rerank=True).euclid
Prints one JSON line: the number of cases and of ssg_sqdist_self_i8 calls."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import gram_i8_ref as ref                   # noqa: E402
from ssg_amd import _lib, rerank            # noqa: E402
from ssg_amd._lib import check, ptr, stream  # noqa: E402

ROWMAX_SENTINEL = 0x5A5A5A5A
# name -> (base case, digits, the entry written into row 40, column 17)
FLAG_CASES = {"half_3dig": ("unit_n200_d128_3dig", 3, 0.5), "nan_3dig": ("unit_n200_d128_3dig", 3, float("nan")),
              "inf_3dig": ("unit_n65_d33_3dig", 3, float("inf")), "over1_4dig": ("wide_n65_d40_4dig", 4, 1.0009765625)}
PUBLIC = ("unit_n385_d160_3dig", "antipodal_n66_d8192_4dig", "antipodal_n66_d16384_4dig")


def encode(L, dev, x, nd):
    N, d = x.shape
    X = torch.from_numpy(np.array(x)).to(dev)
    E = torch.full((L.ssg_gram_i8_encoded_bytes(N, d, nd),), 0x55, dtype=torch.int8, device=dev)
    norms = torch.full((N,), -1, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    check(L.ssg_gram_i8_encode(ptr(X), N, d, nd, ptr(E), ptr(norms), ptr(flag), stream()), "ssg_gram_i8_encode")
    return E, norms, flag


def sqdist(L, dev, E, norms, flag, N, d, nd, row0, nrows, memory_save):
    D = torch.full((nrows, N), -1, dtype=torch.int16, device=dev)                 # 0xFFFF everywhere
    rowmax = torch.full((nrows,), ROWMAX_SENTINEL, dtype=torch.int32, device=dev)
    rc = L.ssg_sqdist_self_i8(ptr(E), ptr(norms), N, d, nd, row0, nrows, memory_save, ptr(D), ptr(rowmax), ptr(flag), stream())
    torch.cuda.synchronize()
    return rc, D.cpu().numpy().view(np.uint16), rowmax.cpu().numpy().view(np.uint32)


def main():
    path, config = sys.argv[1], sys.argv[2]
    env = ref.CONFIGS[config]
    assert all(os.environ.get(k) == v for k, v in env.items()) and not any(k in os.environ for k in ("SSG_I8_DMA", "SSG_I8_SB", "SSG_I8_KB2") if k not in env)
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    out = {}
    calls = 0
    for name in ref.cases_of(config):
        c = ref.CASES[name]
        E, norms, flag = encode(L, dev, ref.inputs(name), c.nd)
        torch.cuda.synchronize()
        out[name + "/E"] = E.cpu().numpy(); out[name + "/norms"] = norms.cpu().numpy(); out[name + "/flag"] = flag.cpu().numpy()
        for ns in ((3, 4) if ref.use_dma(c.N, c.d, c.nd, env) else (0,)):
            if ns:
                os.environ["SSG_I8_DMA_STAGES"] = str(ns)
            for row0, nrows in ((0, c.N),) + c.stripes:
                rc, D, rowmax = sqdist(L, dev, E, norms, flag, c.N, c.d, c.nd, row0, nrows, c.memory_save)
                check(rc, "ssg_sqdist_self_i8")
                calls += 1
                key = "%s/s%d/%d_%d/" % (name, ns, row0, nrows)
                out[key + "D"] = D; out[key + "rowmax"] = rowmax
            os.environ.pop("SSG_I8_DMA_STAGES", None)

    # ---- inputs that do not fit: the flag goes up, the multiply returns SSG_OK and writes nothing
    for fname, (base, nd, v) in FLAG_CASES.items():
        x = np.array(ref.inputs(base)); x[40, 17] = v
        E, norms, flag = encode(L, dev, x, nd)
        rc, D, _ = sqdist(L, dev, E, norms, flag, x.shape[0], x.shape[1], nd, 0, x.shape[0], 0)
        out["flag/%s/rc" % fname] = np.int64(rc); out["flag/%s/flag" % fname] = flag.cpu().numpy(); out["flag/%s/D" % fname] = D

    # ---- the Python layer: a forced digit count that does not fit must raise, not return a matrix
    x = np.array(ref.inputs("unit_n200_d128_3dig")); x[5, 9] = 0.6
    os.environ["SSG_SELF_GRAM_DIGITS"] = "3"
    try:
        rerank.re_ranking_device(torch.from_numpy(x[:50].copy()).to(dev), torch.from_numpy(x).to(dev), no_rerank=True)
        out["pylayer/raised"] = np.int64(0)
    except _lib.SSGError:
        out["pylayer/raised"] = np.int64(1)
    finally:
        del os.environ["SSG_SELF_GRAM_DIGITS"]

    # ---- the public surface (rerank._original_distance picks the digit count from max|feat|)
    for name in PUBLIC:
        if name in ref.cases_of(config):
            x = torch.from_numpy(np.array(ref.inputs(name))).to(dev)
            for ms in (0, 1):
                h = rerank.re_ranking_device(x[:50].clone(), x, no_rerank=True, memory_save=bool(ms))
                out["public/%s/ms%d" % (name, ms)] = h.euclid.cpu().numpy().view(np.uint16)

    np.savez(path, **out)
    print(json.dumps({"cases": len(ref.cases_of(config)), "calls": calls}))


if __name__ == "__main__":
    main()
