"""CPU suite of the Hausdorff re-ranking variant (reid/rerank_hausdorff.py): the numpy restatement tests/hausdorff_ref.py against the
goldens the reference itself wrote (tools/make_golden_hausdorff.py), and every refusal that needs no GPU."""
import os

import numpy as np
import pytest

import hausdorff_ref
from conftest import GOLDEN, bits

CASES = hausdorff_ref.load_cases(os.path.join(GOLDEN, "hausdorff_cases.npz"))


def test_golden_file_holds_the_five_cases():
    assert sorted(CASES) == ["a", "b", "c", "d", "e"]
    shapes = {n: (c["tgt"].shape[0], c["src"].shape[0], c["tgt"].shape[1], c["k"], c["lambda_value"]) for n, c in CASES.items()}
    assert shapes == {"a": (48, 16, 2048, 6, 0.1), "b": (160, 64, 256, 20, 0.3), "c": (33, 1, 7, 2, 0.1), "d": (64, 20, 40, 4, 0.1),
                      "e": (120, 30, 64, 8, 0.2)}
    assert CASES["e"]["MemorySave"] and CASES["e"]["Minibatch"] == 50 and not CASES["a"]["MemorySave"]
    tgt = CASES["d"]["tgt"]                                      # 16 rows present two or three times
    _, counts = np.unique(tgt, axis=0, return_counts=True)
    assert (counts == 2).sum() == 8 and (counts == 3).sum() == 8


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_reference_bit_for_bit(name):
    c = CASES[name]
    r = hausdorff_ref.re_ranking(c["src"], c["tgt"], c["k"], c["lambda_value"], c["MemorySave"])
    assert r["euclidean_dist"].dtype == np.float16 and r["final_dist"].dtype == np.float64
    assert c["euclidean_dist"].dtype == np.float16 and c["final_dist"].dtype == np.float64
    assert np.array_equal(bits(r["euclidean_dist"]), bits(c["euclidean_dist"]))
    assert np.array_equal(r["final_dist"], c["final_dist"])
    f = r["final_dist"]
    assert np.array_equal(f, f.T)
    assert np.array_equal(np.diag(f), 2 * r["vec"] * c["lambda_value"])
    assert not np.isnan(f).any() and np.diag(r["H"]).max() == 0
    if name == "d":
        assert max(len(s) for s in r["sets"]) > c["k"] - 1 and (r["E"][~np.eye(64, dtype=bool)] == 0).any()    # ties widen the sets; zero distances
    if name == "c":
        assert all(len(s) == 1 for s in r["sets"])


def test_python_refusals_need_no_gpu():
    from ssg_amd import rerank_hausdorff as rh
    from ssg_amd.selftraining import compute_dist
    x = np.zeros((10, 8), dtype=np.float32)
    for k in (1, 0, 11):                                         # k < 2, k > N
        with pytest.raises(ValueError, match="2 <= k <= min"):
            rh.re_ranking(x, x, k=k)
        with pytest.raises(ValueError, match="2 <= k <= min"):
            rh.re_ranking_hausdorff_device(x, x, k=k)
    with pytest.raises(ValueError, match="2 <= k <= min"):
        rh.check_limits(1000, 65)                                # k > 64
    rh.check_limits(46340, 20)                                   # 46340^2 < 2^31 <= 46341^2

    class Shape:                                                 # N alone decides: nothing is allocated or copied first
        shape = (46341, 8)
    with pytest.raises(ValueError, match=r"N \* N < 2\^31"):
        rh.re_ranking_hausdorff_device(Shape(), Shape(), k=20)
    with pytest.raises(ValueError, match=r"N \* N < 2\^31"):
        rh.re_ranking(Shape(), Shape(), k=20)
    with pytest.raises(ValueError, match="variant"):
        compute_dist(x, x, 0.1, False, variant="chamfer")
    for v in ("hausdorff", "plain"):
        with pytest.raises(ValueError, match="single GPU"):
            compute_dist(x, x, 0.1, False, group=object(), variant=v)
    import ssg_amd
    assert ssg_amd.re_ranking_hausdorff is rh.re_ranking and ssg_amd.re_ranking_hausdorff_device is rh.re_ranking_hausdorff_device


def test_entry_points_refuse_bad_arguments_without_gpu():
    from ssg_amd import _lib
    L = _lib.lib()
    p = 4096                                                     # a non-null pointer value: refused calls never touch it
    assert L.ssg_seqdist_f64(None, 4, None, 4, 8, 1, None, 4, None) == -1 and b"ssg_seqdist_f64" in L.ssg_last_error()
    for m, n, d, ld in ((0, 4, 8, 4), (4, -1, 8, 4), (4, 4, 0, 4), (4, 4, 8, 3)):
        assert L.ssg_seqdist_f64(p, m, p, n, d, 1, p, ld, None) == -1, (m, n, d, ld)
    assert L.ssg_seqdist_self_f64(None, 4, 8, 1, None, 4, None) == -1
    for n, d, ld in ((0, 8, 4), (4, 0, 4), (4, 8, 3)):
        assert L.ssg_seqdist_self_f64(p, n, d, 1, p, ld, None) == -1, (n, d, ld)
    assert L.ssg_seqdist_rowmin_f64(None, 4, None, 4, 8, None, None) == -1
    for m, n, d in ((0, 4, 8), (4, 0, 8), (4, 4, -2)):
        assert L.ssg_seqdist_rowmin_f64(p, m, p, n, d, p, None) == -1, (m, n, d)
    assert L.ssg_hausdorff_source_finish(None, 4, None, None, None) == -1 and L.ssg_hausdorff_source_finish(p, 0, p, p, None) == -1
    assert L.ssg_hausdorff_workspace_bytes(100, 100) == 100 * 100 * 8 and L.ssg_hausdorff_workspace_bytes(20000, 20000) == 1024 * 20000 * 8
    assert L.ssg_hausdorff_workspace_bytes(0, 4) == 0
    assert L.ssg_hausdorff_directed_rows(None, None, None, 8, 10, 0, 10, None, None, 800, None) == -1
    for N, row0, nrows, cap, wsb in ((0, 0, 1, 8, 800), (10, 0, 0, 8, 800), (10, 4, 7, 8, 800), (10, -1, 4, 8, 800), (10, 0, 10, 0, 800), (10, 0, 10, 8, 799),
                                     (46341, 0, 1, 8, 1 << 30)):
        assert L.ssg_hausdorff_directed_rows(p, p, p, cap, N, row0, nrows, p, p, wsb, None) == -1, (N, row0, nrows, cap, wsb)
    assert b"2^31" in L.ssg_last_error()
    assert L.ssg_hausdorff_symmetrize(None, 10, None, None) == -1 and L.ssg_hausdorff_symmetrize(p, 0, p, None) == -1
    assert L.ssg_hausdorff_symmetrize(p, 46341, p, None) == -1
    assert L.ssg_hausdorff_blend(None, None, None, 10, 0, 10, 0.9, 0.1, None, None) == -1
    for N, row0, nrows in ((0, 0, 1), (10, 0, 0), (10, 8, 3)):
        assert L.ssg_hausdorff_blend(p, p, p, N, row0, nrows, 0.9, 0.1, p, None) == -1, (N, row0, nrows)
    assert L.ssg_half_div_max(None, None, 10, None, None, None) == -1 and L.ssg_half_div_max(p, p, 0, p, p, None) == -1
