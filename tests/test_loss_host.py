"""Host half of the classification-loss tests (no GPU): the names, the argument checks that come before any launch, the rules of the
Python layer, and the float64 restatement (tests/loss_ref.py) against what the reference's own classes gave
(tests/golden/loss_cases.npz, written by tools/make_golden_losses.py).

The golden values are float32 results of a float32 op chain (subtract the maximum, exp, a sum of C terms, log, gather, pow, products,
a mean over B): about a dozen roundings of quantities no larger than A + log C, so against float64

    |golden - ref64| <= 16 * 2^-24 * (|ref64| + (1 + A) max(1, |factor|))

with A and `factor` as in loss_ref's docstring.  OIM has no golden -- the reference's legacy autograd.Function cannot run on a current
torch -- so loss_ref.oim_update / oim_loss are its only yardstick; their properties are checked here."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as ref  # noqa: E402

nn = torch.nn
NAMES = ("CrossEntropyLoss", "FocalLoss", "WeightCE", "OIMLoss", "oim", "accuracy", "cross_entropy_train")


@pytest.fixture(scope="module")
def L():
    from ssg_amd import _lib
    return _lib.lib()


def test_new_names_resolve():
    import ssg_amd
    for n in NAMES:
        assert callable(getattr(ssg_amd, n)), n
    assert issubclass(ssg_amd.CrossEntropyLoss, nn.CrossEntropyLoss)
    assert isinstance(ssg_amd.CrossEntropyLoss(), nn.CrossEntropyLoss)
    assert list(ssg_amd.OIMLoss(64, 5).state_dict()) == ["lut"] and ssg_amd.OIMLoss(64, 5).lut.shape == (5, 64)
    assert list(ssg_amd.CrossEntropyLoss(weight=torch.ones(3)).state_dict()) == ["weight"]


def test_constructors_follow_the_reference():
    import ssg_amd
    assert torch.equal(ssg_amd.FocalLoss(alpha=0.25).alpha, torch.tensor([0.25, 0.75]))
    assert torch.equal(ssg_amd.FocalLoss(alpha=1).alpha, torch.tensor([1.0, 0.0]))
    assert torch.equal(ssg_amd.FocalLoss(alpha=[1.0, 2.0, 3.0]).alpha, torch.tensor([1.0, 2.0, 3.0]))
    f = ssg_amd.FocalLoss()
    assert (f.gamma, f.alpha, f.size_average) == (2.0, None, True)
    with pytest.warns(UserWarning):                              # the legacy arguments are mapped as torch maps them
        assert ssg_amd.CrossEntropyLoss(size_average=False).reduction == "sum"
    with pytest.warns(UserWarning):
        assert ssg_amd.CrossEntropyLoss(reduce=False).reduction == "none"
    c = ssg_amd.CrossEntropyLoss(ignore_index=7, reduction="sum")
    assert (c.ignore_index, c.reduction, c.label_smoothing) == (7, "sum", 0.0)
    o = ssg_amd.OIMLoss(64, 5, scalar=30.0, momentum=0.25)
    assert (o.num_features, o.num_classes, o.scalar, o.momentum, o.weight, o.size_average) == (64, 5, 30.0, 0.25, None, True)
    w = ssg_amd.WeightCE(margin=0.5, num_instances=4, use_semi=False)
    assert (w.margin, w.use_semi) == (0.5, False)


def test_bad_arguments_are_refused_before_any_launch(L):
    cap = L.ssg_softmax_ce_row_capacity()
    assert cap >= 1024 and cap % 4 == 0 and L.ssg_topk_correct_max_k() >= 2
    inf, nan = float("inf"), float("nan")

    def fwd(B=4, C=8, ldx=8, red=1, gamma=0.0):
        return L.ssg_softmax_ce_fwd_f32(None, ldx, None, -100, None, None, gamma, red, B, C, None, None, None, None, None, None)

    def bwd(B=4, C=8, ldx=8, lddx=8, gs=0):
        return L.ssg_softmax_ce_bwd_f32(None, ldx, None, -100, None, None, None, None, gs, None, lddx, B, C, None)

    def topk(B=4, C=8, ldx=8, ks=(1,), nk=None):
        arr = (ctypes.c_int * max(1, len(ks)))(*ks)
        return L.ssg_topk_correct_f32(None, ldx, None, B, C, arr, len(ks) if nk is None else nk, None, None, None)

    def oim(B=4, C=8, F=32, ldx=32, ldl=32, m=0.5):
        return L.ssg_oim_update_f32(None, ldx, None, None, ldl, B, C, F, m, None)

    # NULL pointers, everything else in order
    for call, name in ((fwd, b"ssg_softmax_ce_fwd_f32"), (bwd, b"ssg_softmax_ce_bwd_f32"), (topk, b"ssg_topk_correct_f32"), (oim, b"ssg_oim_update_f32")):
        assert call() == -1 and b"NULL" in L.ssg_last_error() and name in L.ssg_last_error()
    # B < 1, C < 1, a row stride below the row
    for kw in (dict(B=0), dict(B=-3), dict(C=0), dict(C=-1), dict(ldx=7), dict(ldx=-8)):
        for call, name in ((fwd, b"ssg_softmax_ce_fwd_f32"), (bwd, b"ssg_softmax_ce_bwd_f32"), (topk, b"ssg_topk_correct_f32")):
            assert call(**kw) == -1 and name in L.ssg_last_error() and b"NULL" not in L.ssg_last_error(), kw
        assert b"ldx" in L.ssg_last_error()
    assert bwd(lddx=7) == -1 and b"lddx" in L.ssg_last_error()
    for kw in (dict(B=0), dict(C=0), dict(F=0), dict(ldx=31), dict(ldl=31), dict(F=-32)):
        assert oim(**kw) == -1 and b"ssg_oim_update_f32" in L.ssg_last_error() and b"NULL" not in L.ssg_last_error(), kw
    # the codes and the scalars
    for red in (-1, 4, 99):
        assert fwd(red=red) == -1 and b"reduction" in L.ssg_last_error()
    for gamma in (-0.5, inf, -inf, nan):
        assert fwd(gamma=gamma) == -1 and b"gamma" in L.ssg_last_error()
    for m in (-0.1, inf, nan):
        assert oim(m=m) == -1 and b"momentum" in L.ssg_last_error()
    for gs in (-1, 2):
        assert bwd(gs=gs) == -1 and b"g_stride" in L.ssg_last_error()
    assert bwd(B=1 << 30, C=1 << 20, ldx=1 << 20, lddx=1 << 20) == -1 and b"grid" in L.ssg_last_error()
    assert topk(ks=()) == -1 and topk(ks=(1,) * 9) == -1 and b"num_k" in L.ssg_last_error()
    assert topk(ks=(1,), nk=-1) == -1


def test_unsupported_arguments_raise_valueerror_naming_the_rule():
    import ssg_amd
    x, t = torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64)
    for kw, word in [(dict(input=x.double()), "float32"), (dict(target=t.int()), "int64"), (dict(input=torch.zeros(4, 8, 2)), r"\[B, C\]"),
                     (dict(target=torch.zeros(4, 1, dtype=torch.int64)), r"\[B\]"), (dict(target=torch.zeros(5, dtype=torch.int64)), "rows"),
                     (dict(input=torch.zeros(0, 8), target=t[:0]), "empty"), (dict(reduction="avg"), "reduction"), (dict(gamma=-1.0), "gamma"),
                     (dict(gamma=float("nan")), "gamma"), (dict(weight=torch.ones(7)), "8 entries"), (dict(row_weight=torch.ones(8)), "4 entries"),
                     (dict(weight=torch.ones(8).double()), "float32"), (dict(weight=torch.ones(8, requires_grad=True)), "requires grad"),
                     (dict(row_weight=torch.ones(4, requires_grad=True)), "requires grad")]:
        args = dict(input=x, target=t)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            ssg_amd.cross_entropy_train(**args)
    with pytest.raises(ValueError, match="label_smoothing"):
        ssg_amd.CrossEntropyLoss(label_smoothing=0.1)
    with pytest.raises(ValueError, match="probabilities"):
        ssg_amd.CrossEntropyLoss()(x, torch.zeros(4, 8))
    for alpha in (0.25, [1.0] * 7, [1.0] * 9):                    # C = 8: the table must have exactly 8 entries
        with pytest.raises(ValueError, match="exactly C = 8"):
            ssg_amd.FocalLoss(alpha=alpha)(x, t, 0)
    with pytest.raises(ValueError, match="w"):
        ssg_amd.WeightCE()(x, t, torch.ones(5))
    xf = torch.zeros(4, 48)
    with pytest.raises(ValueError, match="F % 32"):
        ssg_amd.oim(xf, t, torch.zeros(6, 48))
    with pytest.raises(ValueError, match="F % 32"):
        ssg_amd.OIMLoss(48, 6)(xf, t)
    xf = torch.zeros(4, 64)
    for args, word in [((xf, t, torch.zeros(6, 32)), "features"), ((xf.double(), t, torch.zeros(6, 64)), "float32"), ((xf, t[:3], torch.zeros(6, 64)), "targets"),
                       ((xf, t, torch.zeros(64, 6).t()), "contiguous"), ((xf, t, torch.zeros(6, 64), -0.5), "momentum"),
                       ((xf, t, torch.zeros(6, 64, requires_grad=True)), "in place")]:
        with pytest.raises(ValueError, match=word):
            ssg_amd.oim(*args)
    for args, word in [((x.double(), t), "float32"), ((x, t.int()), "int64"), ((x, t, ()), "topk"), ((x, t, (0,)), "topk"), ((x[0], t), r"\[B, C\]")]:
        with pytest.raises(ValueError, match=word):
            ssg_amd.accuracy(*args)


def test_forward_without_a_gpu_raises_ssgerror():
    import ssg_amd
    if not torch.cuda.is_available():                            # there is no CPU fallback
        x, t = torch.zeros(4, 64), torch.zeros(4, dtype=torch.int64)
        for call in (lambda: ssg_amd.CrossEntropyLoss()(x, t), lambda: ssg_amd.FocalLoss()(x, t, 0), lambda: ssg_amd.WeightCE()(x, t, torch.ones(4)),
                     lambda: ssg_amd.OIMLoss(64, 5)(x, t), lambda: ssg_amd.accuracy(x, t)):
            with pytest.raises(ssg_amd.SSGError):
                call()


# ---- the restatement against the reference's own results ---------------------------------------------------------------------------------

def _f32_ok(got32, ref64, A, factor):
    lim = 16 * 2.0 ** -24 * (np.abs(ref64) + (1.0 + A) * np.maximum(1.0, np.abs(factor)))
    err = np.abs(np.asarray(got32, dtype=np.float64) - ref64)
    print("max err %.3g, worst err / bound %.3g" % (float(err.max()), float((err / lim).max())))
    return bool((err <= lim).all())


def test_loss_ref_against_the_golden_file(golden):
    g = golden("loss_cases.npz")
    kinds = {"g2_mean": (2.0, False, True), "g05_alpha_sum": (0.5, True, False), "g0_mean": (0.0, False, True), "g2_binary": (2.0, "binary", True)}
    assert sorted(kinds) == sorted(str(n) for n in g["focal"])
    seen = 0
    for si, (B, C, _) in enumerate(g["shapes"]):
        x, t, w, alpha = g["x_%d" % si], g["t_%d" % si], g["w_%d" % si], g["alpha_%d" % si]
        assert x.shape == (B, C) and x.dtype == np.float32
        assert C == 1 or float(np.diff(np.sort(x.astype(np.float64), axis=1), axis=1).min()) >= 1e-3          # tie-free
        for name, (gamma, akind, size_average) in kinds.items():
            if "focal_%s_loss_%d" % (name, si) not in g.files:
                assert akind == "binary" and C != 2
                continue
            a = None if akind is False else np.array([0.25, 0.75], dtype=np.float32) if akind == "binary" else alpha
            r = ref.focal_loss(x, t, gamma=gamma, alpha=a, size_average=size_average)
            assert _f32_ok(g["focal_%s_loss_%d" % (name, si)], r["loss"], r["A"], r["r"] * np.abs(r["s"]).sum()), (name, si)
            assert _f32_ok(g["focal_%s_grad_%d" % (name, si)], r["dx"], r["A"], r["coef"][:, None]), (name, si)
            seen += 1
        r = ref.weight_ce(x, t, w)
        assert _f32_ok(g["wce_loss_%d" % si], r["loss"], r["A"], r["r"] * np.abs(r["s"]).sum())
        assert _f32_ok(g["wce_grad_%d" % si], r["dx"], r["A"], r["coef"][:, None])
        # accuracy: bit for bit
        acc = ref.accuracy(x, t, topk=tuple(int(k) for k in g["topk"]))
        assert np.array_equal(np.concatenate(acc).view(np.uint32), g["acc_%d" % si].view(np.uint32))
    assert seen == 3 * len(g["shapes"]) + 1


def test_loss_ref_agrees_with_torch_cross_entropy_in_float64():
    """the weighted mean is torch's rule, sum w_t ce / sum w_t over the rows that are not ignored; the gradient is autograd's"""
    F = torch.nn.functional
    rng = np.random.default_rng(3)
    x = (3 * rng.standard_normal((7, 11))).astype(np.float32)
    t = rng.integers(0, 11, 7)
    t[2] = -100
    w = rng.uniform(0.5, 2, 11).astype(np.float32)
    for weight in (None, w):
        for reduction in ("mean", "sum", "none"):
            xr = torch.from_numpy(x).double().requires_grad_(True)
            loss = F.cross_entropy(xr, torch.from_numpy(t), weight=None if weight is None else torch.from_numpy(weight).double(), reduction=reduction)
            gy = torch.from_numpy(rng.standard_normal(7)).float().double() if reduction == "none" else torch.tensor(1.25, dtype=torch.float64)
            loss.backward(gy)
            r = ref.cross_entropy_loss(x, t, weight=weight, reduction=reduction)
            mine = ref.cross_entropy(x, t, class_w=weight, reduction=reduction, g=gy.numpy())
            want = r["row_loss"] if reduction == "none" else r["loss"]
            assert np.allclose(want, loss.detach().numpy(), rtol=1e-13, atol=1e-13)
            assert np.allclose(mine["dx"], xr.grad.numpy(), rtol=1e-12, atol=1e-14)
    assert np.isnan(ref.cross_entropy_loss(x, np.full(7, -100))["loss"])                   # all rows ignored: NaN, as torch gives
    assert np.isnan(float(F.cross_entropy(torch.from_numpy(x), torch.full((7,), -100))))


def test_loss_ref_conventions():
    c = ref.value_cases()
    r = ref.cross_entropy(**c["target_eq_C"])
    assert np.isnan(r["loss"]) and np.isnan(r["dx"][3]).all() and np.isfinite(np.delete(r["dx"], 3, axis=0)).all() and np.isfinite(r["r"])
    r = ref.cross_entropy(**c["some_ignored"])
    assert (r["dx"][[1, 4]] == 0).all() and r["s"][1] == 0 and np.isfinite(r["loss"])
    r = ref.cross_entropy(**c["neg_inf_target"])
    assert r["row_loss"][2] == np.inf and np.isfinite(r["dx"]).all()
    r = ref.cross_entropy(**c["pt_near_1_lead80_g0.5"])
    assert (r["s"] == 0).all() and r["loss"] == 0                 # pt is exactly 1: (1 - pt)^0.5 = 0
    assert (ref.cross_entropy(**c["pt_near_1_lead80_g0"])["s"] == 1).all()                 # pow(0, 0) = 1
    # ranks: ties go to the lower index
    x = np.array([[2, 2, 2, 2], [1, 3, 3, 0]], dtype=np.float32)
    assert list(ref.ranks(x, [2, 2])) == [2, 1] and list(ref.ranks(x, [0, 1])) == [0, 0] and list(ref.ranks(x, [4, -1])) == [4, 4]
    assert [float(a[0]) for a in ref.accuracy(x, [2, 2], topk=(1, 2, 3))] == [0.0, 0.5, 1.0]
    assert ref.accuracy(np.zeros((3, 9), dtype=np.float32), [0] * 3, topk=(1,))[0][0] == np.float32(3) * np.float32(1.0 / 3)
    # the OIM update: batch order, float32 storage after every sample, unit rows, untouched rows unchanged
    rng = np.random.default_rng(2)
    lut = rng.standard_normal((5, 32)).astype(np.float32)
    xs = rng.standard_normal((3, 32)).astype(np.float32)
    new = ref.oim_update(lut, xs, [1, 3, 1], 0.5)
    assert np.array_equal(new[[0, 2, 4]], lut[[0, 2, 4]])
    assert np.array_equal(new[1], ref.oim_update(ref.oim_update(lut, xs[:1], [1], 0.5), xs[2:], [1], 0.5)[1])
    assert np.allclose(np.linalg.norm(new[[1, 3]].astype(np.float64), axis=1), 1, atol=1e-6)
    assert np.isnan(ref.oim_update(np.zeros((2, 32)), np.zeros((1, 32)), [0], 0.5)[0]).all()   # a zero norm gives NaN
