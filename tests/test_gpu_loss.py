"""GPU suite of the classification losses (csrc/softmax_ce.hip, ssg_amd/loss.py) against the float64 restatement of tests/loss_ref.py.

Bound, derived and not measured (loss_ref's docstring): every output is a float64 value rounded once, so

    |got - ref64| <= 2^-23 |ref64| + 1e-12 (1 + A) max(1, |factor|)

with A the largest finite |logit| of the case and `factor` = g_i r s_i for dx, s_i for a row loss, r sum |s_i| for the batch loss.  Where
ref64 is NaN or infinite the device must give the same.  The worst ratios measured on the MI355X are in profiles/loss_errors.txt
(tools/loss_errors.py, from `measure()` below); a ratio above 1 is a bug, not a reason to widen the bound.

OIM: the reference's legacy autograd.Function cannot run on a current torch, so loss_ref's restatement is its only yardstick.  Logits and
grad_inputs meet the (L + 2) 2^-24 A bound of tests/test_gpu_head.py's Linear; the table rows after the update are within
2^-22 / (1 - m) absolute (unit-norm rows: one rounding per step plus an inherited last-bit flip damped by m per later step).

Composition: classifier_x2 as ssg_amd.Linear(2048, 751) under ssg_amd.CrossEntropyLoss, weight and bias gradients against float64
autograd.  With e_y <= (K + 3) 2^-24 A_y the bound of the device logits and d_b = max_n e_y[b][n], softmax moves by at most
p (e^(2 d_b) - 1), so |dy_dev - dy64| <= e_dy = bound_ce + |coef_b| p (e^(2 d_b) - 1), and

    |dW_dev - dW64| <= (B + 2) 2^-24 (|dy64| + e_dy)^T |x| + e_dy^T |x|,   |db_dev - db64| <= 2^-24 sum_b (|dy64| + e_dy) + sum_b e_dy.

No test provokes a fault: a target out of range is compared, never used as an index (csrc/softmax_ce.hip tests `t < 0 || t >= C` before
every `[t]`)."""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as ref  # noqa: E402
from train_common import U, _lib, _nan, bound as lin_bound  # noqa: E402

pytestmark = pytest.mark.gpu


def cap():
    return _lib().ssg_softmax_ce_row_capacity()


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def shifted(t):
    """a device copy of t one element into its storage: 4-byte aligned and no more"""
    v = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def run_api(case, place=lambda t: t):
    """one forward + backward through ssg_amd.cross_entropy_train -> dict(loss, dx) of numpy arrays"""
    import ssg_amd
    x = place(cuda(case["x"])).requires_grad_(True)
    loss = ssg_amd.cross_entropy_train(x, cuda(case["target"]), weight=cuda(case["class_w"]), row_weight=cuda(case["row_w"]), gamma=case["gamma"],
                                       reduction=case["reduction"], ignore_index=case["ignore_index"])
    assert loss.dtype == torch.float32 and loss.shape == ((x.shape[0],) if case["reduction"] == "none" else ())
    g = case["g"]
    (dx,) = torch.autograd.grad(loss, x, cuda(np.asarray(g, dtype=np.float32)) if np.ndim(g) else torch.tensor(float(g), dtype=torch.float32, device="cuda"))
    assert dx.shape == x.shape and dx.dtype == torch.float32
    return dict(loss=loss.detach().cpu().numpy(), dx=dx.cpu().numpy())


def run_abi(case, ldx=None, lddx=None, shift=False):
    """the raw entry points on a [B, ldx] buffer (one element into its storage when `shift`); every output starts as NaN with a guard
    behind it, and the gaps of dx between the rows (lddx > C) must stay NaN"""
    from ssg_amd._lib import check, ptr, stream
    from ssg_amd.loss import REDUCTIONS
    L = _lib()
    B, C = case["x"].shape
    ldx, lddx = ldx or C, lddx or C
    xb = torch.zeros(B * ldx + 1, dtype=torch.float32, device="cuda")[1 if shift else 0:][:B * ldx].view(B, ldx)
    xb[:, :C] = cuda(case["x"])
    dxb = _nan(B * lddx + 65)[1 if shift else 0:][:B * lddx + 64]
    t, cw, rw = cuda(case["target"]), cuda(case["class_w"]), cuda(case["row_w"])
    code = REDUCTIONS[case["reduction"]]
    lse, s, r, row_loss, loss = (torch.full((n,), float("nan"), dtype=d, device="cuda") for n, d in
                                 ((B + 8, torch.float64), (B + 8, torch.float64), (9, torch.float64), (B + 8, torch.float32), (9, torch.float32)))
    g = cuda(np.atleast_1d(np.asarray(case["g"], dtype=np.float32)))
    check(L.ssg_softmax_ce_fwd_f32(ptr(xb), ldx, ptr(t), case["ignore_index"], ptr(rw), ptr(cw), float(case["gamma"]), code, B, C, ptr(lse), ptr(s), ptr(r),
                                   ptr(row_loss), ptr(loss) if code else None, stream()), "ssg_softmax_ce_fwd_f32")
    check(L.ssg_softmax_ce_bwd_f32(ptr(xb), ldx, ptr(t), case["ignore_index"], ptr(lse), ptr(s), ptr(r), ptr(g), 1 if code == 0 else 0, ptr(dxb), lddx, B, C,
                                   stream()), "ssg_softmax_ce_bwd_f32")
    torch.cuda.synchronize()
    for name, buf, n in (("lse", lse, B), ("s", s, B), ("r", r, 1), ("row_loss", row_loss, B), ("loss", loss, 1 if code else 0)):
        assert bool(torch.isnan(buf[n:]).all()), "%s: written past its end" % name
    assert bool(torch.isnan(dxb[B * lddx:]).all()), "dx: written past its end"
    rows = dxb[:B * lddx].view(B, lddx)
    assert bool(torch.isnan(rows[:, C:]).all()), "dx: written between the rows"
    return dict(loss=(loss[0] if code else row_loss[:B]).cpu().numpy(), row_loss=row_loss[:B].cpu().numpy(), dx=rows[:, :C].cpu().numpy(),
                lse=lse[:B].cpu().numpy(), s=s[:B].cpu().numpy(), r=float(r[0]))


def check_case(name, case, got, want=None):
    want = want or ref.cross_entropy(**case)
    for o, q in ref.ratios(got, want).items():
        print("%s %s %s: worst err / bound = %.3g" % (name, case["x"].shape, o, q))
        assert q <= 1.0, "%s: %s misses its bound by a factor of %.3g" % (name, o, q)
    return want


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)) for k in ("loss", "dx"))


def class_counts():
    return (1, 2, 63, 64, 65, 751, cap(), cap() + 1)


# ---- shapes --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ci", range(8))
def test_shapes_against_float64(ci):
    """B in {1, 3, 128, 257} at every C, on both sides of the staging capacity, in all four modes; the same call twice gives the same bits"""
    C = class_counts()[ci]
    for B in ref.SHAPE_B:
        for mode in ref.MODES:
            case = ref.shape_case(B, C, mode)
            got = run_api(case)
            check_case(mode[0], case, got)
            if B in (3, 257):
                assert same_bits(got, run_api(case)), (B, C, mode[0])


@pytest.mark.parametrize("C", [2, 65, 751, "cap+1"])
def test_layouts_give_the_same_bits(C):
    """a column slice (ldx > C, also an odd stride, so that the rows take the float4 and the single-element path in turn), dx with gaps
    between its rows, and a base that is 4-byte aligned and no more: the bits of the dense, aligned call"""
    C = cap() + 1 if C == "cap+1" else C
    for mode in (ref.MODES[1], ref.MODES[3]):
        case = ref.shape_case(3, C, mode, seed=1)
        dense = run_abi(case)
        want = check_case("dense", case, dense)
        assert np.array_equal(dense["lse"], want["lse"]) or ref.ratio(dense["lse"], want["lse"], 1e-12 * (1 + want["A"])) <= 1.0
        assert ref.ratio(dense["s"], want["s"], 1e-12 * (1 + want["A"]) * np.maximum(1, np.abs(want["s"]))) <= 1.0
        assert ref.ratio(dense["row_loss"], want["row_loss"], ref.bound(want["row_loss"], want["A"], want["s"])) <= 1.0
        assert abs(dense["r"] - want["r"]) <= 1e-15 * abs(want["r"])
        api = run_api(case)
        assert same_bits(api, dense)                             # the autograd function adds nothing of its own
        for kw in (dict(ldx=C + 4, lddx=C + 8), dict(ldx=C + 3, lddx=C + 1), dict(shift=True), dict(ldx=C + 5, lddx=C + 2, shift=True)):
            other = run_abi(case, **kw)
            assert same_bits(other, dense) and np.array_equal(other["lse"], dense["lse"]) and np.array_equal(other["s"], dense["s"]), kw
        assert same_bits(run_api(case, place=shifted), dense)
        wide = torch.zeros(3, C + 7, device="cuda")
        assert same_bits(run_api(case, place=lambda t: wide[:, 2:2 + C].copy_(t).detach()), dense)      # a column slice through the Python layer


# ---- values --------------------------------------------------------------------------------------------------------------------------------

VALUE_CASES = ref.value_cases()


@pytest.mark.parametrize("name", tuple(VALUE_CASES))
def test_special_values(name):
    case = VALUE_CASES[name]
    want = check_case(name, case, run_api(case))
    check_case(name, case, run_abi(case, ldx=case["x"].shape[1] + 3, shift=True), want)
    if name.startswith("target_"):                               # one target out of range: NaN there, every other row finite and in bound
        got = run_api(case)
        assert np.isnan(got["dx"][3]).all() and np.isfinite(np.delete(got["dx"], 3, axis=0)).all()
        assert np.isnan(got["loss"][3] if case["reduction"] == "none" else got["loss"])
    if name.startswith("all_ignored"):
        got = run_api(case)
        assert (got["dx"] == 0).all() and (np.isnan(got["loss"]) if case["reduction"] == "mean" else got["loss"] == 0)


def test_special_values_on_the_second_route():
    """the special values again on rows longer than the staging capacity"""
    cases = ref.value_cases(C=cap() + 1)
    for name in ("pm1e4_g2", "neg_inf_elsewhere_focal", "neg_inf_target", "some_ignored", "target_eq_C", "pt_near_1_lead16_g0.5"):
        check_case(name, cases[name], run_api(cases[name]))


# ---- the modules ---------------------------------------------------------------------------------------------------------------------------

def test_modules_on_the_golden_inputs(golden):
    """FocalLoss, WeightCE and CrossEntropyLoss as the drivers call them, on the inputs of the reference's own run"""
    import ssg_amd
    g = golden("loss_cases.npz")
    for si, (B, C, _) in enumerate(g["shapes"]):
        x, t, w, alpha = g["x_%d" % si], g["t_%d" % si], g["w_%d" % si], g["alpha_%d" % si]
        runs = [(ssg_amd.FocalLoss(), lambda m, xd: m(xd, cuda(t), 3), ref.focal_loss(x, t)),
                (ssg_amd.FocalLoss(gamma=0.5, alpha=[float(v) for v in alpha], size_average=False), lambda m, xd: m(xd, cuda(t), 0),
                 ref.focal_loss(x, t, gamma=0.5, alpha=alpha, size_average=False)),
                (ssg_amd.WeightCE(), lambda m, xd: m(xd, cuda(t), cuda(w)), ref.weight_ce(x, t, w)),
                (ssg_amd.CrossEntropyLoss(weight=torch.from_numpy(alpha)).cuda(), lambda m, xd: m(xd, cuda(t)), ref.cross_entropy_loss(x, t, weight=alpha)),
                (ssg_amd.CrossEntropyLoss(reduction="sum"), lambda m, xd: m(xd, cuda(t)), ref.cross_entropy_loss(x, t, reduction="sum")),
                (ssg_amd.CrossEntropyLoss(reduction="none"), lambda m, xd: m(xd, cuda(t)).sum(), ref.cross_entropy_loss(x, t, reduction="none"))]
        if C == 2:
            runs.append((ssg_amd.FocalLoss(alpha=0.25), lambda m, xd: m(xd, cuda(t), 0), ref.focal_loss(x, t, alpha=np.array([0.25, 0.75], dtype=np.float32))))
        for k, (module, call, want) in enumerate(runs):
            xd = cuda(x).requires_grad_(True)
            loss = call(module, xd)
            loss.backward()
            got = dict(loss=loss.detach().cpu().numpy(), dx=xd.grad.cpu().numpy())
            if want["loss"] is None:                             # 'none' summed by torch: only the gradient is compared
                want = dict(want, loss=float(want["row_loss"].sum()))
                assert abs(float(got["loss"]) - want["loss"]) <= 2.0 ** -20 * abs(want["loss"])
                got["loss"] = np.float32(want["loss"])
            for o, q in ref.ratios(got, want).items():
                assert q <= 1.0, (si, k, o, q)
    # the 4-D branch of FocalLoss: N,C,H,W -> N*H*W,C on the host side, as the reference lays it out
    x4 = np.random.default_rng(0).standard_normal((2, 5, 3, 2)).astype(np.float32)
    t4 = np.random.default_rng(1).integers(0, 5, (2, 3, 2))
    xd = cuda(x4).requires_grad_(True)
    loss = ssg_amd.FocalLoss()(xd, cuda(t4), 0)
    loss.backward()
    want = ref.focal_loss(x4.reshape(2, 5, 6).transpose(0, 2, 1).reshape(-1, 5), t4.reshape(-1))
    got = dict(loss=loss.detach().cpu().numpy(), dx=xd.grad.cpu().numpy().reshape(2, 5, 6).transpose(0, 2, 1).reshape(-1, 5))
    assert max(ref.ratios(got, want).values()) <= 1.0


def test_frozen_input_and_double_backward():
    import ssg_amd
    case = ref.shape_case(3, 65, ref.MODES[0])
    x = cuda(case["x"])
    loss = ssg_amd.cross_entropy_train(x, cuda(case["target"]))
    assert not loss.requires_grad and np.array_equal(loss.cpu().numpy(), run_api(dict(case, g=np.float32(1)))["loss"])
    with pytest.raises(RuntimeError):
        xr = x.clone().requires_grad_(True)
        (gx,) = torch.autograd.grad(ssg_amd.cross_entropy_train(xr, cuda(case["target"])), xr, create_graph=True)
        gx.sum().backward()


# ---- accuracy ------------------------------------------------------------------------------------------------------------------------------

def test_accuracy_counts_and_values(golden):
    import ssg_amd
    from ssg_amd._lib import check, ptr, stream
    g = golden("loss_cases.npz")
    cases = [(g["x_%d" % si], g["t_%d" % si]) for si in range(len(g["shapes"]))]
    rng = np.random.default_rng(9)
    for B, C in ((1, 1), (3, 2), (7, 65), (257, 751), (3, cap() + 1)):          # tie-free: a random order over a grid of values
        x = np.empty((B, C), dtype=np.float32)
        np.put_along_axis(x, np.argsort(rng.standard_normal((B, C)), axis=1), np.broadcast_to(np.arange(C, dtype=np.float32) * 0.25, (B, C)), axis=1)
        t = rng.integers(0, C, B)
        t[::2] = x.argmax(axis=1)[::2]
        cases.append((x, t))
    for x, t in cases:
        B, C = x.shape
        topk = tuple(k for k in (1, 2, 5, 10, C) if k <= C)
        want = ref.accuracy(x, t, topk)
        for place in (lambda v: v, shifted):
            got = ssg_amd.accuracy(place(cuda(x)), cuda(t), topk)
            assert isinstance(got, list) and len(got) == len(topk)
            for a, b in zip(got, want):
                assert a.shape == (1,) and a.dtype == torch.float32 and a.is_cuda
                assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32)), (B, C, topk)
        rank = torch.full((B + 8,), -7, dtype=torch.int32, device="cuda")                          # the counts themselves, through the entry point
        out = _nan(len(topk) + 8)
        xs = shifted(torch.zeros(B, C + 3))
        xs[:, :C] = cuda(x)
        import ctypes
        td = cuda(t)
        check(_lib().ssg_topk_correct_f32(ptr(xs), C + 3, ptr(td), B, C, (ctypes.c_int * len(topk))(*topk), len(topk), ptr(rank), ptr(out), stream()),
              "ssg_topk_correct_f32")
        assert np.array_equal(rank[:B].cpu().numpy(), ref.ranks(x, t)) and bool((rank[B:] == -7).all()) and bool(torch.isnan(out[len(topk):]).all())
    assert len(ssg_amd.accuracy(cuda(cases[-2][0]), cuda(cases[-2][1]), tuple(range(1, 12)))) == 11        # more values of k than one call takes


def test_accuracy_ties_go_to_the_lower_index():
    import ssg_amd
    x = np.array([[2, 2, 2, 2], [1, 3, 3, 0], [5, 5, 1, 1], [0, 0, 0, 9]], dtype=np.float32)
    for t, want in (([2, 2, 1, 0], [0.0, 0.75, 1.0, 1.0]), ([0, 1, 0, 3], [1.0, 1.0, 1.0, 1.0]), ([3, 2, 3, 2], [0.0, 0.25, 0.25, 1.0]),
                    ([4, -1, 0, 3], [0.5, 0.5, 0.5, 0.5])):                                          # a target out of range is never correct
        got = [float(a) for a in ssg_amd.accuracy(cuda(x), cuda(np.array(t)), (1, 2, 3, 4))]
        assert got == want == [float(a[0]) for a in ref.accuracy(x, t, (1, 2, 3, 4))], (t, got)


# ---- OIM -----------------------------------------------------------------------------------------------------------------------------------

OIM_TARGETS = {"unique": [0, 3, 5, 1, 6, 2], "duplicates": [4, 1, 4, 0, 1, 6], "thrice": [2, 5, 2, 2, 0, 5]}
OIM_C = 7


@lru_cache(maxsize=None)
def _oim_data(F):
    rng = np.random.default_rng(40 + F)
    lut = rng.standard_normal((OIM_C, F))
    lut = (lut / np.linalg.norm(lut, axis=1, keepdims=True)).astype(np.float32)
    return lut, rng.standard_normal((6, F)).astype(np.float32), rng.standard_normal((6, OIM_C)).astype(np.float32)


@pytest.mark.parametrize("F", [32, 2048])
@pytest.mark.parametrize("pattern", tuple(OIM_TARGETS))
def test_oim_logits_gradient_and_table(pattern, F):
    import ssg_amd
    lut0, x, gy = _oim_data(F)
    t = np.array(OIM_TARGETS[pattern])
    touched = sorted(set(t.tolist()))
    for m in (0.0, 0.5, 0.9):
        want = ref.oim_loss(x, t, lut0, momentum=m, g_logits=gy)
        lut = cuda(lut0)
        xd = cuda(x).requires_grad_(True)
        y = ssg_amd.oim(xd, cuda(t), lut, momentum=m)
        assert torch.equal(lut, cuda(lut0))                      # no backward yet: the table is not touched
        err = np.abs(y.detach().cpu().numpy().astype(np.float64) - want["raw"])
        assert (err <= lin_bound(F, want["A_raw"])).all()
        (dx,) = torch.autograd.grad(y, xd, cuda(gy))
        err = np.abs(dx.cpu().numpy().astype(np.float64) - want["dx_inputs"])        # against the table from before the update
        assert (err <= lin_bound(OIM_C, want["A_dx_inputs"])).all()
        new = lut.cpu().numpy()
        rest = [c for c in range(OIM_C) if c not in touched]
        assert np.array_equal(new[rest].view(np.uint32), lut0[rest].view(np.uint32))             # untouched rows: the same bits
        err = np.abs(new[touched].astype(np.float64) - want["lut"][touched].astype(np.float64)).max()
        print("%s F=%d m=%g: max |table - ref| = %.3g (bound %.3g), bit-equal: %s" % (pattern, F, m, err, 2.0 ** -22 / (1 - m), np.array_equal(new, want["lut"])))
        assert err <= 2.0 ** -22 / (1 - m)
        assert not np.array_equal(new[touched], lut0[touched])
        # the same forward + backward from the same table: the same bits
        lut2, xd2 = cuda(lut0), cuda(x).requires_grad_(True)
        (dx2,) = torch.autograd.grad(ssg_amd.oim(xd2, cuda(t), lut2, momentum=m), xd2, cuda(gy))
        assert torch.equal(dx2, dx) and torch.equal(lut2, lut)


def test_oim_update_runs_without_an_input_gradient_and_skips_bad_targets():
    import ssg_amd
    from ssg_amd._lib import check, ptr, stream
    lut0, x, gy = _oim_data(32)
    t = np.array(OIM_TARGETS["duplicates"])
    lut = cuda(lut0)
    y = ssg_amd.oim(cuda(x), cuda(t), lut, momentum=0.5)          # the input needs no gradient
    assert y.requires_grad and torch.equal(lut, cuda(lut0))
    y.backward(cuda(gy))
    assert np.abs(lut.cpu().numpy().astype(np.float64) - ref.oim_update(lut0, x, t, 0.5)).max() <= 2.0 ** -22 / 0.5
    with torch.no_grad():                                        # no graph, no backward, no update
        lut = cuda(lut0)
        assert not ssg_amd.oim(cuda(x), cuda(t), lut).requires_grad and torch.equal(lut, cuda(lut0))
    # the entry point on a table with a row stride and a guard; targets out of range update nothing
    t = np.array([4, OIM_C, 4, -1, 1, 1 << 40])
    buf = _nan(OIM_C * 40 + 64)
    table = buf[:OIM_C * 40].view(OIM_C, 40)
    table[:, :32] = cuda(lut0)
    xd, td = cuda(x), cuda(t)                                    # held until the kernel has run
    check(_lib().ssg_oim_update_f32(ptr(xd), 32, ptr(td), ptr(table), 40, 6, OIM_C, 32, 0.9, stream()), "ssg_oim_update_f32")
    torch.cuda.synchronize()
    assert bool(torch.isnan(table[:, 32:]).all()) and bool(torch.isnan(buf[OIM_C * 40:]).all())
    want = ref.oim_update(lut0, x, t, 0.9)
    got = table[:, :32].cpu().numpy()
    assert np.array_equal(got[[0, 2, 3, 5, 6]], lut0[[0, 2, 3, 5, 6]]) and np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -22 / 0.1
    # a zero norm gives NaN, as in the reference
    z, x0, t1 = torch.zeros(2, 32, device="cuda"), torch.zeros(1, 32, device="cuda"), cuda(np.array([1]))
    check(_lib().ssg_oim_update_f32(ptr(x0), 32, ptr(t1), ptr(z), 32, 1, 2, 32, 0.5, stream()), "ssg_oim_update_f32")
    torch.cuda.synchronize()
    assert bool(torch.isnan(z[1]).all()) and bool((z[0] == 0).all())


def test_oim_loss_module():
    """OIMLoss.forward -> (loss, scalar * logits); the loss is the device cross-entropy of those logits, they are differentiable, and a
    backward updates the buffer"""
    import ssg_amd
    lut0, x, _ = _oim_data(2048)
    t = np.array(OIM_TARGETS["thrice"])
    cw = np.linspace(0.5, 2.0, OIM_C).astype(np.float32)
    for size_average, weight in ((True, None), (False, None), (True, cw)):
        m = ssg_amd.OIMLoss(2048, OIM_C, scalar=10.0, momentum=0.5, weight=cuda(weight), size_average=size_average).cuda()
        assert torch.equal(m.lut, torch.zeros_like(m.lut))
        m.lut.copy_(cuda(lut0))
        xd = cuda(x).requires_grad_(True)
        loss, logits = m(xd, cuda(t))
        assert logits.requires_grad and logits.shape == (6, OIM_C)
        want = ref.cross_entropy_loss(logits.detach().cpu().numpy(), t, weight=weight, reduction="mean" if size_average else "sum")
        loss.backward()
        g_logits = want["dx"].astype(np.float32).astype(np.float64) * 10.0
        full = ref.oim_loss(x, t, lut0, momentum=0.5, g_logits=g_logits)
        assert ref.ratio(loss.detach().cpu().numpy(), want["loss"], ref.bound(want["loss"], want["A"], want["r"] * np.abs(want["s"]).sum())) <= 1.0
        err = np.abs(xd.grad.cpu().numpy().astype(np.float64) - full["dx_inputs"])
        assert (err <= lin_bound(OIM_C, full["A_dx_inputs"]) + 10.0 * np.abs(lut0).sum(axis=0) * 2.0 ** -22 * np.abs(want["dx"]).max()).all()
        assert np.abs(m.lut.cpu().numpy().astype(np.float64) - full["lut"]).max() <= 2.0 ** -22 / 0.5
        assert list(m.state_dict()) == ["lut"]


# ---- reproducibility and composition -----------------------------------------------------------------------------------------------------

def test_the_same_step_twice_gives_the_same_bits():
    for C in (751, cap() + 1):
        for mode in ref.MODES:
            case = ref.shape_case(128, C, mode, seed=2)
            a, b = run_api(case), run_api(case)
            assert same_bits(a, b), (C, mode[0])


def test_classifier_under_cross_entropy_against_float64():
    """classifier_x2 = ssg_amd.Linear(2048, 751) under ssg_amd.CrossEntropyLoss at B = 128: weight and bias gradients within the
    composed bound of the module's docstring, and bit-equal run to run"""
    import ssg_amd
    B, K, N = 128, 2048, 751
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, K, generator=gen)
    w = torch.randn(N, K, generator=gen) * K ** -0.5
    b = torch.randn(N, generator=gen) * 0.1
    t = torch.randint(0, N, (B,), generator=gen)
    x64, w64, b64 = x.double(), w.double().requires_grad_(True), b.double().requires_grad_(True)
    y64 = torch.nn.functional.linear(x64, w64, b64)
    y64.retain_grad()
    torch.nn.functional.cross_entropy(y64, t).backward()
    dy64 = y64.grad.abs()

    def device():
        lin = ssg_amd.Linear(K, N).cuda()
        with torch.no_grad():
            lin.weight.copy_(w)
            lin.bias.copy_(b)
        ssg_amd.CrossEntropyLoss()(lin(x.cuda()), t.cuda()).backward()
        return lin.weight.grad.cpu(), lin.bias.grad.cpu()

    dw, db = device()
    A_y = x64.abs() @ w64.detach().abs().t() + b64.detach().abs()
    d = ((K + 3) * U * A_y).max(dim=1, keepdim=True).values
    p = torch.softmax(y64.detach(), dim=1)
    A = float(y64.detach().abs().max()) + float(d.max())
    shift = (1.0 / B) * p * torch.expm1(2 * d)
    e_dy = U * 2 * (dy64 + shift) + 1e-12 * (1 + A) + shift
    lim_w = (B + 2) * U * ((dy64 + e_dy).t() @ x64.abs()) + e_dy.t() @ x64.abs()
    lim_b = U * (dy64 + e_dy).sum(dim=0) + e_dy.sum(dim=0)
    err_w, err_b = (dw.double() - w64.grad).abs(), (db.double() - b64.grad).abs()
    print("dW: worst err / bound %.3g; db: %.3g" % (float((err_w / lim_w).max()), float((err_b / lim_b).max())))
    assert bool((err_w <= lim_w).all()) and bool((err_b <= lim_b).all())
    dw2, db2 = device()
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


# ---- for tools/loss_errors.py --------------------------------------------------------------------------------------------------------------

def measure():
    """[(case, shape, via, output, worst err / bound)]"""
    rows = []
    for C in class_counts():
        for B in ref.SHAPE_B:
            for mode in ref.MODES:
                case = ref.shape_case(B, C, mode)
                for o, q in ref.ratios(run_api(case), ref.cross_entropy(**case)).items():
                    rows.append((mode[0], (B, C), "cross_entropy_train", o, q))
    for name, case in VALUE_CASES.items():
        want = ref.cross_entropy(**case)
        for via, got in (("cross_entropy_train", run_api(case)), ("entry points", run_abi(case, ldx=case["x"].shape[1] + 3, shift=True))):
            for o, q in ref.ratios(got, want).items():
                rows.append((name, case["x"].shape, via, o, q))
    for F in (32, 2048):
        import ssg_amd
        lut0, x, gy = _oim_data(F)
        for pattern, t in OIM_TARGETS.items():
            for m in (0.0, 0.5, 0.9):
                t = np.asarray(t)
                lut, xd = cuda(lut0), cuda(x).requires_grad_(True)
                torch.autograd.grad(ssg_amd.oim(xd, cuda(t), lut, momentum=m), xd, cuda(gy))
                want = ref.oim_update(lut0, x, t, m)
                err = np.abs(lut.cpu().numpy().astype(np.float64) - want).max()
                rows.append(("oim_%s_m%g" % (pattern, m), (6, OIM_C, F), "oim", "lut" + (" (bit-equal)" if err == 0 else ""), err / (2.0 ** -22 / (1 - m))))
    return rows
