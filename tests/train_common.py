"""What the train-mode suites (tests/test_gpu_conv_train.py, test_gpu_conv_strided.py, test_gpu_head.py) and their yardsticks
(tests/conv_train_ref.py, conv_strided_ref.py, head_ref.py) share: the unit roundoff and the derived bound, the handles on the library,
the mutated references that show what the bound can see (`sensitivity`, host only), and the composition harness (a model whose ReLU inputs stay away from 0, its parameter gradients, and the criterion

    err(device) <= F_COMP * err(float32 CPU run) + 2^-24,   err(v) = max |v - ref64| / max |ref64|

with the F_COMP of each suite).  A plain module, imported by name: no fixture lives here."""
import copy

import torch

U = 2.0 ** -24
FLOOR = 2.0 ** -24


def bound(L, A):
    """|dev - ref64| <= (L + 2) 2^-24 A: a length-L float32 sum in any order, plus one rounding"""
    return (L + 2) * U * A


def _lib():
    from ssg_amd import _lib as m
    return m.lib()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _err(v, r):
    return float((v - r).abs().max()) / float(r.abs().max())


def check_bound(reference, case, got, which):
    """every element of the outputs `which` of `got` meets (L + 2) 2^-24 A of `reference(*case)`"""
    _, r64, A, L = reference(*case)
    for o in which:
        g = got[o].detach().cpu().double()
        assert g.shape == r64[o].shape and bool(torch.isfinite(g).all()), o
        err, lim = (g - r64[o]).abs(), bound(L[o], A[o])
        worst = float((err / lim.clamp_min(1e-300)).max())
        print("%s %s: max |dev - ref64| = %.3g, worst err / bound = %.3g (L = %d)" % (case[:6], o, float(err.max()), worst, L[o]))
        assert bool((err <= lim).all()), "%s: %s misses (L + 2) 2^-24 A by a factor of %.3g" % (case[:6], o, worst)


def bound_rows(reference, outputs, name, case, routes, outs):
    """the rows of a conv suite's measure(): (case, shape, path, output, max |dev - ref64|, max |f32 CPU - ref64|, worst err_dev / bound)"""
    d, r64, A, L = reference(*case)
    f32 = outputs(d["x"], d["w"], d["gy"], d["pad"], torch.float32)
    rows = []
    for path, got in routes:
        for o in outs:
            err = (got[o].detach().cpu().double() - r64[o]).abs()
            rows.append((name, case[:6], path, o, float(err.max()), float((f32[o].double() - r64[o]).abs().max()),
                         float((err / bound(L[o], A[o]).clamp_min(1e-300)).max())))
    return rows


# ---- what the bound can see --------------------------------------------------------------------------------------------------------------

def tap_reach(B, H, W, k, stride):
    """[k, k, B, OH, OW] bool: tap (r, s) of output pixel (b, oh, ow) reads inside the H x W image (padding k // 2)"""
    p = k // 2
    OH, OW = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    ih = torch.arange(OH)[None, :] * stride + torch.arange(k)[:, None] - p                 # [k, OH]
    iw = torch.arange(OW)[None, :] * stride + torch.arange(k)[:, None] - p                 # [k, OW]
    ok = ((ih >= 0) & (ih < H))[:, None, :, None] & ((iw >= 0) & (iw < W))[None, :, None, :]
    return ok[:, :, None].expand(k, k, B, OH, OW)


def tap_hits(H, W, k, stride, r, s):
    """[H, W] bool: the input pixels that tap (r, s) of some output pixel reads (ih = oh stride + r - k // 2 with 0 <= oh < OH)"""
    p = k // 2
    OH, OW = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    th, tw = torch.arange(H) + p - r, torch.arange(W) + p - s
    ok_h = (th >= 0) & (th % stride == 0) & (th // stride < OH)
    ok_w = (tw >= 0) & (tw % stride == 0) & (tw // stride < OW)
    return ok_h[:, None] & ok_w[None, :]


def sensitivity(reference, case, stride):
    """How much of a plausible kernel fault the bound (L + 2) 2^-24 A sees.  Three mutated float64 references of `reference(*case)`:
        y   one 32-channel chunk of one tap missing from the weight        (the last chunk of the last tap)
        dx  one stage of 32 output channels of one tap missing             (the last 32 output channels of the last tap)
        dw  the last 32 output pixels missing
    -> {output: (fraction of the touched elements on which |mutated - ref64| > bound, number of touched elements)}; an element is
    touched when the missing terms include one that reads inside the image."""
    from torch.nn import grad as G
    B, H, W, cin, cout, k, _ = case
    d, r64, A, L = reference(*case)
    x, w, gy, pad = d["x"].double(), d["w"].double(), d["gy"].double(), d["pad"]
    r = s = k - 1
    reach = tap_reach(B, H, W, k, stride)
    mut, touched = {}, {}
    wm = w.clone()
    wm[:, cin - 32:, r, s] = 0
    mut["y"] = torch.nn.functional.conv2d(x, wm, None, stride, pad)
    touched["y"] = reach[r, s][:, None].expand_as(r64["y"])
    wm = w.clone()
    wm[cout - 32:, :, r, s] = 0
    mut["dx"] = G.conv2d_input(x.shape, wm, gy, stride, pad)
    touched["dx"] = tap_hits(H, W, k, stride, r, s)[None, None].expand_as(r64["dx"])
    gm = gy.permute(0, 2, 3, 1).contiguous()                                               # [B, OH, OW, Cout]: pixels in the kernels' order
    gm.view(-1, cout)[-32:] = 0
    mut["dw"] = G.conv2d_weight(x, w.shape, gm.permute(0, 3, 1, 2), stride, pad)
    touched["dw"] = reach.reshape(k, k, -1)[:, :, -32:].any(2)[None, None].expand_as(r64["dw"])
    out = {}
    for o in ("y", "dx", "dw"):
        assert mut[o].shape == r64[o].shape and bool(touched[o].any()), o
        seen = (mut[o] - r64[o]).abs() > bound(L[o], A[o])
        assert not bool(seen[~touched[o]].any()), o                                          # the untouched elements did not move
        out[o] = (float(seen[touched[o]].double().mean()), int(touched[o].sum()))
    return out


def check_sensitivity(reference, outputs, cases, stride, need=0.75):
    """every case: each mutation of `sensitivity` breaks the bound on at least `need` of the elements it touches, and torch's float32
    CPU convolution (a correct float32 implementation) meets the bound everywhere"""
    for name, case in cases.items():
        d, r64, A, L = reference(*case)
        f32 = outputs(d["x"], d["w"], d["gy"], d["pad"], torch.float32)
        fr = sensitivity(reference, case, stride)
        ok32 = {o: float(((f32[o].double() - r64[o]).abs() / bound(L[o], A[o]).clamp_min(1e-300)).max()) for o in fr}
        print("%-22s %-28s seen: y %.3f dx %.3f dw %.3f   float32 CPU err / bound: y %.3g dx %.3g dw %.3g"
              % (name, case[:6], fr["y"][0], fr["dx"][0], fr["dw"][0], ok32["y"], ok32["dx"], ok32["dw"]))
        for o in fr:
            assert fr[o][0] >= need, (name, o, fr[o])
            assert ok32[o] <= 1.0, (name, o, ok32[o])


# ---- composition -----------------------------------------------------------------------------------------------------------------------

def relu_margin(model, x, calls):
    """the smallest |input| any nn.ReLU of `model` sees in a float64 train-mode forward of x; the ReLUs run `calls` times in all"""
    m = copy.deepcopy(model).double().train()
    seen = []
    hooks = [r.register_forward_pre_hook(lambda mod, inp: seen.append(float(inp[0].detach().abs().min())))
             for r in m.modules() if isinstance(r, torch.nn.ReLU)]
    m(x.double())
    for h in hooks:
        h.remove()
    assert len(seen) == calls
    return min(seen)


def quiet_data(seeds, make_model, make_inputs, calls, margin):
    """(model in float32 on the CPU, x, what else make_inputs gives): the first seed whose ReLU inputs all stay `margin` away from 0
    in float64.  The batch norms get weights in [0.5, 1.5) and biases in [-0.5, 0.5); make_inputs(generator) -> (x, ...)."""
    for seed in seeds:
        torch.manual_seed(seed)
        model = make_model()
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                torch.nn.init.uniform_(m.weight, 0.5, 1.5)
                torch.nn.init.uniform_(m.bias, -0.5, 0.5)
        data = make_inputs(torch.Generator().manual_seed(seed))
        if relu_margin(model, data[0], calls) >= margin:
            return (model,) + tuple(data)
    raise AssertionError("no seed keeps the ReLU inputs away from 0")


def grads(model, backward):
    """{parameter: gradient in float64 on the CPU} after `backward(model)` ran one train-mode forward + backward from zeroed gradients"""
    model.train()
    model.zero_grad()
    backward(model)
    return {n: p.grad.detach().cpu().double() for n, p in model.named_parameters() if p.grad is not None}


def reference_grads(data, calls, margin, backward):
    """(float64, float32) CPU parameter gradients of `quiet_data`'s (model, x, ...) under `backward(model, x, ...)`"""
    model = data[0]
    assert relu_margin(model, data[1], calls) >= margin           # before anything touches the device
    as64 = [[e.double() for e in t] if isinstance(t, list) else t.double() for t in data[1:]]
    g64 = grads(copy.deepcopy(model).double(), lambda m: backward(m, *as64))
    g32 = grads(copy.deepcopy(model), lambda m: backward(m, *data[1:]))
    return g64, g32


def composition_rows(g64, g32, dev):
    """[(parameter, err_dev, err_f32)] of the parameter gradients"""
    assert sorted(dev) == sorted(g64)
    return [(n, _err(dev[n], g64[n]), _err(g32[n], g64[n])) for n in g64]


def check_composition(rows, f_comp, width=22):
    for n, e_dev, e_f32 in rows:
        print("%-*s err_dev %.3g  err_f32 %.3g  ratio %.3g" % (width, n, e_dev, e_f32, e_dev / e_f32 if e_f32 else float("inf")))
        assert e_dev <= f_comp * e_f32 + FLOOR, (n, e_dev, e_f32)


def composition_table(rows, f_comp, width=24):
    """the lines tools/*_errors.py write below their composition header: one per parameter gradient, then the worst counting ratio"""
    lines = ["%-*s %11s %11s %9s" % (width, "parameter", "err_dev", "err_f32", "ratio")]
    worst = 0.0
    for n, e_dev, e_f32 in rows:
        ratio = e_dev / e_f32 if e_f32 > 0 else float("inf") if e_dev > 0 else 0.0
        if e_dev > FLOOR:
            worst = max(worst, ratio)
        lines.append("%-*s %11.3e %11.3e %9.3g%s" % (width, n, e_dev, e_f32, ratio, " *" if e_dev > FLOOR else ""))
    lines.append("worst ratio among gradients with err_dev > 2^-24 (*): %.3g; the test asserts F_COMP = %g" % (worst, f_comp))
    return lines
