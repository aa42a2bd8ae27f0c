"""Yardstick of the train-mode batch normalisation tests: the formulas restated step by step in torch on the CPU, in the dtype asked for
(float64: the reference; float32: the arithmetic a user gets from torch without the kernels).  No call of F.batch_norm here --
tests/test_batchnorm_host.py checks this file against it.

    mean = E[x], var = E[(x - mean)^2] over (N, *spatial);  invstd = 1 / sqrt(var + eps);  xh = (x - mean) * invstd
    z = xh * weight + bias [+ residual];  y = max(z, 0) with relu, else z
    running_mean = (1 - f) running_mean + f mean;  running_var = (1 - f) running_var + f var n / (n - 1)
    g = gy * [y > 0] with relu, else gy;  dbias = sum g;  dweight = sum g xh
    dx = (g - dbias / n - xh dweight / n) * invstd * weight;  dresidual = g
"""
import torch

MARGIN = 2.0 ** -8          # every pre-activation of the test data is at least this far from 0 (in float64)


def _dims(x):
    return [0] + list(range(2, x.dim()))


def _bc(v, x):
    """[C] -> broadcastable against x [N, C, ...]"""
    return v.view([1, -1] + [1] * (x.dim() - 2))


def count(x):
    return x.numel() // x.shape[1]


def forward(x, weight, bias, eps=1e-5, relu=False, residual=None, dtype=torch.float64):
    x, w, b = x.to(dtype), weight.to(dtype), bias.to(dtype)
    mean = x.mean(_dims(x))
    var = ((x - _bc(mean, x)) ** 2).mean(_dims(x))
    invstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - _bc(mean, x)) * _bc(invstd, x)
    z = xh * _bc(w, x) + _bc(b, x)
    if residual is not None:
        z = z + residual.to(dtype)
    y = torch.clamp(z, min=0.0) if relu else z
    return dict(mean=mean, var=var, invstd=invstd, xh=xh, z=z, y=y)


def running_update(running_mean, running_var, mean, var, n, f, dtype=torch.float64):
    """-> (running_mean, running_var) after one batch with factor f"""
    rm, rv, mean, var = running_mean.to(dtype), running_var.to(dtype), mean.to(dtype), var.to(dtype)
    return (1.0 - f) * rm + f * mean, (1.0 - f) * rv + f * (var * (float(n) / float(n - 1)))


def backward(x, weight, fwd, gy, relu=False, dtype=torch.float64):
    """fwd: the dict of forward() in the same dtype -> dict(dx, dweight, dbias, dresidual)"""
    x, w, gy = x.to(dtype), weight.to(dtype), gy.to(dtype)
    n = float(count(x))
    g = gy * (fwd["y"] > 0).to(dtype) if relu else gy
    xh = fwd["xh"]
    db = g.sum(_dims(x))
    dw = (g * xh).sum(_dims(x))
    dx = (g - _bc(db, x) / n - xh * _bc(dw, x) / n) * _bc(fwd["invstd"] * w, x)
    return dict(dx=dx, dweight=dw, dbias=db, dresidual=g)


def rel_err(v, ref64):
    v, ref64 = torch.as_tensor(v).detach().cpu().double(), ref64.double()
    assert v.shape == ref64.shape, (tuple(v.shape), tuple(ref64.shape))
    den = float(ref64.abs().max())
    return float((v - ref64).abs().max()) / (den if den > 0 else 1.0)


def min_margin(x, weight, bias, eps, residual=None):
    """smallest |z| of the float64 forward"""
    return float(forward(x, weight, bias, eps, False, residual)["z"].abs().min())


def nudge(x, weight, bias, eps, residual=None, frozen_channels=()):
    """float32 test data whose ReLU mask cannot depend on the precision: move x (or the residual, where there is one) until every
    pre-activation has |z| >= MARGIN in float64.  Without a residual the elements of x that are too close are pushed away from the
    boundary by 4 * MARGIN in z (which shifts the statistics a little, hence the rounds); with one, the residual takes the push and
    one round does.  `frozen_channels` of x are never touched (a constant channel: its z is the bias).  -> (x, residual); gives up
    with an assertion after 8 rounds."""
    x = x.clone()
    residual = None if residual is None else residual.clone()
    for _ in range(8):
        f = forward(x, weight, bias, eps, False, residual)
        bad = f["z"].abs() < MARGIN
        if not bool(bad.any()):
            return x, residual
        sign = torch.where(f["z"] < 0, -1.0, 1.0).double()
        if residual is not None:
            residual = torch.where(bad, (residual.double() + sign * 4 * MARGIN).float(), residual)
        else:
            step = 4 * MARGIN / _bc(f["invstd"] * weight.double(), x)          # moves z by 4 * MARGIN (to first order)
            for c in frozen_channels:
                assert not bool(bad[:, c].any()), "a frozen channel is too close to 0: choose its bias away from 0"
            x = torch.where(bad, (x.double() + sign * step).float(), x)
    raise AssertionError("no margin of %g after 8 rounds" % MARGIN)


def make_case(shape, seed, kind=None):
    """seeded float32 inputs of one case: x, weight, bias, residual, gy, running_mean, running_var (CPU tensors), nudged so that both
    the variant without and the one with the residual keep the margin.  kind: None, 'large_mean' (x = 1000 + N(0, 1)), 'const' (channel
    1 of x holds one value)"""
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    x = torch.randn(shape, generator=g)
    weight = torch.randn(C, generator=g)
    weight = torch.where(weight.abs() < 0.25, weight.sign() * 0.25 + (weight == 0).float() * 0.25, weight)     # |w| >= 0.25
    bias = torch.randn(C, generator=g)
    residual = torch.randn(shape, generator=g)
    gy = torch.randn(shape, generator=g)
    running_mean = torch.randn(C, generator=g)
    running_var = torch.rand(C, generator=g) + 0.5
    frozen = ()
    if kind == "large_mean":
        x = x + 1000.0
    if kind == "const":
        x[:, 1] = 0.7251
        bias[1] = -0.5
        frozen = (1,)
    eps = 1e-5
    x, _ = nudge(x, weight, bias, eps, None, frozen)
    _, residual = nudge(x, weight, bias, eps, residual)
    return dict(x=x, weight=weight, bias=bias, residual=residual, gy=gy, running_mean=running_mean, running_var=running_var, eps=eps)
