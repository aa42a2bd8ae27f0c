"""What tests/test_fold_host.py and tests/test_gpu_fold.py share: crafted Conv2d + BatchNorm parameters for the device fold
(csrc/fold.hip) and the host reference they are held to -- `_fold` of ssg_amd/resnet.py and, for the dual form, the lines of
`ResNet._prepare` that build the [conv3 | downsample] row from two host folds.  Everything here is CPU torch."""
import torch

from ssg_amd import resnet

EPS = resnet._BN_EPS
POW2_J = (-20, -3, 0, 5, 13, 14, 15)          # crafted row maxima 2^j (8192 and 16384 among them), each exact and one float32 ulp above / below
N_POW2_ROWS = 3 * len(POW2_J)
ROW_ZERO, ROW_TINY_GAMMA, ROW_HUGE_GAMMA, ROW_VAR0, ROW_NEG_GAMMA = range(N_POW2_ROWS, N_POW2_ROWS + 5)


def folded_value(w, gamma, var):
    """float32(w * gamma / sqrt(var + eps)) in float64, the arithmetic of `_fold`"""
    return (w.double() * (gamma.double() / torch.sqrt(var.double() + EPS))).float()


def _weight_for(target, gamma, var):
    """a float32 w with folded_value(w) == target (float32 scalar tensor) among the neighbours of target / scale, or None: the
    products of consecutive w lie scale ulps of w apart, which just below a power of two is more than one ulp of the target"""
    scale = gamma.double() / torch.sqrt(var.double() + EPS)
    w0 = (target.double() / scale).float()
    up, down = torch.tensor(float("inf")), torch.tensor(float("-inf"))
    cands = [w0]
    for _ in range(3):
        cands = [torch.nextafter(cands[0], down)] + cands + [torch.nextafter(cands[-1], up)]
    for w in cands:
        if folded_value(w, gamma, var) == target:
            return w
    return None


def _crafted_max(target):
    """-> (w, gamma) with var = 1 that fold to exactly `target`: gamma = 1 (scale 1 - 5e-6) where that hits, else a scale just above
    1/2, where the weight sits at the top of its binade and nearly every target has a preimage"""
    for gm in (1.0, 0.51, 0.52, 0.53, 0.55, 0.6, 0.7):
        w = _weight_for(target, torch.tensor(gm), torch.tensor(1.0))
        if w is not None:
            return w, gm
    raise AssertionError("no float32 weight folds to %r" % float(target))


def crafted(cout, cin, kh, kw, seed, quiet_head=False):
    """-> {'w' [cout,cin,kh,kw], 'gamma', 'beta', 'mean', 'var'}: Kaiming-like weights and random statistics as
    `synthetic_state_dict` draws them, with the first rows crafted (var = 1 and gamma = 1, or just above 1/2, in the rows whose maximum is crafted):
      rows 0 .. 3*len(POW2_J)-1   row maximum after folding exactly 2^j, one ulp above, one ulp below; the 2^14 row also holds values
                                  whose lo half is a half subnormal (1 + 2^-20), zero (exact halves) and whose hi half is subnormal
      ROW_ZERO all-zero weights;  ROW_TINY_GAMMA gamma = 1e-12 (the exponent clamp +40);  ROW_HUGE_GAMMA gamma = 1e6;
      ROW_VAR0 running_var = 0;   ROW_NEG_GAMMA gamma < 0
    quiet_head: the crafted-maximum rows and the zero row are all zero instead (the second source of a dual form, so that the maximum
    of the concatenated row is the first source's)."""
    g = torch.Generator().manual_seed(seed)
    n = cin * kh * kw
    w = (torch.randn(cout, n, generator=g) * (2.0 / (cout * kh * kw)) ** 0.5)
    gamma = torch.rand(cout, generator=g) + 0.5
    beta = torch.randn(cout, generator=g) * 0.1
    mean = torch.randn(cout, generator=g) * 0.1
    var = torch.rand(cout, generator=g) + 0.5
    one = torch.tensor(1.0)
    inf = torch.tensor(float("inf"))
    if quiet_head:
        w[:ROW_ZERO + 1] = 0
    else:
        row = 0
        for j in POW2_J:
            p = torch.tensor(2.0 ** j)
            for target in (p, torch.nextafter(p, inf), torch.nextafter(p, -inf)):
                wmax, gm = _crafted_max(target)
                gamma[row] = gm; var[row] = 1.0
                w[row] *= 2.0 ** j / (4.0 * w[row].abs().max())             # everything else at most a quarter of the maximum
                w[row, (7 * row + 3) % n] = wmax * (-1.0 if row % 2 else 1.0)
                if j == 14 and target is p and n >= 8:
                    picks = (1.0 + 2.0 ** -20, 1.0, 0.5 + 2.0 ** -11, 3.0e-6, 2.0 ** -24, 1.5 * 2.0 ** -25)
                    for i, val in enumerate(picks):
                        w[row, (7 * row + 4 + i) % n] = _weight_for(torch.tensor(val), torch.tensor(gm), one)
                row += 1
        w[ROW_ZERO] = 0
    gamma[ROW_TINY_GAMMA] = 1e-12
    gamma[ROW_HUGE_GAMMA] = 1e6
    var[ROW_VAR0] = 0.0
    gamma[ROW_NEG_GAMMA] = -0.75
    return dict(w=w.view(cout, cin, kh, kw).contiguous(), gamma=gamma, beta=beta, mean=mean, var=var)


def check_crafted(case):
    """the crafted properties hold in the reference arithmetic (a test of the test data, run once by the host test)"""
    w = folded_value(case["w"].flatten(1), case["gamma"].view(-1, 1), case["var"].view(-1, 1))
    mx = w.abs().amax(dim=1)
    inf = torch.tensor(float("inf"))
    row = 0
    for j in POW2_J:
        p = torch.tensor(2.0 ** j)
        for target in (p, torch.nextafter(p, inf), torch.nextafter(p, -inf)):
            assert mx[row] == target, (row, j, float(mx[row]), float(target))
            row += 1
    assert mx[ROW_ZERO] == 0
    sc = resnet._row_scales(w)
    assert sc[ROW_TINY_GAMMA] == 2.0 ** 40 and float(mx[ROW_TINY_GAMMA]) * 2.0 ** 40 < 8192         # the clamp is active
    r14 = 3 * POW2_J.index(14)
    v = w[r14] * sc[r14]
    lo = (v - v.half().float()).half()
    tiny = 2.0 ** -14
    assert sc[r14] == 1.0 and ((lo != 0) & (lo.float().abs() < tiny)).any() and (lo == 0).any() and ((v != 0) & (v.abs() < tiny)).any()


def _sd(case, conv="c", bn="b"):
    return {conv + ".weight": case["w"], bn + ".weight": case["gamma"], bn + ".bias": case["beta"], bn + ".running_mean": case["mean"],
            bn + ".running_var": case["var"]}


def host_fold(case, split):
    """-> (w, bias, cscale or None) of `_fold` on the CPU"""
    f = resnet._fold(_sd(case), "c", "b", 1, 0, "cpu", split=split)
    return f.w, f.bias, f.cscale


def host_fold_dual(case1, case2, split):
    """the [conv3 | downsample] row as `ResNet._prepare` builds it on the host: two plain folds, concatenated along K, one row scale
    over the concatenated row, the biases added in float32"""
    c3 = resnet._fold(_sd(case1), "c", "b", 1, 0, "cpu")
    ds = resnet._fold(_sd(case2), "c", "b", 1, 0, "cpu")
    wcat = torch.cat([c3.w, ds.w], dim=1)
    bias = (c3.bias + ds.bias).contiguous()
    if not split:
        return wcat.contiguous(), bias, None
    sc = resnet._row_scales(wcat)
    return resnet._h8l8(wcat * sc.view(-1, 1)), bias, (1.0 / sc).contiguous()
