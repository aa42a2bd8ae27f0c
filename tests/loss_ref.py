"""Float64 yardstick of the classification losses (csrc/softmax_ce.hip, ssg_amd/loss.py): a restatement in numpy float64 of the
reference's FocalLoss (reid/loss/triplet.py:79-106), WeightCE (reid/loss/weight_cross_entropy.py:17-23), OIM / OIMLoss
(reid/loss/oim.py:14-27, 47-52), of nn.CrossEntropyLoss as reid/eug.py:132 builds it, and of accuracy
(reid/evaluation_metrics/classification.py:6-19), with their gradients towards the logits written out.

Everything goes through `cross_entropy`, the row-wise log-softmax cross-entropy with a per-row factor

    lse_i = max + log(sum exp(x - max)),  logpt_i = x[i][t_i] - lse_i,  s_i = row_w_i * class_w[t_i] * (1 - exp(logpt_i))^gamma,
    loss_i = -s_i * logpt_i,  dx[i][j] = g_i * r * s_i * (exp(x[i][j] - lse_i) - [j == t_i])

(the focal factor is a constant of the backward: triplet.py:97 detaches pt).  The conventions that are this project's, not the
reference's: a row whose target is ignore_index has s = 0, zero gradient and is in no denominator; a target outside [0, C) gives NaN in
its row, in the batch loss and in its gradient row, and counts in the weighted mean's denominator with class weight 1.

The bound the GPU tests assert is derived, not measured: every device output is a float64 value rounded once to float32, so

    |got - ref64| <= 2^-23 |ref64| + 1e-12 (1 + A) max(1, |factor|)

with A the largest finite |logit| of the case.  The absolute term covers what two float64 evaluations may differ by (the cancellation in
p - 1 near p = 1, lse of magnitude A).  `factor` is g_i r s_i for dx, s_i for a row loss, and r * sum_i |s_i| for the batch loss, a sum
of B row terms whose absolute errors add."""
import numpy as np

U23 = 2.0 ** -23
REDUCTIONS = ("none", "sum", "batch_mean", "mean")


def cross_entropy(x, target, row_w=None, class_w=None, gamma=0.0, reduction="mean", ignore_index=-100, g=None):
    """-> dict(lse [B], s [B], row_loss [B], loss (None under 'none'), r, dx [B, C], A) in float64; g: the upstream gradient, a scalar or
    [B] under 'none' (default ones)"""
    x32 = np.asarray(x, dtype=np.float32)
    x = x32.astype(np.float64)
    t = np.asarray(target, dtype=np.int64)
    B, C = x.shape
    with np.errstate(all="ignore"):
        mx = x.max(axis=1)
        lse = mx + np.log(np.exp(x - mx[:, None]).sum(axis=1))
        ignored = t == ignore_index
        bad = ~ignored & ((t < 0) | (t >= C))
        ok = ~ignored & ~bad
        tc = np.where(ok, t, 0)
        w = np.ones(B) if row_w is None else np.asarray(row_w, dtype=np.float32).astype(np.float64)
        if class_w is not None:
            w = w * np.where(ok, np.asarray(class_w, dtype=np.float32).astype(np.float64)[tc], 1.0)
        logpt = x[np.arange(B), tc] - lse
        f = np.ones(B) if gamma == 0 else np.power(1.0 - np.exp(logpt), gamma)
        s = np.where(ignored, 0.0, np.where(bad, np.nan, w * f))
        row_loss = np.where(ignored, 0.0, np.where(bad, np.nan, -s * logpt))
        tot = 0.0
        for v in row_loss:                          # ascending row order
            tot += v
        W = 0.0
        for v in np.where(ignored, 0.0, w):
            W += v
        den = {"none": 1.0, "sum": 1.0, "batch_mean": float(B), "mean": W}[reduction]
        r = np.float64(1.0) / np.float64(den)
        loss = None if reduction == "none" else (tot if reduction == "sum" else np.float64(tot) / np.float64(den))
        gv = np.ones(B) if g is None else np.broadcast_to(np.asarray(g, dtype=np.float32).astype(np.float64), (B,))
        coef = (gv * r) * s
        onehot = np.zeros((B, C))
        onehot[np.arange(B)[ok], t[ok]] = 1.0
        dx = coef[:, None] * (np.exp(x - lse[:, None]) - onehot)
        dx[ignored] = 0.0
        dx[bad] = np.nan
    finite = np.abs(x[np.isfinite(x)])
    return dict(lse=lse, s=s, row_loss=row_loss, loss=loss, r=r, dx=dx, coef=np.where(ignored, 0.0, coef), A=float(finite.max()) if finite.size else 0.0)


def bound(ref64, A, factor):
    """the asserted bound of an output with float64 value ref64 (see the module's docstring); non-finite factors count as 1"""
    with np.errstate(all="ignore"):
        fac = np.abs(np.asarray(factor, dtype=np.float64))
        fac = np.where(np.isfinite(fac), np.maximum(fac, 1.0), 1.0)
        ref = np.abs(np.asarray(ref64, dtype=np.float64))
        return U23 * np.where(np.isfinite(ref), ref, 0.0) + 1e-12 * (1.0 + A) * fac


def ratio(got, ref64, lim):
    """worst |got - ref64| / lim over the finite elements of ref64; where ref64 is NaN or infinite `got` must be the same (else inf)"""
    got = np.asarray(got, dtype=np.float64).reshape(np.shape(ref64))
    ref64 = np.asarray(ref64, dtype=np.float64)
    lim = np.broadcast_to(np.asarray(lim, dtype=np.float64), ref64.shape)
    fin = np.isfinite(ref64)
    same = np.where(np.isnan(ref64), np.isnan(got), got == ref64)
    if not bool(same[~fin].all()):
        return float("inf")
    if not fin.any():
        return 0.0
    with np.errstate(all="ignore"):
        q = np.abs(got[fin] - ref64[fin]) / lim[fin]
    return float("inf") if np.isnan(q).any() else float(q.max())


def ratios(got, ref):
    """{output: worst error-to-bound ratio} of got = dict(loss | row_loss, dx) against cross_entropy's dict"""
    A, out = ref["A"], {}
    with np.errstate(all="ignore"):
        if ref["loss"] is None:
            out["row_loss"] = ratio(got["loss"], ref["row_loss"], bound(ref["row_loss"], A, ref["s"]))
        else:
            s = ref["s"][np.isfinite(ref["s"])]
            out["loss"] = ratio(got["loss"], ref["loss"], bound(ref["loss"], A, ref["r"] * np.abs(s).sum()))
        out["dx"] = ratio(got["dx"], ref["dx"], bound(ref["dx"], A, ref["coef"][:, None]))
    return out


# ---- the reference's classes -------------------------------------------------------------------------------------------------------------

def focal_loss(x, target, gamma=2.0, alpha=None, size_average=True):
    """triplet.py:88-106: logpt = log_softmax gathered at the target, pt = exp(logpt) detached, logpt *= alpha[target],
    loss = -(1 - pt)^gamma logpt, mean or sum"""
    return cross_entropy(x, target, class_w=alpha, gamma=gamma, reduction="batch_mean" if size_average else "sum", ignore_index=-(1 << 62))


def weight_ce(x, target, w):
    """weight_cross_entropy.py:19-22: loss = sum_i w[i] * CE(x[i], t[i]); loss /= B"""
    return cross_entropy(x, target, row_w=w, reduction="batch_mean", ignore_index=-(1 << 62))


def cross_entropy_loss(x, target, weight=None, reduction="mean", ignore_index=-100):
    """nn.CrossEntropyLoss: under 'mean' the sum of w[t_i] ce_i over the sum of w[t_i], the rows that are not ignored"""
    return cross_entropy(x, target, class_w=weight, reduction=reduction, ignore_index=ignore_index)


def oim_update(lut, x, target, momentum):
    """oim.py:24-26 row by row in batch order; the table row is stored as float32 after each sample's update.  -> the new table"""
    lut = np.array(lut, dtype=np.float32)
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    m = np.float64(momentum)
    with np.errstate(all="ignore"):
        for xi, y in zip(x, np.asarray(target)):
            if y < 0 or y >= lut.shape[0]:
                continue
            v = m * lut[y].astype(np.float64) + (1.0 - m) * xi
            lut[y] = (v / np.sqrt((v * v).sum())).astype(np.float32)
    return lut


def oim_loss(x, target, lut, scalar=1.0, momentum=0.5, weight=None, size_average=True, g_logits=None):
    """oim.py:14-27 and 47-52: logits = scalar * x lut^T, loss = F.cross_entropy(logits, target, weight, size_average); the backward
    gives grad_inputs = grad_outputs lut on the table from BEFORE the update, then updates the table.
    -> dict(logits, A_logits, loss ..., dx_inputs, A_dx_inputs, lut)"""
    x64, l64 = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(lut, dtype=np.float32).astype(np.float64)
    raw = x64 @ l64.T
    logits = (raw.astype(np.float32) * np.float32(scalar))
    ce = cross_entropy(logits, target, class_w=weight, reduction="mean" if size_average else "sum")
    g = ce["dx"].astype(np.float32).astype(np.float64) * scalar if g_logits is None else np.asarray(g_logits, dtype=np.float64)
    return dict(raw=raw, A_raw=np.abs(x64) @ np.abs(l64).T, ce=ce, g_raw=g, dx_inputs=g @ l64, A_dx_inputs=np.abs(g) @ np.abs(l64),
                lut=oim_update(lut, x, target, momentum))


def ranks(x, target):
    """#{j : x[i][j] > x[i][t] or (x[i][j] == x[i][t] and j < t)}; C for a target out of range"""
    x = np.asarray(x, dtype=np.float32)
    B, C = x.shape
    out = np.full(B, C, dtype=np.int64)
    for i, t in enumerate(np.asarray(target)):
        if 0 <= t < C:
            out[i] = int((x[i] > x[i, t]).sum()) + int((x[i, :t] == x[i, t]).sum())
    return out


def accuracy(x, target, topk=(1,)):
    """classification.py:6-19: correct_k.float().sum().mul_(1. / batch_size), a float32 product, per k; [float32 array of one element]"""
    rk = ranks(x, target)
    B = len(rk)
    return [np.array([np.float32(int((rk < k).sum())) * np.float32(1.0 / B)], dtype=np.float32) for k in topk]


# ---- cases -------------------------------------------------------------------------------------------------------------------------------

SHAPE_B = (1, 3, 128, 257)
# (name, gamma, class weights, row weights, reduction)
MODES = (("ce_mean", 0.0, False, False, "mean"), ("focal_alpha", 0.5, True, False, "batch_mean"), ("focal2_sum", 2.0, False, False, "sum"),
         ("rows_none", 0.0, False, True, "none"))


def shape_case(B, C, mode, seed=0):
    """dict(x, target, row_w, class_w, gamma, reduction, g) of random logits N(0, 3^2)"""
    _, gamma, cw, rw, reduction = mode
    rng = np.random.default_rng(1000 * seed + 7 * B + C)
    return dict(x=(3.0 * rng.standard_normal((B, C))).astype(np.float32), target=rng.integers(0, C, B).astype(np.int64),
                class_w=rng.uniform(0.25, 2.0, C).astype(np.float32) if cw else None, row_w=rng.uniform(0.0, 1.0, B).astype(np.float32) if rw else None,
                gamma=gamma, reduction=reduction, ignore_index=-100,
                g=rng.standard_normal(B).astype(np.float32) if reduction == "none" else np.float32(rng.uniform(0.5, 2.0)))


def value_cases(C=65, B=6):
    """name -> case dict: the special values, on a shape with a ragged last quad"""
    rng = np.random.default_rng(5)
    base = (3.0 * rng.standard_normal((B, C))).astype(np.float32)
    tgt = rng.integers(0, C, B).astype(np.int64)
    cases = {}

    def add(name, x, target=tgt, class_w=None, row_w=None, gamma=0.0, reduction="mean", ignore_index=-100, g=np.float32(1.5)):
        cases[name] = dict(x=np.ascontiguousarray(x, dtype=np.float32), target=np.asarray(target, dtype=np.int64), class_w=class_w, row_w=row_w, gamma=gamma,
                           reduction=reduction, ignore_index=ignore_index, g=g)

    sign = np.where(rng.random((B, C)) < 0.5, -1.0, 1.0)
    for gamma in (0.0, 2.0):
        add("pm80_g%g" % gamma, 80.0 * sign, gamma=gamma)
        add("pm1e4_g%g" % gamma, 1e4 * sign, gamma=gamma)
    x = base.copy(); x[1] = 2.5; x[4] = -7.0
    add("equal_rows", x, gamma=0.5, reduction="sum")
    x = base.copy()
    for i in range(B):
        x[i, (tgt[i] + 1 + i) % C] = -np.inf
    add("neg_inf_elsewhere", x)
    add("neg_inf_elsewhere_focal", x, gamma=2.0, reduction="batch_mean")
    x = base.copy(); x[2, tgt[2]] = -np.inf
    add("neg_inf_target", x, reduction="none", g=np.ones(B, dtype=np.float32))
    add("neg_inf_target_sum", x, reduction="sum")
    for lead in (8.0, 16.0, 28.0, 80.0):                # pt from 1 - 1e-2 to exactly 1
        x = (0.5 * rng.standard_normal((B, C))).astype(np.float32)
        x[np.arange(B), tgt] = lead
        for gamma in (0.0, 0.5, 2.0):
            add("pt_near_1_lead%g_g%g" % (lead, gamma), x, gamma=gamma, reduction="sum")
    cw = rng.uniform(0.5, 2.0, C).astype(np.float32); cw[tgt[0]] = 0.0; cw[(tgt[0] + 1) % C] = 0.0
    add("zero_class_weight", base, class_w=cw)
    add("zero_class_weight_focal", base, class_w=cw, gamma=2.0, reduction="batch_mean")
    t = tgt.copy(); t[1] = -100; t[4] = -100
    add("some_ignored", base, target=t, class_w=cw)
    add("some_ignored_none", base, target=t, reduction="none", g=rng.standard_normal(B).astype(np.float32))
    add("ignore_inside_range", base, target=np.where(np.arange(B) % 2 == 0, 3, tgt), ignore_index=3)
    add("all_ignored", base, target=np.full(B, -100))
    add("all_ignored_sum", base, target=np.full(B, -100), reduction="sum")
    for name, badv in (("target_eq_C", C), ("target_negative", -5), ("target_huge", 1 << 40)):
        t = tgt.copy(); t[3] = badv
        add(name, base, target=t, class_w=cw)
        add(name + "_none", base, target=t, reduction="none", g=np.ones(B, dtype=np.float32))
    return cases
