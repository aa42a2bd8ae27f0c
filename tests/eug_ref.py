"""Plain restatements and case tables for the SSG++ label step (csrc/eug.hip behind ssg_amd.eug), shared by tests/test_eug_range_host.py
(no GPU) and tests/test_gpu_eug_range.py.  numpy itself is the reference of every case: `pairwise_norm` restates what
np.linalg.norm(l - u, axis=1) does in float32 (the host suite holds it to the installed numpy bit for bit), `dist_label_ref` is the
loop of reid/eug.py:232-240 on a float32 matrix, `select_ref` the stable-argsort rule of ssg_amd.select_top.  The generators are
seeded; nothing here touches the device."""
import numpy as np

F32 = np.float32
PW_BLOCK = 128        # numpy's pairwise-sum leaf (PW_BLOCKSIZE)
CHUNK = 8192          # numpy's reduction buffer: s = s + pairwise(chunk)

# every width class of kernel a: d < 8 and the < 8 second chunk (8193..8199), leaves with a tail (d % 8 != 0), the 128 / 256 leaf
# and split edges, 6 and 7 splits below one chunk (2047, 4103), a full evaluation stack (8185, 8191, 16383, 32767), two, three and
# four chunks, the accepted maximum
D_EDGE = [1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 137, 255, 256, 257, 263, 1000, 2047, 4103, 8184, 8185, 8191, 8192, 8193,
          8195, 8199, 8201, 8329, 16383, 16385, 16391, 24577, 32767, 32768]
D_FULL_STACK = [8185, 8191, 16383, 32767]
D_WIDE = [8191, 32768]                           # also run with a wide dynamic range
NU, NL = 33, 130                                 # two u blocks (the second ragged), three l tiles (the last ragged), three splits
MAXD = 8                                         # EUG_MAXD
TU, TL = 32, 64                                  # EUG_TU, EUG_TL

# ------------------------------------------------------------------ kernel a: the restatement


def leaf_sum(sq):
    """numpy's pairwise leaf over the last axis of float32 `sq` (at most 128 columns): fewer than 8 -> 0 + x0 + x1 ...; else 8 running
    sums over the whole groups of 8, folded ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail one by one"""
    n = sq.shape[-1]
    assert 1 <= n <= PW_BLOCK and sq.dtype == F32
    if n < 8:
        res = np.zeros(sq.shape[:-1], F32)
        for k in range(n):
            res = res + sq[..., k]
        return res
    body = n - n % 8
    r = sq[..., 0:8].copy()
    for k in range(8, body, 8):
        r = r + sq[..., k:k + 8]
    res = ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))
    for k in range(body, n):
        res = res + sq[..., k]
    return res


def _squares(l, u, a, b):
    df = l[..., a:b] - u[..., a:b]               # rounded once
    return df * df                               # rounded once more: no fused multiply-add


def _pairwise(l, u, a, n):
    """-> (float32 sum of the squares of columns [a, a + n), the evaluation-stack entries it needed)"""
    if n <= PW_BLOCK:
        return leaf_sum(_squares(l, u, a, a + n)), 1
    n2 = n // 2
    n2 -= n2 % 8
    left, dl = _pairwise(l, u, a, n2)
    right, dr = _pairwise(l, u, a + n2, n - n2)  # `left` stays live while the right half is evaluated
    return left + right, max(dl, 1 + dr)


def pairwise_norm(l_row, u_row):
    """np.linalg.norm(l_row - u_row, axis=-1) restated in sequential float32: difference and square rounded separately, numpy's
    pairwise order within chunks of 8192 columns, s = s + pairwise(chunk) from s = 0, np.sqrt last.  The last axis is the feature
    axis, the leading ones broadcast (the rows are independent).  -> (norm, the deepest evaluation stack it needed)"""
    l, u = np.asarray(l_row, F32), np.asarray(u_row, F32)
    d = l.shape[-1]
    assert u.shape[-1] == d and d >= 1
    s = np.zeros(np.broadcast_shapes(l.shape[:-1], u.shape[:-1]), F32)
    depth = 0
    with np.errstate(all="ignore"):
        for c0 in range(0, d, CHUNK):
            p, dp = _pairwise(l, u, c0, min(CHUNK, d - c0))
            s = s + p
            depth = max(depth, dp)
        return np.sqrt(s), depth


def run_program(prog, l_row, u_row):
    """executes a leaf program of eug_build_program -- rows (start, length, pops, chunk end) -- the way eug_nn_kernel does: push the
    leaf, `pops` times replace the two top entries by below + top, at a chunk end s = s + top; -> (norm, the most live entries)"""
    l, u = np.asarray(l_row, F32), np.asarray(u_row, F32)
    s = np.zeros(np.broadcast_shapes(l.shape[:-1], u.shape[:-1]), F32)
    stack, peak = [], 0
    with np.errstate(all="ignore"):
        for start, length, pops, end in np.asarray(prog).tolist():
            stack.append(leaf_sum(_squares(l, u, start, start + length)))
            peak = max(peak, len(stack))
            for _ in range(pops):
                top = stack.pop()
                stack.append(stack.pop() + top)
            if end:
                s = s + stack.pop()
                assert not stack
        assert not stack
        return np.sqrt(s), peak


def naive_norm(l_row, u_row):
    """the same squares summed left to right in float32: what a kernel that ignored numpy's order would give"""
    l, u = np.asarray(l_row, F32), np.asarray(u_row, F32)
    with np.errstate(all="ignore"):
        sq = _squares(l, u, 0, l.shape[-1])
        return np.sqrt(np.cumsum(sq, axis=-1, dtype=F32)[..., -1])        # cumsum is sequential


def nn_ref(u, l):
    """the loop of reid/eug.py:205-209, row by row on numpy: -> (argmin int64 [Nu], min float32 [Nu])"""
    u, l = np.asarray(u), np.asarray(l)
    assert u.dtype == F32 and l.dtype == F32
    am, mv = np.empty(len(u), np.int64), np.empty(len(u), F32)
    with np.errstate(all="ignore"):
        for i, x in enumerate(u):
            dist = np.linalg.norm(l - x, axis=1)
            am[i] = np.argmin(dist)
            mv[i] = dist[am[i]]
    return am, mv


def features(nu, nl, d, seed, wide=False):
    """standard-normal float32 features; wide: every element times exp(uniform(-8, 8)), so the order of the additions shows in
    more than the last bit"""
    rng = np.random.default_rng(seed)
    u, l = rng.standard_normal((nu, d), dtype=F32), rng.standard_normal((nl, d), dtype=F32)
    if wide:
        u = u * np.exp(rng.uniform(-8, 8, u.shape)).astype(F32)
        l = l * np.exp(rng.uniform(-8, 8, l.shape)).astype(F32)
    return u, l


def width_seed(d):
    return 7000 + d


def labels_perm(nl, seed):
    """labels drawn from a permutation, so a wrong index gives a wrong label"""
    return np.random.default_rng(seed).permutation(nl).astype(np.int64) * 3 + 11


def structure(nu, nl, nsplit):
    """(u blocks, l tiles, l tiles per split) of eug_nn_kernel's grid for the split count ssg_eug_nn_splits returned"""
    ntiles = -(-nl // TL)
    return -(-nu // TU), ntiles, -(-ntiles // nsplit)


# ------------------------------------------------------------------ kernel a: exact ties between labelled rows
TIE_SHAPES = [(8197, 1283, 8), (NU, NL, 17)]
TIE_KINDS = ["next", "lanes", "column", "tile", "splits", "ragged", "zero", "all_equal", "everywhere"]


def tie_pairs(kind, nl, per):
    """the (j, copies of row j) groups of a tie case; `per` = l tiles per split.  Lane = j % 16 and register column = j % 64 // 16 of
    eug_nn_kernel; a copy in a LOWER lane than its original tells an index tie-break from a lane order"""
    last = (nl - 1) // TL * TL                   # first row of the last, ragged tile
    span = per * TL                              # rows of one split
    if kind in ("next", "zero"):
        return [(5, [6]), (15, [16]), (63, [64]), (nl - 2, [nl - 1])]
    if kind == "lanes":                          # within one 16-lane group, every butterfly distance, copy in a higher lane
        return [(0, [1]), (2, [4]), (16 + 3, [16 + 7]), (32 + 1, [32 + 9]), (48, [63])]
    if kind == "column":                         # another register column of the same tile, the copy in the same, a lower, a higher lane
        return [(4, [20]), (9, [24]), (10, [27]), (7, [48 + 2]), (64 + 13, [64 + 16])]
    if kind == "tile":                           # the next tile (the same split where a split has two tiles)
        return [(3, [3 + 64]), (12, [64 + 2]), (40, [64 + 57])]
    if kind == "splits":                         # two different splits, the copy in a lower lane and in the last split
        return [(8, [span + 3]), (21, [span + 21]), (37, [nl - 1])]
    if kind == "ragged":                         # inside the last, ragged tile, and from a whole tile into it
        return [(last, [last + 1]), (last - 30, [nl - 1])] if nl - last >= 3 else [(last, [last + 1])]
    if kind == "everywhere":                     # one row at many places
        return [(11, sorted({12, 26, 11 + 64, 64 + 2, span + 1, last, nl - 1}))]
    raise ValueError(kind)


def tie_case(nu, nl, d, kind, per, seed):
    """-> (u, l, {aimed u row: its group}, the groups).  Every aimed u row is a duplicated labelled row plus small noise (the copies
    are then at exactly the same distance, and nearest); the first one of every group is the row itself (distance exactly 0), in
    kind 'zero' all of them are"""
    u, l = features(nu, nl, d, seed)
    rng = np.random.default_rng(seed + 1)
    if kind == "all_equal":
        l[:] = l[0]
        return u, l, {r: 0 for r in range(nu)}, [(0, list(range(1, nl)))]
    groups = tie_pairs(kind, nl, per)
    for j, copies in groups:
        assert j < min(copies) and max(copies) < nl
        l[copies] = l[j]
    aim = {}
    for q, r in enumerate(rng.permutation(nu)[:min(nu, 6 * len(groups))].tolist()):      # spread over the u blocks
        aim[r] = q % len(groups)
        j = groups[aim[r]][0]
        u[r] = l[j] if (q < len(groups) or kind == "zero") else l[j] + F32(0.01) * rng.standard_normal(d, dtype=F32)
    return u, l, aim, groups


# ------------------------------------------------------------------ kernel a: special values
SPECIAL_WIDTHS = [9, 137]
SPECIAL_KINDS = ["nan_l", "nan_l2_splits", "nan_l2_tile", "nan_u", "inf_l", "inf_u", "inf_both", "overflow", "denormal"]


def special_case(kind, d, seed):
    u, l = features(NU, NL, d, seed)
    c = d // 2
    if kind == "nan_l":                          # every answer is that row, score NaN
        l[70, c] = np.nan
    elif kind == "nan_l2_splits":                # two NaN rows in different splits: the lower index
        l[100, c] = np.nan
        l[20, d - 1] = np.nan
    elif kind == "nan_l2_tile":                  # two in one tile, the lower index in the higher lane
        l[64 + 33, 0] = np.nan
        l[64 + 15, c] = np.nan
    elif kind == "nan_u":                        # every distance of that row is NaN: argmin 0
        u[17, c] = np.nan
        u[32, 0] = np.nan
    elif kind == "inf_l":                        # an infinite distance, which never wins
        l[5, c] = np.inf
    elif kind == "inf_u":                        # every distance of that row is +inf: argmin 0
        u[3, c] = np.inf
        u[32, d - 1] = -np.inf
    elif kind == "inf_both":                     # inf - inf = NaN for that pair alone
        u[9, c] = np.inf
        l[77, c] = np.inf
        u[32, 0] = -np.inf
        l[129, 0] = -np.inf
    elif kind == "overflow":                     # the squares overflow: every distance inf, argmin 0
        u, l = u * F32(1e20), l * F32(1e20)
    elif kind == "denormal":                     # the squares are float32 denormals; numpy keeps them
        u, l = u * F32(2.0 ** -70), l * F32(2.0 ** -70)
    else:
        raise ValueError(kind)
    return u, l


# ------------------------------------------------------------------ kernel b
DIST_SHAPES = [(1, 1), (1, 300), (63, 1), (64, 64), (65, 257), (127, 63), (128, 65), (129, 513), (4097, 70)]
DIST_KINDS = ["grid", "nan", "nan_column", "negative", "inf"]


def dist_label_ref(D, l_label):
    """the loop of reid/eug.py:232-240 on a float32 matrix: -> (labels, scores, confidence) float64 and the argmin"""
    D = np.asarray(D)
    assert D.dtype == F32 and D.ndim == 2
    nu = D.shape[0]
    labels, scores, conf, am = np.zeros(nu), np.zeros(nu), np.zeros(nu), np.zeros(nu, np.int64)
    with np.errstate(all="ignore"):
        for i, dist in enumerate(D):
            j = np.argmin(dist)
            am[i] = j
            scores[i] = -dist[j]
            labels[i] = int(l_label[j])
            conf[i] = F32(1) - dist[j] / np.max(D[:, j])
    return labels, scores, conf, am


def dist_case(nu, nl, kind, seed):
    """a [Nu, Nl] float32 matrix on the tie grid {0, 1/4 .. 1}: rows whose minimum stands at j and j + 1 and at j and j + 64 (other
    lanes of the row's wave: column j is lane j % 64), plus what `kind` adds.  No -0.0 anywhere: a column maximum of zero with both
    signs is np.max's own business"""
    rng = np.random.default_rng(seed)
    D = (rng.integers(0, 5, (nu, nl)) / 4).astype(F32)
    rows = rng.permutation(nu)

    def crafted(r, cols):
        D[r] = np.maximum(D[r], F32(0.5))
        D[r, [c for c in cols if c < nl]] = F32(0.25)
    if nu >= 6:
        crafted(rows[0], [nl - 2, nl - 1])
        crafted(rows[1], [3, 67])
        crafted(rows[2], [70, 6])
        crafted(rows[3], [nl - 1])
        crafted(rows[4], [63, 64, 128, 256, 512])
    if kind == "nan":                            # a NaN at column 70 and at column 5 of one row: 5 wins; a NaN in the last column
        r = rows[-1]
        D[r, min(70, nl - 1)] = np.nan
        D[r, min(5, nl - 1)] = np.nan
        if nu > 1:
            D[rows[-2], nl - 1] = np.nan
    elif kind == "nan_column":                   # a NaN in a column that only some rows select: only their confidence is NaN
        j = int(np.argmin(D[rows[0]]))
        D[rows[-1], j] = np.nan
    elif kind == "negative":
        D -= (rng.integers(0, 3, (nu, nl)) * F32(0.75)).astype(F32)
        if nl > 2:
            D[:, 2] = -np.abs(D[:, 2]) - F32(0.25)                         # a column whose maximum is negative
    elif kind == "inf":                          # +inf scattered and as a whole column; -inf in a third of the rows, twice in some
        D[rng.random((nu, nl)) < 0.05] = np.inf
        if nl > 1:
            D[:, 1] = np.inf
        for r in rows[:max(1, nu // 3)]:
            D[r, rng.integers(0, nl, 1 + r % 2)] = -np.inf
    assert not np.signbit(D[D == 0]).any()
    return D


# ------------------------------------------------------------------ selection
SELECT_N = [1023, 1024, 1025, 2049]
SELECT_KINDS = ["equal", "nan", "inf", "mixed", "grid"]


def select_ref(scores, k, labels=None):
    """the first k of a STABLE np.argsort(-scores) (NaN last, -0 == +0); with labels, those labelled -1 are dropped afterwards"""
    scores = np.asarray(scores, np.float64)
    mask = np.zeros(len(scores), bool)
    mask[np.argsort(-scores, kind="stable")[:k]] = True
    return mask if labels is None else mask & (np.asarray(labels, np.float64) != -1)


def select_case(n, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "equal":
        return np.full(n, -0.375)
    if kind == "nan":
        return np.full(n, np.nan)
    if kind == "inf":
        return rng.choice(np.array([np.inf, -np.inf, 0.0, -0.0, 1.0]), n)
    if kind == "mixed":
        return np.where(rng.random(n) < 0.3, np.nan, rng.choice(np.array([-np.inf, -1e300, -5e-324, -0.0, 0.0, 5e-324, 2.5, np.inf]), n))
    if kind == "grid":
        return -rng.integers(0, 7, n) / 8.0
    raise ValueError(kind)


def select_ks(scores):
    """0, 1, n - 1, n, and the cuts just before, inside and just after the widest run of equal scores in sorted order"""
    n = len(scores)
    s = -np.asarray(scores, np.float64)[np.argsort(-np.asarray(scores, np.float64), kind="stable")]
    same = np.concatenate([[False], (s[1:] == s[:-1]) | (np.isnan(s[1:]) & np.isnan(s[:-1]))])
    start = np.flatnonzero(~same)
    length = np.diff(np.concatenate([start, [n]]))
    a = int(start[np.argmax(length)])
    b = a + int(length.max())                    # the run is s[a:b]
    ks = {0, 1, n - 1, n, a, a + 1, (a + b) // 2, b - 1, b}
    return sorted(k for k in ks if 0 <= k <= n)


def select_labels(n, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([-1.0, 0.0, 3.0, np.nan, -1.0, 750.0]), n)
