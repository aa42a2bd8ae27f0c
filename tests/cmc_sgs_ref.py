"""Plain-Python restatement of the single-gallery-shot CMC protocol (reid/evaluation_metrics/ranking.py:10-16,53-66 with
single_gallery_shot=True), written for this project, and the cases tests/golden/cmc_sgs_cases.npz records the reference on.

The reference draws one gallery entry per identity with np.random.choice(list), ten times per query.  For a list of s entries that is
the legacy randint(0, s): s == 1 returns 0 and consumes nothing; otherwise successive 32-bit MT19937 words w are masked with
2^bit_length(s - 1) - 1 and the first w & mask <= s - 1 is the draw.  Queries, repeats and identities are visited in that nesting, the
identities in order of first appearance along the query's ranking, over valid entries only; the bin credited is the number of other
identities whose drawn entry is ranked before the drawn true match.  Equal distances are ordered by gallery index (a stable argsort)."""
import hashlib

import numpy as np

REPEAT = 10


class Stream(object):
    """the 32-bit words of a legacy MT19937 stream (a get_state(legacy=False) dict), read without touching it"""

    def __init__(self, state):
        assert state["bit_generator"] == "MT19937"
        self.start = state
        self.bg = np.random.MT19937()
        self.bg.state = {"bit_generator": "MT19937", "state": dict(state["state"])}
        self.buf = np.zeros(0, np.uint64)
        self.consumed = 0

    def word(self):
        if self.consumed >= len(self.buf):
            self.buf = np.concatenate([self.buf, self.bg.random_raw(4096)])
        self.consumed += 1
        return int(self.buf[self.consumed - 1])

    def state_after(self):
        """the legacy state after `consumed` words: the cached Gaussian of the original stays"""
        bg = np.random.MT19937()
        bg.state = {"bit_generator": "MT19937", "state": dict(self.start["state"])}
        bg.random_raw(self.consumed)
        out = dict(bg.state)
        out["has_gauss"] = self.start["has_gauss"]; out["gauss"] = self.start["gauss"]
        return out


def draw(stream, s, stats=None):
    """legacy randint(0, s)"""
    if s == 1:
        return 0
    mask = (1 << (s - 1).bit_length()) - 1
    while True:
        v = stream.word() & mask
        if v <= s - 1:
            if stats is not None:
                stats["draws"] += 1
            return v


def single_shot_ranks(dist, qid, gid, qcam, gcam, stream, separate_camera_set=False):
    """-> (k int32 [m, 10], -1 rows for queries without a valid true match; stats: group sizes met, draws made)"""
    dist = np.asarray(dist, np.float32); qid = np.asarray(qid); gid = np.asarray(gid); qcam = np.asarray(qcam); gcam = np.asarray(gcam)
    m = dist.shape[0]
    k = np.full((m, REPEAT), -1, np.int32)
    stats = {"sizes": set(), "draws": 0}
    for i in range(m):
        order = np.argsort(dist[i], kind="stable")
        valid = (gid[order] != qid[i]) | (gcam[order] != qcam[i])
        if separate_camera_set:
            valid &= gcam[order] != qcam[i]
        ids = gid[order][valid]                        # identities along the ranking, valid entries only
        if not (ids == qid[i]).any():
            continue
        groups = {}                                    # identity -> its rank positions, keyed in order of first appearance
        for pos, x in enumerate(ids.tolist()):
            groups.setdefault(x, []).append(pos)
        stats["sizes"].update(len(v) for v in groups.values())
        for r in range(REPEAT):
            chosen = {x: members[draw(stream, len(members), stats)] for x, members in groups.items()}
            mine = chosen[int(qid[i])]
            k[i, r] = sum(1 for p in chosen.values() if p < mine)
    return k, stats


def curve(k, topk=100, first_match_break=False):
    """the reference's accumulation (ranking.py:69-79): the same float64 adds in the same (query, repeat) order"""
    ret = np.zeros(topk)
    nvalid = 0
    for row in k:
        if row[0] < 0:
            continue
        for b in row:
            if b < topk:
                ret[b] += 1 if first_match_break else 1. / REPEAT
        nvalid += 1
    if nvalid == 0:
        raise RuntimeError("No valid query")
    return ret.cumsum() / nvalid


# ------------------------------------------------------------------ the recorded cases
# name -> seed of the case's generator, m, group sizes of the gallery identities (its n is their sum), cameras, topk, tied distances,
# seed of the stream the protocol consumes
CASES = {
    "mixed":   dict(seed=11, m=12, sizes=[1, 1, 2, 2, 3, 3, 5, 5, 4, 8, 9, 16, 17, 2, 3, 1, 6, 7, 10, 12, 33, 32, 16], ncam=4, topk=100, tied=False, stream=101),
    "tied":    dict(seed=12, m=8, sizes=[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], ncam=3, topk=100, tied=True, stream=102),
    "large":   dict(seed=13, m=6, sizes=[300, 600, 257] + [5] * 197 + [4] * 200 + [58], ncam=6, topk=100, tied=False, stream=103),
    "onecam":  dict(seed=14, m=4, sizes=[4] * 10, ncam=1, topk=100, tied=False, stream=104),
    "oneid":   dict(seed=15, m=3, sizes=[40], ncam=4, topk=100, tied=False, stream=105),
    "onequery": dict(seed=16, m=1, sizes=[3] * 20 + [5] * 8, ncam=3, topk=100, tied=False, stream=106),
    "smalltopk": dict(seed=17, m=10, sizes=[2] * 30 + [3] * 13, ncam=2, topk=3, tied=False, stream=107),
    "rejects": dict(seed=18, m=24, sizes=[5] * 60 + [9] * 30 + [17] * 12 + [33] * 6 + [65] * 2, ncam=5, topk=100, tied=True, stream=108),
    # more than 1024, 2048, 4096 and 8192 identities: the device orders them with 2, 4, 8 and 16 keys per thread
    "ids1100": dict(seed=19, m=3, sizes=[1] * 400 + [2] * 500 + [3] * 200, ncam=3, topk=100, tied=False, stream=109),
    "ids3000": dict(seed=20, m=1, sizes=[1] * 1500 + [2] * 1000 + [5] * 500, ncam=3, topk=100, tied=False, stream=110),
    "ids5000": dict(seed=21, m=1, sizes=[1] * 3000 + [2] * 1500 + [3] * 500, ncam=4, topk=100, tied=True, stream=111),
    "ids9000": dict(seed=22, m=2, sizes=[1] * 6000 + [2] * 2500 + [4] * 500, ncam=3, topk=100, tied=False, stream=112),
}
SETTINGS = [(False, False), (False, True), (True, False), (True, True)]     # (separate_camera_set, first_match_break)
GAUSS_CASE = "mixed"           # recorded once more with a cached Gaussian left in the stream before the call


def make_case(name):
    """-> dict(dist float32 [m, n], qid, gid, qcam, gcam int64, topk).  np.random.RandomState streams are frozen, so the seed is the case."""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"])
    sizes = c["sizes"]
    G, n, m = len(sizes), int(sum(sizes)), c["m"]
    names = np.arange(G, dtype=np.int64) * 7 + 3                     # gallery identities: small, then the junk id and large sparse ones
    if G >= 3:
        names[1] = -1; names[2] = 2000000011; names[G - 1] = 1999999
    gid = np.repeat(names, sizes)[rs.permutation(n)]
    gcam = rs.randint(0, c["ncam"], n)
    qid = names[rs.randint(0, G, m)]
    qcam = rs.randint(0, c["ncam"], m)
    if name == "mixed":
        qid[3] = 123456                                              # an identity the gallery does not hold
        qid[5] = names[0]; qcam[5] = gcam[gid == names[0]][0]        # its only gallery entry is on the query's camera: no valid match
    dist = rs.rand(m, n) - 0.35 * (gid[None, :] == qid[:, None]) - 0.1
    if c["tied"]:
        dist = np.round(dist * 16) / 16
    else:                                                            # distinct float32 values in every row
        dist = (np.argsort(np.argsort(dist, axis=1), axis=1) - n // 3) / 64.0
    return dict(dist=dist.astype(np.float32), qid=qid, gid=gid, qcam=qcam.astype(np.int64), gcam=gcam.astype(np.int64), topk=c["topk"])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(name, separate_camera_set, gauss=False):
    """the restatement on a case -> dict(k, consumed, stats, state) from a fresh RandomState(stream seed)"""
    case = make_case(name)
    rs = np.random.RandomState(CASES[name]["stream"])
    if gauss:
        rs.standard_normal()                                        # leaves the second value of the pair cached
    st = Stream(rs.get_state(legacy=False))
    k, stats = single_shot_ranks(case["dist"], case["qid"], case["gid"], case["qcam"], case["gcam"], st, separate_camera_set)
    return dict(k=k, consumed=st.consumed, stats=stats, state=st.state_after(), topk=case["topk"])


def reference_table(curves, cmc_topk=(1, 5, 10)):
    """the score table of reid/evaluators.py:120-126 for {protocol: curve} (protocols in the order allshots, cuhk03, market1501)"""
    names = [p for p in ("allshots", "cuhk03", "market1501") if p in curves]
    lines = ["CMC Scores" + "".join("{:>12}".format(p) for p in names)]
    for k in cmc_topk:
        lines.append("  top-{:<4}".format(k) + "".join("{:12.1%}".format(curves[p][k - 1]) for p in names))
    return "\n".join(lines) + "\n"
