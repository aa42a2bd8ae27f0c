"""CPU checks of the single-gallery-shot CMC protocol: the restatement tests/cmc_sgs_ref.py against what the reference itself gave
(tests/golden/cmc_sgs_cases.npz: curves, words consumed, the stream's next draws), the argument validation of the ssg_cmc_sgs_* entry
points, and what ssg_amd.ranking decides before it touches the device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cmc_sgs_ref as ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cmc_sgs_cases.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def test_cases_are_the_recorded_ones(gold):
    assert list(gold["cases"]) == list(ref.CASES)
    for name in ref.CASES:
        case = ref.make_case(name)
        assert [ref.sha(case[k]) for k in ("dist", "qid", "gid", "qcam", "gcam")] == list(gold[name + "_sha256"])
        if name + "_dist" in gold:
            assert all(np.array_equal(case[k], gold[name + "_" + k]) for k in ("dist", "qid", "gid", "qcam", "gcam"))


@pytest.mark.parametrize("name", list(ref.CASES))
def test_restatement_equals_golden(gold, name):
    for sep in (False, True):
        r = ref.run_case(name, sep)
        assert np.array_equal(r["k"], gold["%s_s%d_k" % (name, sep)])
        rs = np.random.RandomState(0); rs.set_state(r["state"])
        nxt = (rs.standard_normal(), rs.random_sample())
        for fmb in (False, True):
            tag = "%s_s%d_f%d_" % (name, sep, fmb)
            assert r["consumed"] == int(gold[tag + "consumed"])
            assert nxt == (float(gold[tag + "next_normal"]), float(gold[tag + "next_uniform"]))
            if gold[name + "_raised"][ref.SETTINGS.index((sep, fmb))]:
                with pytest.raises(RuntimeError, match="No valid query"):
                    ref.curve(r["k"], r["topk"], fmb)
            else:
                assert np.array_equal(ref.curve(r["k"], r["topk"], fmb), gold[tag + "curve"])


def test_restatement_keeps_a_cached_gaussian(gold):
    r = ref.run_case(ref.GAUSS_CASE, True, gauss=True)
    assert r["state"]["has_gauss"] == 1 and r["consumed"] == int(gold["gauss_consumed"])
    rs = np.random.RandomState(0); rs.set_state(r["state"])
    assert (rs.standard_normal(), rs.random_sample()) == (float(gold["gauss_next_normal"]), float(gold["gauss_next_uniform"]))
    assert np.array_equal(ref.curve(r["k"], r["topk"], False), gold["gauss_curve"])


def test_draw_rule_is_numpys_choice():
    """np.random.choice(list) of the installed numpy against the masked-rejection rule, word for word"""
    for s in (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 257, 300, 16384):
        np.random.seed(s)
        st = ref.Stream(np.random.get_state(legacy=False))
        got = [int(np.random.choice(list(range(s)))) for _ in range(200)]
        assert got == [ref.draw(st, s) for _ in range(200)], s
        rs = np.random.RandomState(0); rs.set_state(st.state_after())
        assert rs.random_sample() == np.random.random_sample()
        if s & (s - 1) == 0:
            assert st.consumed == (0 if s == 1 else 200)          # one entry: no word; a power of two never rejects
        else:
            assert st.consumed > 200


def test_entry_points_validate_without_gpu():
    from ssg_amd import _lib
    L = _lib.lib()
    assert L.ssg_cmc_sgs_max_group() == 16384
    assert L.ssg_cmc_sgs_workspace_bytes(1, 131072, 16384) > 2 * 8 * 131072
    assert L.ssg_cmc_sgs_workspace_bytes(4, 100, 7) >= 4 * (16 * 100 + 4 * 8 + 4 * 7 + 8 + 20 * 7)
    for mq, n, G in ((0, 10, 2), (1, 0, 1), (1, 10, 0), (1, 131073, 5), (1, 10, 16385)):
        assert L.ssg_cmc_sgs_workspace_bytes(mq, n, G) == 0
    ws = (np.zeros(1 << 16, np.uint64)).ctypes.data           # host memory: never dereferenced, the calls below are refused before a launch
    assert L.ssg_cmc_sgs_groups(None, 1, 131073, 131073, None, None, None, None, None, None, 5, 0, ws, 1 << 19, None) == -1
    assert b"n=131073" in L.ssg_last_error()
    assert L.ssg_cmc_sgs_groups(None, 1, 10, 10, None, None, None, None, None, None, 16385, 0, ws, 1 << 19, None) == -1
    assert b"G=16385" in L.ssg_last_error()
    assert L.ssg_cmc_sgs_groups(None, 1, 10, 10, None, None, None, None, None, None, 2, 0, None, 0, None) == -1          # no workspace
    assert L.ssg_cmc_sgs_groups(None, 1, 10, 10, None, None, None, None, None, None, 2, 0, ws, 16, None) == -1           # too small
    assert b"workspace" in L.ssg_last_error()
    assert L.ssg_cmc_sgs_groups(None, 1, 10, 10, None, None, None, None, None, None, 2, 0, ws, 1 << 19, None) == -1      # null inputs
    assert L.ssg_cmc_sgs_groups(ws, 1, 10, 8, ws, ws, ws, ws, ws, ws, 2, 0, ws, 1 << 19, None) == -1 and b"ld=8" in L.ssg_last_error()
    assert L.ssg_cmc_sgs_draws(ws, 1 << 19, 1, 10, 2, None, 0, 0, None, None) == -1                                         # no state
    assert L.ssg_cmc_sgs_draws(ws, 1 << 19, 1, 10, 2, None, 0, 64, ws, None) == -1 and b"nwords=64" in L.ssg_last_error()   # words announced, none given
    assert L.ssg_cmc_sgs_draws(ws, 1 << 19, 0, 10, 2, ws, 0, 64, ws, None) == -1
    assert L.ssg_cmc_sgs_counts(ws, 1 << 19, 1, 10, 2, None, None) == -1
    assert L.ssg_cmc_sgs_counts(None, 1 << 19, 1, 10, 2, ws, None) == -1


def test_limits_are_refused_before_the_device_is_touched():
    from ssg_amd import ranking
    big = np.zeros((1, 131073), np.float32)
    with pytest.raises(ValueError, match="n = 131073"):
        ranking.cmc(big, [0], np.zeros(131073), [0], np.ones(131073), single_gallery_shot=True, rng=0)
    d = np.zeros((1, 16385), np.float32)
    with pytest.raises(ValueError, match="G = 16385"):
        ranking.cmc(d, [0], np.arange(16385), [0], np.ones(16385), single_gallery_shot=True, rng=0)
    d = np.zeros((1, 16390), np.float32)
    with pytest.raises(ValueError, match="16385 entries"):
        ranking.single_shot_ranks(d, [0], np.r_[np.zeros(16385), np.arange(1, 6)], [0], np.ones(16390), rng=0)
    with pytest.raises(ValueError, match="do not match"):
        ranking.cmc(np.zeros((2, 5), np.float32), [0], np.arange(5), [0, 0], np.ones(5), single_gallery_shot=True, rng=0)


def test_rng_kinds():
    from ssg_amd import ranking
    d = np.zeros((2, 5), np.float32)
    before = np.random.get_state()
    with pytest.raises(NotImplementedError, match="rng="):
        ranking.cmc(d, single_gallery_shot=True)
    for bad in (np.random.default_rng(0), np.random.RandomState(np.random.PCG64(1)), "seed", 1.5, True):
        with pytest.raises(TypeError, match="rng must be"):
            ranking.cmc(d, single_gallery_shot=True, rng=bad)
    with pytest.raises(TypeError, match="rng must be"):
        ranking.evaluate_all(d, query_ids=[0, 1], gallery_ids=np.arange(5), query_cams=[0, 0], gallery_cams=np.ones(5),
                             cmc_protocols=("cuhk03",), rng=np.random.default_rng(0))
    with pytest.raises(NotImplementedError):
        ranking.evaluate_all(d, query_ids=[0, 1], gallery_ids=np.arange(5), query_cams=[0, 0], gallery_cams=np.ones(5), cmc_protocols=("cuhk03", "market1501"))
    with pytest.raises(ValueError, match="cmc_protocols"):
        ranking.evaluate_all(d, query_ids=[0, 1], gallery_ids=np.arange(5), query_cams=[0, 0], gallery_cams=np.ones(5), cmc_protocols=("viper",))
    after = np.random.get_state()
    assert before[2] == after[2] and np.array_equal(before[1], after[1])


def test_legacy_stream_words_and_commit():
    """the host side of the word supply: any pattern of top-ups yields the stream's words, commit(c) leaves the stream c words on"""
    from ssg_amd import ranking
    rs = np.random.RandomState(7)
    rs.standard_normal()
    want = np.random.RandomState(7); want.standard_normal()
    expect = want.randint(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)
    st = ranking._LegacyStream(rs)
    assert np.array_equal(st.words(0, 64)[:64], expect[:64])
    assert np.array_equal(st.words(10, 64)[:64], expect[10:74])
    assert np.array_equal(st.words(70, 3000)[:3000], expect[70:3070])
    assert np.array_equal(st.words(3069, 1)[:1], expect[3069:3070])
    st.commit(3071)
    want2 = np.random.RandomState(7); want2.standard_normal(); want2.randint(0, 1 << 32, 3071, dtype=np.uint64)
    assert rs.standard_normal() == want2.standard_normal() and rs.random_sample() == want2.random_sample()


def test_export():
    import ssg_amd
    from ssg_amd import ranking
    assert ssg_amd.single_shot_ranks is ranking.single_shot_ranks
