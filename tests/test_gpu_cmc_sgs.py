"""The single-gallery-shot CMC protocol on the device (csrc/cmc_sgs.hip, ssg_amd.ranking) against what the reference itself gave on
the cases of tests/cmc_sgs_ref.py (tests/golden/cmc_sgs_cases.npz): curves bit for bit, and the numpy stream left exactly where the
reference's loop leaves it."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cmc_sgs_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cmc_sgs_cases.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def cases():
    return {name: ref.make_case(name) for name in ref.CASES}


def _args(case):
    return case["dist"], case["qid"], case["gid"], case["qcam"], case["gcam"]


def _cmc(case, sep, fmb, rng):
    from ssg_amd import ranking
    return ranking.cmc(*_args(case), topk=case["topk"], separate_camera_set=sep, single_gallery_shot=True, first_match_break=fmb, rng=rng)


def _same_stream(a, b):
    return a[2] == b[2] and np.array_equal(a[1], b[1]) and a[3:] == b[3:]


@pytest.mark.parametrize("sep, fmb", ref.SETTINGS)
@pytest.mark.parametrize("name", list(ref.CASES))
def test_global_stream_equals_reference(gold, cases, name, sep, fmb):
    tag = "%s_s%d_f%d_" % (name, sep, fmb)
    np.random.seed(ref.CASES[name]["stream"])
    if gold[name + "_raised"][ref.SETTINGS.index((sep, fmb))]:
        with pytest.raises(RuntimeError, match="No valid query"):
            _cmc(cases[name], sep, fmb, np.random)
    else:
        assert np.array_equal(_cmc(cases[name], sep, fmb, np.random), gold[tag + "curve"])
    assert np.random.standard_normal() == float(gold[tag + "next_normal"])
    assert np.random.random_sample() == float(gold[tag + "next_uniform"])


def test_cached_gaussian_survives(gold, cases):
    name = ref.GAUSS_CASE
    np.random.seed(ref.CASES[name]["stream"])
    np.random.standard_normal()                          # leaves the second value of the pair in the state
    assert np.array_equal(_cmc(cases[name], True, False, np.random), gold["gauss_curve"])
    assert np.random.standard_normal() == float(gold["gauss_next_normal"])
    assert np.random.random_sample() == float(gold["gauss_next_uniform"])


@pytest.mark.parametrize("name", ["mixed", "tied", "smalltopk"])
def test_randomstate_instance_and_int_seed(gold, cases, name):
    tag = name + "_s1_f0_"
    np.random.seed(4242)
    before = np.random.get_state()
    rs = np.random.RandomState(ref.CASES[name]["stream"])
    assert np.array_equal(_cmc(cases[name], True, False, rs), gold[tag + "curve"])
    assert rs.standard_normal() == float(gold[tag + "next_normal"]) and rs.random_sample() == float(gold[tag + "next_uniform"])
    assert _same_stream(before, np.random.get_state())
    assert np.array_equal(_cmc(cases[name], True, False, ref.CASES[name]["stream"]), gold[tag + "curve"])
    assert np.array_equal(_cmc(cases[name], True, False, np.int64(ref.CASES[name]["stream"])), gold[tag + "curve"])
    assert _same_stream(before, np.random.get_state())


@pytest.mark.parametrize("sep", [False, True])
@pytest.mark.parametrize("name", list(ref.CASES))
def test_single_shot_ranks_equal_restatement(gold, cases, name, sep):
    import torch
    from ssg_amd import ranking
    k = ranking.single_shot_ranks(*_args(cases[name]), separate_camera_set=sep, rng=ref.CASES[name]["stream"])
    assert k.is_cuda and k.dtype == torch.int32 and tuple(k.shape) == (cases[name]["dist"].shape[0], 10)
    assert np.array_equal(k.cpu().numpy(), gold["%s_s%d_k" % (name, sep)])
    assert ranking.single_shot_ranks.last_consumed == int(gold["%s_s%d_f0_consumed" % (name, sep)])


def test_device_distance_block_with_row_pitch(gold, cases):
    import torch
    from ssg_amd import ranking
    case = cases["mixed"]
    m, n = case["dist"].shape
    padded = torch.full((m, n + 37), -9.0, device="cuda"); padded[:, :n] = torch.from_numpy(case["dist"]).cuda()
    k = ranking.single_shot_ranks(padded[:, :n], *_args(case)[1:], separate_camera_set=True, rng=ref.CASES["mixed"]["stream"])
    assert np.array_equal(k.cpu().numpy(), gold["mixed_s1_k"])


def test_refill_path(gold, cases, monkeypatch):
    """word blocks of 64: the draw stage runs out again and again, stores where it stopped and resumes"""
    from ssg_amd import ranking
    rejections = {n: int(gold[n + "_s1_f0_consumed"]) - int(gold[n + "_s1_draws"]) for n in ref.CASES}
    name = max(rejections, key=rejections.get)
    assert rejections[name] > 1000
    free = ranking.single_shot_ranks(*_args(cases[name]), separate_camera_set=True, rng=ref.CASES[name]["stream"]).cpu().numpy()
    consumed = ranking.single_shot_ranks.last_consumed
    monkeypatch.setenv("SSG_CMC_SGS_WORDS", "64")
    rs = np.random.RandomState(ref.CASES[name]["stream"])
    forced = ranking.single_shot_ranks(*_args(cases[name]), separate_camera_set=True, rng=rs).cpu().numpy()
    assert np.array_equal(forced, free) and np.array_equal(forced, gold[name + "_s1_k"])
    assert ranking.single_shot_ranks.last_consumed == consumed == int(gold[name + "_s1_f0_consumed"])
    assert rs.standard_normal() == float(gold[name + "_s1_f0_next_normal"])
    np.random.seed(ref.CASES[name]["stream"])
    assert np.array_equal(_cmc(cases[name], True, False, np.random), gold[name + "_s1_f0_curve"])
    assert np.random.standard_normal() == float(gold[name + "_s1_f0_next_normal"])


@pytest.mark.parametrize("name", ["mixed", "rejects", "large"])
def test_one_query_per_chunk(gold, cases, name, monkeypatch):
    from ssg_amd import ranking
    monkeypatch.setenv("SSG_CMC_SGS_CHUNK", "1")
    for sep in (False, True):
        k = ranking.single_shot_ranks(*_args(cases[name]), separate_camera_set=sep, rng=ref.CASES[name]["stream"]).cpu().numpy()
        assert np.array_equal(k, gold["%s_s%d_k" % (name, sep)])
        assert ranking.single_shot_ranks.last_consumed == int(gold["%s_s%d_f0_consumed" % (name, sep)])


def test_evaluate_all_table(gold, cases):
    from oracle import eval_oracle
    from ssg_amd import ranking
    name = "mixed"
    case = cases[name]
    kw = dict(query_ids=case["qid"], gallery_ids=case["gid"], query_cams=case["qcam"], gallery_cams=case["gcam"])
    curves = {"allshots": eval_oracle.cmc(*_args(case)), "cuhk03": gold[name + "_s1_f0_curve"],
              "market1501": eval_oracle.cmc(*_args(case), first_match_break=True)}
    head = "Mean AP: {:4.1%}\n".format(eval_oracle.mean_ap(*_args(case)))
    np.random.seed(ref.CASES[name]["stream"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        top1 = ranking.evaluate_all(case["dist"], cmc_protocols=("allshots", "cuhk03", "market1501"), rng=np.random, **kw)
    assert buf.getvalue() == head + ref.reference_table(curves)
    assert top1 == curves["market1501"][0]
    assert np.random.standard_normal() == float(gold[name + "_s1_f0_next_normal"])           # only 'cuhk03' consumed words
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        top1 = ranking.evaluate_all(case["dist"], cmc_protocols=("cuhk03", "allshots"), rng=ref.CASES[name]["stream"], cmc_topk=(1, 3), **kw)
    two = {p: curves[p] for p in ("allshots", "cuhk03")}
    assert buf.getvalue() == head + ref.reference_table(two, (1, 3)) and top1 == curves["cuhk03"][0]
    # the default call prints and returns what it always did
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        top1 = ranking.evaluate_all(case["dist"], **kw)
    want = head + "CMC Scores{:>12}\n".format("market1501") + "".join("top-{:<4}{:12.1%}\n".format(k, curves["market1501"][k - 1]) for k in (1, 5, 10))
    assert buf.getvalue() == want and top1 == curves["market1501"][0]


def test_without_rng_still_not_implemented(cases):
    from ssg_amd import ranking
    before = np.random.get_state()
    with pytest.raises(NotImplementedError, match="rng="):
        ranking.cmc(*_args(cases["mixed"]), single_gallery_shot=True)
    assert _same_stream(before, np.random.get_state())
