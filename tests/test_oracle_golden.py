"""CPU suite: the oracle (oracle/ssg_oracle.c) against the committed golden vectors that were
produced by importing the reference (tools/make_golden.py).  No GPU, no /root/reference."""
import glob
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, bits


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


RERANK = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "rerank_n*.npz")) + glob.glob(os.path.join(GOLDEN, "rerank_tiefree_*.npz")) +
                glob.glob(os.path.join(GOLDEN, "rerank_var_*.npz")))


@pytest.mark.parametrize("name", RERANK)
def test_rerank_stages_match_reference(name, golden, ora):
    g = golden(name)
    mode = "stable" if bool(g["stable"]) else "introsort"   # 'ref' fixtures = untouched reference incl. unstable ties
    msave = bool(g["memory_save"]) if "memory_save" in g.files else False      # MemorySave=True branch, rerank.py:49-59
    e, f, st = ora.re_ranking(g["src"], g["tgt"], k1=int(g["k1"]), k2=int(g["k2"]), lambda_value=float(g["lambda_value"]),
                              MemorySave=msave, rank_mode=mode, stages=True)
    assert not bool(g["exp_quirk"])
    assert np.array_equal(st["rank"][:, :g["rank"].shape[1]], g["rank"])
    if "sha_euclid" in g.files:
        assert sha(e) == str(g["sha_euclid"])
        assert sha(st["V"]) == str(g["sha_V"])
        assert sha(st["V_qe"]) == str(g["sha_Vqe"])
        assert sha(st["jaccard"]) == str(g["sha_jaccard"])
        assert sha(f) == str(g["sha_final"])
    else:
        assert np.array_equal(bits(st["V"]), bits(g["V"])) and np.array_equal(bits(st["V_qe"]), bits(g["V_qe"]))
        assert np.array_equal(bits(st["jaccard"]), bits(g["jaccard"]))
    if bool(g["tie_free"]):     # the argsort kind cannot matter on a tie-free input
        e2, f2 = ora.re_ranking(g["src"], g["tgt"], k1=int(g["k1"]), k2=int(g["k2"]), lambda_value=float(g["lambda_value"]), rank_mode="stable")
        assert np.array_equal(f2, g["final"])
    if "final" in g.files:
        assert np.array_equal(f, g["final"])
        assert np.array_equal(bits(e), bits(g["euclid"]))
    # source term: row 0 of source_dist = half(v + v[0]) (rerank.py:43)
    v = st["v"]
    assert np.array_equal((v + v[0]).astype(np.float64), g["v"])
    eps, cnt, top = ora.eps_rule(f, float(g["rho"]))
    assert eps == float(g["eps"]) and cnt == int(g["count"]) and top == int(g["top_num"])
    assert np.array_equal(ora.dbscan(f, eps, 4), g["labels"])


def test_rerank_at_bench_width_matches_reference(golden, ora):
    """the oracle at the bench's feature width (d = 2048: 2048-term float64 cdist sums, rerank.py:37,61) against the
    UNTOUCHED reference run by tools/make_golden.py (--only-wide) at N = Ns = 2000 on the hard set, lambda = 0.3: every N x N
    stage by sha256, the first 21 rank columns, the source vector, eps and sklearn's labels.  The inputs are regenerated from their
    seeds (tools/synth.py) and checked against the stored sha256."""
    from conftest import hard_clustered
    g = golden("rerank_wide_d2048_ref.npz")
    N, Ns, d = int(g["N"]), int(g["Ns"]), int(g["d"])
    tgt = hard_clustered(N, d, int(g["seed_tgt"])); src = hard_clustered(Ns, d, int(g["seed_src"]), intra=float(g["intra_src"]))
    assert sha(tgt) == str(g["sha_tgt"]) and sha(src) == str(g["sha_src"]), "tools/synth.py no longer reproduces the fixture's inputs"
    ora.set_num_threads(min(os.cpu_count() or 8, 16))
    e, f, st = ora.re_ranking(src, tgt, k1=int(g["k1"]), k2=int(g["k2"]), lambda_value=float(g["lambda_value"]), rank_mode="introsort", stages=True)
    assert sha(e) == str(g["sha_euclid"]), "euclidean_dist"
    assert np.array_equal(st["rank"][:, :21], g["rank"]), "initial_rank[:, :21]"
    assert sha(st["V"]) == str(g["sha_V"]) and sha(st["V_qe"]) == str(g["sha_Vqe"]) and sha(st["jaccard"]) == str(g["sha_jaccard"])
    assert sha(f) == str(g["sha_final"]), "final_dist"
    assert np.array_equal((st["v"] + st["v"][0]).astype(np.float64), g["v"])
    eps, cnt, top = ora.eps_rule(f, float(g["rho"]))
    assert eps == float(g["eps"]) and cnt == int(g["count"]) and top == int(g["top_num"])
    assert np.array_equal(ora.dbscan(f, eps, 4), g["labels"])


@pytest.mark.parametrize("name", ["norerank_n256.npz", "norerank_n1024.npz"])
def test_norerank_path(name, golden, ora):
    g = golden(name)
    e, none = ora.re_ranking(g["tgt"][:8], g["tgt"], no_rerank=True)
    assert none is None and sha(e) == str(g["sha_euclid"])
    eps, cnt, top = ora.eps_rule(e, float(g["rho"]))
    assert np.float16(eps).view(np.uint16) == int(g["eps_bits"]) and cnt == int(g["count"]) and top == int(g["top_num"])
    assert np.array_equal(ora.dbscan(e.astype(np.float64), float(eps), 4), g["labels"])


def test_dbscan_cases(golden, ora):
    g = golden("dbscan_cases.npz")
    for D, eps, lab in zip(g["D"], g["eps"], g["labels"]):
        assert np.array_equal(ora.dbscan(D, float(eps), 4), lab)


def test_half_exp_table(golden, ora):
    """Correctly rounded half exp == this host's numpy table except the recorded quirk inputs."""
    g = golden("half_exp_table.npz")
    cr = ora.half_exp_table().view(np.uint16)
    npx = g["numpy_exp_bits"]
    allh = np.arange(65536, dtype=np.uint16).view(np.float16)
    diff = np.nonzero((cr != npx) & ~(np.isnan(cr.view(np.float16)) & np.isnan(npx.view(np.float16))))[0]
    assert set(diff.tolist()) == set(g["quirk_input_bits"].tolist())
    assert len(diff) <= 4
    # every differing entry is a 1-ulp difference
    assert np.all(np.abs(cr[diff].astype(np.int32) - npx[diff].astype(np.int32)) == 1)
    assert np.isfinite(allh[diff]).all()


def test_numpy_primitives(ora):
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(1, 900))
        a = rng.random(n).astype(np.float32)
        assert np.sum(a) == ora.pairwise_sum(a)
        b = rng.random(n)
        assert np.sum(b) == ora.pairwise_sum(b)
        h = (rng.integers(0, 30, n) / 32.0).astype(np.float16)
        assert np.array_equal(np.argsort(h), ora.argsort_half(h))
        assert np.sum(h) == np.float16(ora.pairwise_sum(h.astype(np.float32)))


def test_installed_numpy_introsort_threshold(ora):
    """The default rank_mode replays np.argsort's unstable introsort, whose tie order depends on the range size at which numpy
    switches to insertion sort.  The kernel (csrc/topk_intro.hip SSG_INTRO_SMALL), the oracle and the goldens use 15
    (`pr - pl > 15`: 17 elements are still partitioned), the behaviour of the numpy 2.2.6 build of this image; numpy's source
    constant reads 16.  This probe finds 17-element tie patterns on which the two thresholds order differently and checks that the
    INSTALLED numpy sides with 15 -- if it ever fails, rebuild with -DSSG_INTRO_SMALL=16 and regenerate the goldens."""
    rng = np.random.default_rng(11)
    probes = 0
    for _ in range(4000):
        h = (rng.integers(0, 4, 17) / 4.0).astype(np.float16)
        a15, a16 = ora.argsort_half(h, small=15), ora.argsort_half(h, small=16)
        if not np.array_equal(a15, a16):
            probes += 1
            assert np.array_equal(np.argsort(h), a15), "installed numpy %s partitions at a different range size than 15" % np.__version__
    assert probes > 20


def test_oracle_matches_scipy_cdist(ora):
    from scipy.spatial.distance import cdist
    rng = np.random.default_rng(3)
    x = rng.standard_normal((40, 37)).astype(np.float32)
    f = x.astype(np.float16)
    ref = np.power(cdist(f, f).astype(np.float16), 2).astype(np.float16)
    assert np.array_equal(bits(ora.euclid(x)), bits(ref))


def test_edge_cases(ora):
    # duplicates -> exact zeros; tiny N (< k1+1); all-identical source
    rng = np.random.default_rng(9)
    x = rng.standard_normal((12, 16)).astype(np.float32)
    x[5] = x[3]
    e, f = ora.re_ranking(x[:4], x, k1=20, k2=6, lambda_value=0.1)
    assert e[3, 5] == 0 and e[5, 3] == 0 and np.all(np.diag(e) == 0)
    assert f.shape == (12, 12) and np.isfinite(f).all()
    assert np.array_equal(f, f.T)
    lab = ora.dbscan(f, 10.0, 4)
    assert (lab == 0).all()
    lab = ora.dbscan(f, 1e-9, 4)
    assert (lab == -1).all()


def test_re_ranking_init_oracle_vs_reference_golden(golden, ora):
    """float32 cosine variant (rerank.py:171-234): tolerance based (np.dot / np.exp are not
    reproducible bit for bit across BLAS builds)."""
    g = golden("rerank_init.npz")
    for tag in ("a", "b"):
        out = ora.re_ranking_init(g["q_" + tag], g["g_" + tag], k1=int(g["k1_" + tag]), k2=int(g["k2_" + tag]), lambda_value=float(g["lam_" + tag]))
        ref = g["final_" + tag]
        assert out.shape == ref.shape and out.dtype == np.float32
        assert np.abs(out - ref).max() < 5e-6


def test_eval_oracle_matches_reference_golden(golden):
    """cmc / mean_ap restatement (oracle/eval_oracle.py) vs the values the reference functions produced
    (tools/make_golden.py eval_fixture): bitwise for mAP and the CMC curves."""
    from oracle import eval_oracle
    g = golden("eval_cases.npz")
    for tag in "abc":
        args = (g["dist_" + tag], g["qid_" + tag], g["gid_" + tag], g["qcam_" + tag], g["gcam_" + tag])
        assert eval_oracle.mean_ap(*args) == float(g["map_" + tag])
        assert np.array_equal(eval_oracle.cmc(*args, first_match_break=True), g["cmc_" + tag])
        assert np.array_equal(eval_oracle.cmc(*args), g["cmc_all_" + tag])
        first, ap = eval_oracle.per_query(*args)
        assert np.array_equal(first, g["first_" + tag]) and np.array_equal(np.isnan(ap), np.isnan(g["ap_" + tag]))
        mAP, scores, ret = eval_oracle.evaluate_all(*args)
        assert ret == g["cmc_" + tag][0]
    # a query whose only same-id gallery entries share its camera is skipped; none valid -> RuntimeError like the reference
    d = np.array([[0.1, 0.2, 0.3]], np.float32)
    with pytest.raises(RuntimeError):
        eval_oracle.mean_ap(d, [1], [1, 2, 3], [0], [0, 1, 1])


def test_rerank_plain_oracle_matches_reference_golden(golden):
    """kNN-set Jaccard variant (reid/rerank_plain.py:125-178): oracle restatement vs the reference's own output, bitwise."""
    from oracle import ssg_oracle as ora
    g = golden("rerank_plain.npz")
    for tag in "abc":
        final, final2, st = ora.re_ranking_plain(g["src_" + tag], g["tgt_" + tag], k=int(g["k_" + tag]), lambda_value=float(g["lam_" + tag]), stages=True)
        assert final is final2 and np.array_equal(final, g["final_" + tag])
        assert np.array_equal(st["knn"].sum(axis=1), g["setsize_" + tag])
        eps, _, _ = ora.eps_rule(final, float(g["rho_" + tag]))
        assert eps == float(g["eps_" + tag])
        assert np.array_equal(ora.dbscan(final, eps, 4), g["labels_" + tag])


def test_parallel_partition_model_matches_introsort(ora):
    """tools/introsort_model.py states the data-parallel form of numpy's Hoare partition that csrc/topk_intro.hip
    executes (stopper ranks instead of scanning pointers, only the ranges that reach the first K columns); it must
    give the first K entries of the sequential restatement (== np.argsort) on tie-heavy, sorted, reversed and
    adversarial (depth budget exhausted -> heapsort) keys."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "tools"))
    from introsort_model import argsort_topk
    from antiqsort import killer_keys
    rng = np.random.default_rng(5)
    for t in range(120):
        n = int(rng.integers(17, 2500))
        nv = int(rng.choice([1, 2, 3, 8, 50, 1000]))
        key = rng.integers(0, nv, n)
        if t % 4 == 1:
            key = np.sort(key)
        elif t % 4 == 2:
            key = np.sort(key)[::-1]
        key = key.astype(np.uint16)
        K = int(rng.integers(1, min(64, n) + 1))
        ref = np.argsort(key.view(np.float16))[:K]
        assert np.array_equal(ora.argsort_half(key.view(np.float16))[:K], ref)
        assert np.array_equal(argsort_topk(key, K), ref), (t, n, nv, K)
    for n in (100, 1000):
        key = killer_keys(n)
        ref = np.argsort(key.view(np.float16))[:64]
        assert np.array_equal(ora.argsort_half(key.view(np.float16))[:64], ref)
        assert np.array_equal(argsort_topk(key, 64), ref)


# ------------------------------------------------------------------ JPEG decode (the decode half of preprocessor.py:28)
def _random_jpeg(rng, h, w, kind, **kw):
    import io
    from PIL import Image
    if kind == 0:
        a = rng.integers(0, 256, (h, w, 3))
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([xx * 255.0 / max(w - 1, 1), yy * 255.0 / max(h - 1, 1), (xx + yy) * 127.0 / max(h + w - 2, 1)], -1) + rng.normal(0, 9, (h, w, 3))
    buf = io.BytesIO(); Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(buf, "JPEG", **kw)
    data = buf.getvalue()
    return data, np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def test_selftraining_fixture_oracle_and_host_join(golden, ora):
    """The fixture written by the reference's own compute_dist / generate_selflabel / generate_dataloader (selftraining.py:255-331,
    tools/make_golden.py selftraining_fixture): the oracle reproduces final_dist, eps (iteration 0) and the labels of both iterations
    (iteration 1 with the frozen eps), and the product's HOST-side join (ssg_amd.selftraining.generate_dataset, no GPU) rebuilds the
    dataset the reference handed to its Preprocessor."""
    import ssg_amd  # noqa: F401  (package alias)
    from ssg_amd.selftraining import generate_dataset
    g = golden("selftraining_ref.npz")
    N, S1, lam, rho = int(g["N"]), int(g["splits"]), float(g["lambda_value"]), float(g["rho"])
    trainval = [("img_%05d_c%d.jpg" % (i, i % 6), i // 16, i % 6) for i in range(N)]
    for it in range(2):
        labels = []
        for s in range(S1):
            _, f = ora.re_ranking(g["src_%d_%d" % (it, s)], g["tgt_%d_%d" % (it, s)], lambda_value=lam)
            assert hashlib.sha256(np.ascontiguousarray(f).tobytes()).hexdigest() == str(g["sha_final_%d_%d" % (it, s)]), (it, s)
            if it == 0:
                assert ora.eps_rule(f, rho)[0] == float(g["eps_%d" % s])
            lab = ora.dbscan(f, float(g["eps_%d" % s]), 4)
            assert np.array_equal(lab, g["labels_%d_%d" % (it, s)]), (it, s)
            labels.append(g["labels_%d_%d" % (it, s)])
        ds = generate_dataset(trainval, labels)
        assert [int(f[4:9]) for f, _, _ in ds] == g["kept_%d" % it].tolist() and all(c == 0 for _, _, c in ds)
        assert np.array_equal(np.array([[int(x) for x in lab] for _, lab, _ in ds], np.int64).reshape(len(ds), S1), g["kept_labels_%d" % it])
        assert 0 < len(ds) < N


def test_jpeg_oracle_vs_golden_and_pillow(golden):
    """oracle/jpeg_oracle.py (numpy restatement of libjpeg's default decompression) == the committed Pillow outputs, and == Pillow
    itself on freshly generated files (sizes that are not MCU multiples, all three chroma layouts, restart intervals)."""
    from oracle import jpeg_oracle
    g = golden("jpeg_cases.npz")
    for i in range(int(g["count"])):
        assert np.array_equal(jpeg_oracle.decode(g["file_%02d" % i].tobytes()), g["rgb_%02d" % i]), i
    with pytest.raises(jpeg_oracle.Unsupported):
        jpeg_oracle.decode(g["progressive_file"].tobytes())
    rng = np.random.default_rng(5)
    for h, w in ((16, 16), (23, 41), (9, 70)):
        for ss in (0, 1, 2):
            for extra in ({}, {"restart_marker_blocks": 2}, {"optimize": True}):
                data, ref = _random_jpeg(rng, h, w, int(rng.integers(0, 2)), quality=int(rng.integers(30, 96)), subsampling=ss, **extra)
                assert np.array_equal(jpeg_oracle.decode(data), ref), (h, w, ss, extra)


def test_jpeg_host_parser_matches_oracle(golden):
    """ssg_amd/jpeg.py's marker walk (product host code, no GPU needed) agrees with the oracle's independent parser on geometry,
    tables and the extent of the entropy-coded data; its derived Huffman tables decode every code of the file's DHT segments; files
    outside the supported class are refused (they go to Pillow in the product)."""
    from oracle import jpeg_oracle
    from ssg_amd import jpeg as pj
    g = golden("jpeg_cases.npz")
    for i in range(int(g["count"])):
        data = g["file_%02d" % i].tobytes()
        h = pj.scan_header(data); o = jpeg_oracle.parse(data)
        assert (h.width, h.height, h.ri) == (o["width"], o["height"], o["restart_interval"])
        assert [tuple(c) for c in h.comps] == [tuple(c) for c in o["comps"]] and h.scan == o["scan"]
        assert data[h.ecs_start:h.ecs_end] == o["ecs"]
        for tid, q in h.qt.items():
            assert np.array_equal(q.astype(np.int32), o["qt"][tid])
        for spec in list(h.dc.values()) + list(h.ac.values()):
            look, maxcode, valoff, vals = pj._derived(spec[0], spec[1])
            code, p = 0, 0
            for length in range(1, 17):
                for _ in range(spec[0][length - 1]):
                    if length <= 8:
                        assert look[code << (8 - length)] == ((length << 8) | spec[1][p])
                    assert code <= maxcode[length] and vals[code + valoff[length]] == spec[1][p]
                    code += 1; p += 1
                code <<= 1
    for bad in (g["progressive_file"].tobytes(), b"\x89PNG\r\n\x1a\n" + bytes(32), b""):
        with pytest.raises(pj.NotBaseline):
            pj.scan_header(bad)


def test_jpeg_native_parser_matches_python(golden):
    """csrc/jpeg_host.hip (ssg_jpeg_parse_open / _fill / _close: the threaded native marker walk the product uses) against the Python
    statement of the same bookkeeping (ssg_amd.jpeg.parse_batch_python), field by field -- which files go to the GPU, geometry,
    block / plane / output offsets, restart segments, the entropy-coded pool, derived Huffman tables, quantisation tables -- on the
    committed files, on every 3rd truncation of one of them and on 2000 files with random byte damage in their headers (both must
    hand exactly the same files to Pillow).  Host code only: no GPU."""
    from ssg_amd import jpeg as pj
    g = golden("jpeg_cases.npz")
    files = [g["file_%02d" % i].tobytes() for i in range(int(g["count"]))] + [g["progressive_file"].tobytes(), b"", b"\x89PNG\r\n\x1a\n" + bytes(32)]

    def same(a, b):
        assert a.kept == b.kept and a.fallback == b.fallback and a.dims == b.dims
        if not a.kept:
            return
        for k in ("imgs", "segs", "pool", "look", "maxcode", "valoff", "vals", "qts"):
            x, y = getattr(a, k), getattr(b, k)
            assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), k
        for k in ("blocks", "max_blocks", "plane_bytes", "out_bytes", "max_pixels"):
            assert getattr(a, k) == getattr(b, k), k
    same(pj._parse_batch_native(files), pj.parse_batch_python(files))
    same(pj._parse_batch_native(files, threads=1), pj._parse_batch_native(files, threads=7))
    rng = np.random.default_rng(0)
    cases = [files[0][:c] for c in range(0, len(files[0]), 3)]
    for _ in range(2000):
        f = bytearray(files[int(rng.integers(0, len(files) - 3))])
        for q in rng.integers(2, min(len(f), 700), int(rng.integers(1, 4))):
            f[int(q)] = int(rng.integers(0, 256))
        cases.append(bytes(f))
    nat = pj._parse_batch_native(cases, threads=4)
    same(nat, pj.parse_batch_python(cases))
    assert len(nat.fallback) > 100 and len(nat.kept) > 100
    assert pj._parse_batch_native([]).kept == []


def test_jpeg_kernel_text_executed_on_host_matches_pillow(golden):
    """The three kernels of csrc/jpeg.hip use no wave-level operation, so their SOURCE TEXT -- cut from the file, `__global__` /
    `__device__` mapped to host functions (tools/fuzz/jpeg_device_fuzz.cpp, the libFuzzer harness built as a plain decoder, with ASan)
    -- runs thread by thread on the CPU: native parser -> Huffman -> IDCT -> colour on exactly-sized buffers must give Pillow's bytes
    for the committed files and for fresh ones (all chroma layouts, odd sizes, restart intervals, optimised tables); progressive files
    are refused by the parser (exit 3).  A CPU-side pin of the device code; the `-m gpu` tests run the same text on the GPU."""
    import jpeg_cases_ref as jc                  # (the build of the host decoder is shared with tests/test_jpeg_damage_host.py)
    if jc.host_decoder() is None:
        pytest.skip("ROCm clang++ not present")
    run = jc.run_host                            # asserts exit code 0 / 3 / 4: anything else = a sanitizer report

    g = golden("jpeg_cases.npz")
    for i in range(int(g["count"])):
        rc, px = run(g["file_%02d" % i].tobytes())
        assert rc == 0 and np.array_equal(px.reshape(g["rgb_%02d" % i].shape), g["rgb_%02d" % i]), i
    assert run(g["progressive_file"].tobytes())[0] == 3
    rng = np.random.default_rng(11)
    for h, w in ((16, 16), (23, 41), (9, 70), (128, 64)):
        for ss in (0, 1, 2):
            for extra in ({}, {"restart_marker_blocks": 2}, {"optimize": True}):
                data, ref = _random_jpeg(rng, h, w, int(rng.integers(0, 2)), quality=int(rng.integers(30, 96)), subsampling=ss, **extra)
                rc, px = run(data)
                assert rc == 0 and np.array_equal(px.reshape(ref.shape), ref), (h, w, ss, extra)
    # damaged entropy-coded data: decoded without a sanitizer report; a short segment is flagged (exit 4) like on the GPU
    data, _ = _random_jpeg(rng, 64, 48, 1, quality=80)
    assert run(data[:len(data) // 2] + b"\xff\xd9")[0] in (3, 4)


def test_jpeg_host_parser_hands_malformed_files_to_pillow(golden):
    """a short / odd marker segment must never abort the batch with IndexError / struct.error -- every truncation and a set of
    corrupted headers either parses (damage inside the entropy-coded data is caught on the device) or raises NotBaseline (-> Pillow);
    3-component files whose ids spell 'RGB' without a JFIF / Adobe marker are RGB for libjpeg (no colour transform): refused too."""
    from ssg_amd import jpeg as pj
    g = golden("jpeg_cases.npz")
    data = g["file_00"].tobytes()
    hdr = pj.scan_header(data)
    for cut in list(range(0, hdr.ecs_start + 4)) + list(range(hdr.ecs_start + 4, len(data), 97)):
        try:
            pj.scan_header(data[:cut])
        except pj.NotBaseline:
            pass
    rng = np.random.default_rng(3)
    for _ in range(300):                       # random byte damage inside the header region
        b = bytearray(data)
        for q in rng.integers(2, hdr.ecs_start, int(rng.integers(1, 4))):
            b[int(q)] = int(rng.integers(0, 256))
        try:
            pj.scan_header(bytes(b))
        except pj.NotBaseline:
            pass
    # a DC table with a category > 15 is JERR_BAD_HUFF_TABLE in libjpeg
    q = data.index(b"\xff\xc4")
    b = bytearray(data); b[q + 4 + 17] = 200
    assert (b[q + 4] >> 4) == 0
    with pytest.raises(pj.NotBaseline):
        pj.scan_header(bytes(b))
    # component ids R, G, B and no JFIF / Adobe marker
    q = data.index(b"\xff\xc0")
    b = bytearray(data)
    assert b[q + 9] == 3
    b[q + 10], b[q + 13], b[q + 16] = 82, 71, 66
    s = data.index(b"\xff\xda"); b[s + 5], b[s + 7], b[s + 9] = 82, 71, 66
    j = data.index(b"\xff\xe0"); b[j + 4:j + 8] = b"XXXX"
    with pytest.raises(pj.NotBaseline):
        pj.scan_header(bytes(b))
    b[j + 4:j + 8] = b"JFIF"                   # with the JFIF marker the ids do not matter: YCbCr
    pj.scan_header(bytes(b))
