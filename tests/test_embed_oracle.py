"""CPU suite: the torch-fp32 restatement of the embedding path against the golden features
produced by the real reference model (tools/make_golden.py, tests/golden/embed_ref.npz)."""
import numpy as np
import torch


def test_embed_restatement_matches_reference_golden(golden):
    import ssg_amd
    from oracle import embed_oracle
    g = golden("embed_ref.npz")
    sd = ssg_amd.synthetic_state_dict(seed=int(g["weight_seed"]))
    imgs = torch.randn(4, 3, 256, 128, generator=torch.Generator().manual_seed(int(g["image_seed"])))
    for S in (2, 1):
        mine = torch.stack(embed_oracle.embed_with_flip(sd, imgs[:2], S)).numpy()
        ref = g["feats_S%d" % S][:, :2]
        assert mine.shape == ref.shape
        # same machine/threads -> identical; other hosts may pick other oneDNN kernels
        assert np.abs(mine - ref).max() < 2e-6
        assert np.allclose(np.linalg.norm(mine, axis=2), 1.0, atol=1e-5)


def test_embed_restatement_matches_the_wide_reference_goldens(golden):
    """round 5: the 16-image fixture and the checkpoint-like-BatchNorm fixture, both written by the REAL reference model
    (tools/make_golden.py --only-embed-wide); the restatement is checked on the first two images of each (CPU time)."""
    import ssg_amd
    from oracle import embed_oracle
    from synth import checkpoint_like_state_dict
    for fname, mk in (("embed_ref16.npz", lambda s: ssg_amd.synthetic_state_dict(seed=s)), ("embed_ckpt_ref.npz", checkpoint_like_state_dict)):
        g = golden(fname)
        n = int(g["n"])
        sd = mk(int(g["weight_seed"]))
        imgs = torch.randn(n, 3, 256, 128, generator=torch.Generator().manual_seed(int(g["image_seed"])))
        mine = torch.stack(embed_oracle.embed_with_flip(sd, imgs[:2], 2)).numpy()
        ref = g["feats_S2"]
        assert ref.shape == (3, n, 2048) and np.allclose(np.linalg.norm(ref, axis=2), 1.0, atol=1e-5)
        assert np.abs(mine - ref[:, :2]).max() < 2e-6, fname
    sd = checkpoint_like_state_dict(7)
    sc = (sd["base.layer2.0.bn2.weight"] / torch.sqrt(sd["base.layer2.0.bn2.running_var"] + 1e-5)).abs()
    assert float(sc.max() / sc.min()) > 1e3          # the point of the second fixture: per-channel scales spanning decades


def test_state_dict_surface():
    import ssg_amd
    m = ssg_amd.create("resnet50", num_classes=0, num_split=2, cluster=False)
    sd = m.state_dict()
    assert "base.conv1.weight" in sd and "base.layer4.2.bn3.running_var" in sd and "feat.weight" in sd and "feat_bn.running_mean" in sd
    assert sd["base.layer2.0.downsample.0.weight"].shape == (512, 256, 1, 1)
    conv_params = sum(v.numel() for k, v in sd.items() if k.endswith("weight") and v.dim() == 4)
    assert conv_params == 23454912          # 23.5 M conv parameters
    sd2 = {k: v for k, v in sd.items() if not k.startswith("base.fc")}
    missing, unexpected = m.load_state_dict(sd2, strict=False)
    assert set(missing) == {"base.fc.weight", "base.fc.bias"} and not unexpected
    try:
        m(torch.zeros(1, 3, 256, 128))
        assert False, "CPU forward must not silently work"
    except ssg_amd.SSGError:
        pass


def test_float64_restatement_matches_reference_golden_and_float32_path(golden):
    """dtype=torch.float64 is the reference the kernel tests (test_gpu_fused_blocks.py, test_gpu_embed_batch.py) judge the HIP path
    by: it is pinned here against the features the REAL reference model wrote (embed_ref.npz, synthetic weights; embed_ckpt_ref.npz,
    checkpoint-like BatchNorm statistics) inside the 5e-6 every golden test uses, and against the float32 path to the same bound."""
    import ssg_amd
    from oracle import embed_oracle
    from synth import checkpoint_like_state_dict
    for fname, mk, n_all in (("embed_ref.npz", lambda s: ssg_amd.synthetic_state_dict(seed=s), 4), ("embed_ckpt_ref.npz", checkpoint_like_state_dict, None)):
        g = golden(fname)
        n = n_all or int(g["n"])
        sd = mk(int(g["weight_seed"]))
        imgs = torch.randn(n, 3, 256, 128, generator=torch.Generator().manual_seed(int(g["image_seed"])))[:2]
        f64 = torch.stack(embed_oracle.embed_with_flip(sd, imgs, 2, dtype=torch.float64))
        f32 = torch.stack(embed_oracle.embed_with_flip(sd, imgs, 2))
        assert f64.dtype == torch.float64 and f32.dtype == torch.float32 and f64.shape == f32.shape
        ref = torch.from_numpy(g["feats_S2"][:, :2]).double()
        e_gold, e_32 = float((f64 - ref).abs().max()), float((f64 - f32.double()).abs().max())
        print("%s: |f64 - golden| %.3g  |f64 - f32| %.3g" % (fname, e_gold, e_32))
        assert e_gold < 5e-6 and e_32 < 5e-6, (fname, e_gold, e_32)
        assert np.allclose(np.linalg.norm(f64.numpy(), axis=2), 1.0, atol=1e-12)
        # the layer4 map itself, relative to its largest value (the unit-norm features hide a common factor)
        m64 = embed_oracle.feature_map(sd, imgs[:1], dtype=torch.float64)
        m32 = embed_oracle.feature_map({k: v.float() for k, v in sd.items() if v.dtype.is_floating_point}, imgs[:1])
        rel = float((m64 - m32.double()).abs().max() / m64.abs().max())
        print("%s: layer4 map, float32 against float64: %.3g of its maximum" % (fname, rel))
        assert m64.dtype == torch.float64 and rel < 5e-5     # 10 x the 1.8e-6 measured: only says the two dtypes run the same network


def test_block_restatements_are_the_feature_maps_own_statements():
    """embed_oracle.stem / bottleneck (what the fused-kernel tests compare with) compose to feature_map's first stages exactly."""
    import ssg_amd
    from oracle import embed_oracle
    sd = {k: v.double() for k, v in ssg_amd.synthetic_state_dict(seed=2).items() if v.dtype.is_floating_point}
    bn = lambda p: tuple(sd[p + s] for s in (".weight", ".bias", ".running_mean", ".running_var"))      # noqa: E731
    x = torch.randn(1, 3, 32, 128, generator=torch.Generator().manual_seed(5)).double()
    for flip in (False, True):
        y = embed_oracle.stem(x, sd["base.conv1.weight"], bn("base.bn1"), flip=flip)
        xin = embed_oracle.fliplr(x) if flip else x
        want = torch.nn.functional.max_pool2d(torch.relu(embed_oracle._bn(torch.nn.functional.conv2d(xin, sd["base.conv1.weight"], None, 2, 3), sd, "base.bn1")), 3, 2, 1)
        assert y.shape == (1, 64, 8, 32) and torch.equal(y, want)
    for b in (0, 1):
        p = "base.layer1.%d" % b
        ds = (sd[p + ".downsample.0.weight"], bn(p + ".downsample.1")) if b == 0 else None
        y = embed_oracle.bottleneck(y, [sd[p + ".conv%d.weight" % i] for i in (1, 2, 3)], [bn(p + ".bn%d" % i) for i in (1, 2, 3)], ds)
    # layer1.0 and layer1.1 of the flipped image, restated from feature_map's own lines
    z = want
    for b in (0, 1):
        p = "base.layer1.%d" % b
        o = torch.relu(embed_oracle._bn(torch.nn.functional.conv2d(z, sd[p + ".conv1.weight"]), sd, p + ".bn1"))
        o = torch.relu(embed_oracle._bn(torch.nn.functional.conv2d(o, sd[p + ".conv2.weight"], None, 1, 1), sd, p + ".bn2"))
        o = embed_oracle._bn(torch.nn.functional.conv2d(o, sd[p + ".conv3.weight"]), sd, p + ".bn3")
        r = embed_oracle._bn(torch.nn.functional.conv2d(z, sd[p + ".downsample.0.weight"]), sd, p + ".downsample.1") if b == 0 else z
        z = torch.relu(o + r)
    assert torch.equal(y, z)
