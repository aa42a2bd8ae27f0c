"""GPU half of the embedder-refresh tests: csrc/fold.hip (ssg_fold_conv_bn_f32, ssg_fold_conv_bn_dual_f32) and `ResNet.refresh` against
the host route -- `_fold` / `ResNet._prepare` of ssg_amd/resnet.py with every tensor on the CPU, the code of the parent commit.  The fold
is deterministic element-wise arithmetic, so every comparison is torch.equal on the int32 view of the outputs: no tolerance anywhere.
"""
import functools
import types
import warnings

import pytest
import torch

import fold_ref
import ssg_amd
from ssg_amd import _lib, resnet
from ssg_amd._lib import ptr, stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PATTERN = -7.25                                   # what the outputs hold before a call


def _i32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(got, ref, what):
    assert (got is None) == (ref is None), what
    if ref is not None:
        assert tuple(got.shape) == tuple(ref.shape) and got.dtype == ref.dtype, what
        assert torch.equal(_i32(got), _i32(ref)), what


# ------------------------------------------------------------------ 1. one layer at a time, through the C ABI
LAYERS = {"stem": (64, 3, 7, 7),                  # h4l4 layout, Kpad = 224, the zero tail
          "one_chunk": (64, 32, 1, 1),            # a single 32-channel chunk
          "chunk_major": (64, 64, 3, 3),          # two chunks: the chunk-major order is visible
          "longest_row": (64, 512, 3, 3),         # K = 4608
          "linear": (64, 512, 1, 1)}              # feat + feat_bn: the [N, K] Linear weight with BatchNorm1d statistics
DUALS = {"dual_equal": (256, 64, 64), "dual_unequal": (128, 32, 64)}


@functools.lru_cache(maxsize=None)
def _layer_case(name):
    return fold_ref.crafted(*LAYERS[name], seed=100 + sorted(LAYERS).index(name))


@functools.lru_cache(maxsize=None)
def _layer_ref(name, split):
    return fold_ref.host_fold(_layer_case(name), split)


@functools.lru_cache(maxsize=None)
def _dual_case(name):
    cout, c1, c2 = DUALS[name]
    i = sorted(DUALS).index(name)
    return fold_ref.crafted(cout, c1, 1, 1, seed=200 + i), fold_ref.crafted(cout, c2, 1, 1, seed=300 + i, quiet_head=True)


@functools.lru_cache(maxsize=None)
def _dual_ref(name, split):
    return fold_ref.host_fold_dual(*_dual_case(name), split)


def _source_args(case, channels_last):
    """the argument run of one source: weight pointer, four strides, then (for the caller to place) the shape and the statistics"""
    w = case["w"].to(DEV)
    if channels_last:
        w = w.contiguous(memory_format=torch.channels_last)
    keep = [w] + [case[k].to(DEV) for k in ("gamma", "beta", "mean", "var")]
    return keep, list(w.stride())


def _outputs(cout, kp):
    return (torch.full((cout, kp), PATTERN, device=DEV), torch.full((cout,), PATTERN, device=DEV), torch.full((cout,), PATTERN, device=DEV))


def _call_single(case, split, channels_last, linear_2d=False):
    L = _lib.lib()
    cout, cin, kh, kw = case["w"].shape
    keep, st = _source_args(case, channels_last)
    if linear_2d:                                 # nn.Linear's own [N, K] weight, read where it lies
        keep[0] = case["w"].view(cout, cin).to(DEV)
        st = [cin, 1, 1, 1]
    kp = 32 * ((kh * kw + 7) // 8) if cin == 3 else cin * kh * kw
    w_out, bias, cs = _outputs(cout, kp)
    rc = L.ssg_fold_conv_bn_f32(ptr(keep[0]), st[0], st[1], st[2], st[3], cout, cin, kh, kw, ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]),
                                fold_ref.EPS, 1 if split else 0, ptr(w_out), ptr(bias), ptr(cs), stream())
    torch.cuda.synchronize()
    return rc, w_out, bias, cs


def _call_dual(case1, case2, split, channels_last):
    L = _lib.lib()
    cout = case1["w"].shape[0]
    args, keep = [], []
    for case in (case1, case2):
        k, st = _source_args(case, channels_last)
        keep.append(k)
        _, cin, kh, kw = case["w"].shape
        args += [ptr(k[0]), st[0], st[1], st[2], st[3], cin, kh, kw, ptr(k[1]), ptr(k[2]), ptr(k[3]), ptr(k[4])]
    kp = sum(c["w"].shape[1] * c["w"].shape[2] * c["w"].shape[3] for c in (case1, case2))
    w_out, bias, cs = _outputs(cout, kp)
    rc = L.ssg_fold_conv_bn_dual_f32(*args, fold_ref.EPS, cout, 1 if split else 0, ptr(w_out), ptr(bias), ptr(cs), stream())
    torch.cuda.synchronize()
    return rc, w_out, bias, cs


def _check_outputs(got, ref, split, what):
    rc, w_out, bias, cs = got
    assert rc == 0, (what, _lib.lib().ssg_last_error())
    _same(bias, ref[1], what + " bias")
    _same(w_out, ref[0], what + " w")
    if split:
        _same(cs, ref[2], what + " ch_scale")
    else:
        assert ref[2] is None and bool((cs == PATTERN).all()), what + ": f32 mode must not touch ch_scale"


@pytest.mark.parametrize("channels_last", (False, True))
@pytest.mark.parametrize("split", (False, True))
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_layer_fold_is_the_host_fold(name, split, channels_last):
    """ssg_fold_conv_bn_f32 == `_fold`, bit for bit, on the crafted rows (row maxima 2^j +- one ulp, an all-zero row, gamma = 1e-12 / 1e6 /
    negative, running_var = 0, subnormal and zero lo halves) and on random rows"""
    got = _call_single(_layer_case(name), split, channels_last)
    _check_outputs(got, _layer_ref(name, split), split, "%s split=%s channels_last=%s" % (name, split, channels_last))


@pytest.mark.parametrize("split", (False, True))
def test_linear_weight_is_read_where_it_lies(split):
    """the feat + feat_bn fold: the 2-D [N, K] weight with strides (K, 1, 1, 1)"""
    got = _call_single(_layer_case("linear"), split, False, linear_2d=True)
    _check_outputs(got, _layer_ref("linear", split), split, "linear 2-D split=%s" % split)


@pytest.mark.parametrize("channels_last", (False, True))
@pytest.mark.parametrize("split", (False, True))
@pytest.mark.parametrize("name", sorted(DUALS))
def test_dual_fold_is_the_host_concatenation(name, split, channels_last):
    """ssg_fold_conv_bn_dual_f32 == two host folds concatenated along K, one row scale over the concatenated row, biases added in float32"""
    got = _call_dual(*_dual_case(name), split, channels_last)
    _check_outputs(got, _dual_ref(name, split), split, "%s split=%s channels_last=%s" % (name, split, channels_last))


def test_dual_row_scale_spans_both_sources():
    """the maximum of the concatenated row may sit in the second source: exchanged sources give the host's bits too"""
    c1, c2 = _dual_case("dual_unequal")
    got = _call_dual(c2, c1, True, False)
    _check_outputs(got, fold_ref.host_fold_dual(c2, c1, True), True, "dual exchanged")


def _plain(cout, cin, k, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(w=torch.randn(cout, cin, k, k, generator=g), gamma=torch.rand(cout, generator=g) + 0.5, beta=torch.randn(cout, generator=g),
                mean=torch.randn(cout, generator=g), var=torch.rand(cout, generator=g) + 0.5)


def test_refusals_leave_the_outputs_untouched():
    L = _lib.lib()
    for what, call, fn in (("Cin = 48", lambda: _call_single(_plain(64, 48, 1, 1), True, False), b"ssg_fold_conv_bn_f32"),
                           ("Cout = 96", lambda: _call_single(_plain(96, 64, 1, 2), True, False), b"ssg_fold_conv_bn_f32"),
                           ("3x3 second source", lambda: _call_dual(_plain(64, 64, 1, 3), _plain(64, 64, 3, 4), True, False), b"ssg_fold_conv_bn_dual_f32")):
        rc, w_out, bias, cs = call()
        assert rc == -1, what
        msg = L.ssg_last_error()
        assert fn in msg and b"unsupported shape" in msg, (what, msg)
        for t in (w_out, bias, cs):
            assert bool((t == PATTERN).all()), what
    assert L.ssg_fold_max_k() >= 4608


# ------------------------------------------------------------------ 2. the whole model: refresh against load_state_dict
_FIELDS = ("cin", "cout", "k", "stride", "pad", "split", "acc_scale")


def _same_conv(a, b, what):
    assert (a is None) == (b is None), what
    if a is None:
        return
    for f in _FIELDS:
        assert getattr(a, f) == getattr(b, f) and type(getattr(a, f)) is type(getattr(b, f)), (what, f, getattr(a, f), getattr(b, f))
    for f in ("w", "bias", "cscale"):
        _same(getattr(a, f), getattr(b, f), "%s.%s" % (what, f))
        if getattr(a, f) is not None:
            assert getattr(a, f).device == getattr(b, f).device, (what, f)


def _same_folded(a, b, need_feat=False):
    """two `_folded` nets: same structure, same bits; the lazily folded feat is compared where both have it (need_feat: both must)"""
    lazy = {"feat", "centers"}
    assert sorted(set(a) - lazy) == sorted(set(b) - lazy) and a["split"] == b["split"] and len(a["blocks"]) == len(b["blocks"])
    _same_conv(a["stem"], b["stem"], "stem")
    for i, (x, y) in enumerate(zip(a["blocks"], b["blocks"])):
        assert sorted(x) == sorted(y) and x.get("kind") == y.get("kind"), i
        for key in x:
            if key != "kind":
                _same_conv(x[key], y[key], "block %d %s" % (i, key))
    assert not need_feat or ("feat" in a and "feat" in b)
    if "feat" in a and "feat" in b:
        _same_conv(a["feat"], b["feat"], "feat")


def _build_feat(m):
    m._x2(torch.zeros(1, m.out_planes, device=DEV))              # the feat + feat_bn fold is built on first use


@functools.lru_cache(maxsize=None)
def _pair(depth, precision):
    """(host embedder through load_state_dict, device embedder through refresh of the same tensors placed on the GPU, the tensors)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sd = ssg_amd.synthetic_state_dict(seed=5, depth=depth)
        host = resnet.ResNet(depth, pretrained=False, precision=precision).cuda().eval()
        host.load_state_dict(sd)
        host._prepare(); _build_feat(host)
        dev = resnet.ResNet(depth, pretrained=False, precision=precision, seed=2).cuda().eval()
        dev.refresh({k: v.to(DEV) for k, v in sd.items()}, strict=True)
        assert dev._folded is not None and "feat" not in dev._folded      # rebuilt by refresh itself; feat stays lazy
        _build_feat(dev)
    torch.cuda.synchronize()
    return host, dev, sd


IMAGES = torch.randn(2, 3, 256, 128, generator=torch.Generator().manual_seed(3))


@pytest.mark.parametrize("precision", ("split", "f32"))
@pytest.mark.parametrize("depth", (18, 50))
def test_refresh_builds_what_load_state_dict_builds(depth, precision):
    """every tensor and every scalar field of every folded convolution, the lazily folded feat included, then the embedding itself"""
    host, dev, sd = _pair(depth, precision)
    assert all(v.device.type == "cpu" for v in host._sd.values()) and all(v.device == DEV for v in dev._sd.values())
    assert dev._weights == "loaded" and dev._twin is None
    _same_folded(host._folded, dev._folded, need_feat=True)
    a, b = host.embed_with_flip(IMAGES), dev.embed_with_flip(IMAGES)
    _same(b, a, "embed_with_flip")
    x1a, x2a = host(IMAGES)
    x1b, x2b = dev(IMAGES)
    _same(x1b, x1a, "x1"); _same(x2b, x2a, "x2")


def test_fp32_twin_follows_the_device_entries():
    """the fp32 twin shares `_sd`, so after a refresh it folds on the device and gives the host twin's bits"""
    host, dev, _ = _pair(18, "split")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        th, td = host._f32_twin(), dev._f32_twin()
    try:
        assert td._sd is dev._sd
        _same_folded(th._prepare(), td._prepare())
    finally:
        host._twin = dev._twin = None


# ------------------------------------------------------------------ 3. refresh from a module
def module_tree(sd, device):
    """a bare nn.Module tree with the reference's key names: parameters and buffers set by key path, 4-D weights in channels_last"""
    root = torch.nn.Module()
    for key, v in sd.items():
        *path, leaf = key.split(".")
        m = root
        for name in path:
            if name not in m._modules:
                m.add_module(name, torch.nn.Module())
            m = m._modules[name]
        t = v.clone().to(device)
        if t.dim() == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        if leaf.startswith("running_") or leaf == "num_batches_tracked":
            m.register_buffer(leaf, t)
        else:
            m.register_parameter(leaf, torch.nn.Parameter(t))
    return root


@functools.lru_cache(maxsize=None)
def _module18():
    _, _, sd = _pair(18, "split")
    return module_tree(sd, DEV)


def test_refresh_from_a_wrapped_channels_last_module_takes_a_snapshot():
    host, _, sd = _pair(18, "split")
    tree = module_tree(sd, DEV)
    assert sorted(tree.state_dict()) == sorted(sd) and tree.state_dict()["base.layer1.0.conv1.weight"].stride()[1] == 1      # channels_last
    m = resnet.ResNet(18, pretrained=False, seed=9).cuda().eval()
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # every key is there: no warning
        missing, unexpected = m.refresh(types.SimpleNamespace(module=tree))
    assert missing == [] and unexpected == []
    _build_feat(m)
    before = m.embed_with_flip(IMAGES)
    with torch.no_grad():                                        # the optimiser's in-place steps on the source, after the refresh
        for p in tree.parameters():
            p.mul_(0.5).add_(1.0)
        for b in tree.buffers():
            if b.dtype.is_floating_point:
                b.add_(3.0)
    torch.cuda.synchronize()
    _same(m.embed_with_flip(IMAGES), before, "features after the source changed")
    _same(before, host.embed_with_flip(IMAGES), "features of the refreshed weights")
    m._invalidate()                                              # a rebuild folds the snapshot again, not the source
    m._prepare(); _build_feat(m)
    _same_folded(host._folded, m._folded, need_feat=True)
    out = m.state_dict()
    assert list(out) == list(sd)
    for k, v in out.items():
        assert v.device.type == "cpu" and v.dtype == sd[k].dtype and torch.equal(v, sd[k]), k
    # load_state_dict afterwards puts what it is given back on the CPU
    m.load_state_dict(sd)
    assert all(v.device.type == "cpu" for v in m._sd.values())
    _same_folded(host._folded, m._prepare())


def test_refresh_refusals_change_nothing():
    _, _, sd = _pair(18, "split")
    m = resnet.ResNet(18, pretrained=False, seed=9).cuda().eval()
    gpu = {k: v.to(DEV) for k, v in sd.items()}
    m.refresh(gpu, strict=True)
    folded, entries = m._folded, dict(m._sd)
    bad = dict(gpu)
    bad["base.layer4.1.conv2.weight"] = torch.zeros(512, 512, 1, 1, device=DEV)      # late in the dict: everything before it matches
    with pytest.raises(RuntimeError, match="size mismatch"):
        m.refresh(bad)
    assert m._folded is folded and list(m._sd) == list(entries) and all(m._sd[k] is entries[k] for k in entries)
    short = {k: v for k, v in gpu.items() if k != "base.layer2.0.bn1.weight"}
    with pytest.raises(RuntimeError, match="missing"):
        m.refresh(short, strict=True)
    assert m._folded is folded and all(m._sd[k] is entries[k] for k in entries)
    with pytest.warns(UserWarning, match="refresh: 1 backbone tensors"):
        missing, unexpected = m.refresh({"module." + k: v for k, v in short.items()})            # DataParallel's prefix, strict=False
    assert missing == ["base.layer2.0.bn1.weight"] and unexpected == [] and m._weights == "loaded"
    assert m._sd["base.layer2.0.bn1.weight"] is entries["base.layer2.0.bn1.weight"] and m._sd["base.conv1.weight"] is not entries["base.conv1.weight"]
    m.refresh({"state_dict": gpu, "epoch": 3}, strict=True)                                       # the checkpoint wrapper
    cpu_model = resnet.ResNet(18, pretrained=False)
    with pytest.raises(_lib.SSGError):
        cpu_model.refresh(gpu)


def test_mixed_residency_and_the_env_switch(monkeypatch):
    """SSG_DEVICE_FOLD=0 after a refresh and SSG_DEVICE_FOLD=1 after a plain load_state_dict each rebuild the same bits; entries that
    arrive on the CPU are moved, and a partial load_state_dict after a refresh leaves a mixed `_sd` that still folds to the same bits"""
    host, _, sd = _pair(18, "split")
    m = resnet.ResNet(18, pretrained=False, seed=9).cuda().eval()
    m.refresh(sd, strict=True)                                   # CPU tensors: moved to the device
    assert all(v.device == DEV for v in m._sd.values())
    _same_folded(host._folded, m._folded)
    monkeypatch.setenv("SSG_DEVICE_FOLD", "0")                   # the host fold of device entries
    m._invalidate()
    m._prepare(); _build_feat(m)
    _same_folded(host._folded, m._folded, need_feat=True)
    assert all(v.device == DEV for v in m._sd.values())
    monkeypatch.setenv("SSG_DEVICE_FOLD", "1")                   # the device fold of CPU entries
    c = resnet.ResNet(18, pretrained=False, seed=9).cuda().eval()
    c.load_state_dict(sd)
    c._prepare(); _build_feat(c)
    assert all(v.device.type == "cpu" for v in c._sd.values())
    _same_folded(host._folded, c._folded, need_feat=True)
    monkeypatch.delenv("SSG_DEVICE_FOLD")
    m.load_state_dict({k: v for k, v in sd.items() if k.startswith("base.layer3.")}, strict=False)
    assert {v.device.type for v in m._sd.values()} == {"cpu", "cuda"}
    m._prepare(); _build_feat(m)
    _same_folded(host._folded, m._folded, need_feat=True)


# ------------------------------------------------------------------ 4. no host synchronisation
def test_refresh_does_not_synchronise():
    tree = _module18()
    m = resnet.ResNet(18, pretrained=False, seed=9).cuda().eval()
    m.refresh(tree)                                              # warm-up: library load, allocator
    torch.cuda.synchronize()
    control_raised = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=DEV).item()
        except RuntimeError:
            control_raised = True
        if control_raised:
            m.refresh(tree)
            m.refresh(types.SimpleNamespace(module=tree), strict=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    if not control_raised:
        pytest.skip("this torch build does not raise on .item() under set_sync_debug_mode('error')")
    host, _, _ = _pair(18, "split")
    _same_folded(host._folded, m._folded)
