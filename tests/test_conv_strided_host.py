"""Host half of the strided train-mode Conv2d / max-pool tests (no GPU): the slice cut of the strided weight gradient, the argument
checks that come before any launch, the class rules of the Python layer, and use_device_conv(strided=True) / use_device_maxpool on a
hand-built model."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_strided_ref as ref  # noqa: E402
import train_common as tc  # noqa: E402
from test_conv_train_host import _model  # noqa: E402


@pytest.fixture(scope="module")
def L():
    from ssg_amd import _lib
    return _lib.lib()


def test_new_names_resolve():
    import ssg_amd
    for n in ("conv2d_train_strided", "StridedConv2d", "max_pool2d_train", "MaxPool2d", "use_device_maxpool"):
        assert callable(getattr(ssg_amd, n)), n
    assert issubclass(ssg_amd.StridedConv2d, torch.nn.Conv2d) and issubclass(ssg_amd.MaxPool2d, torch.nn.MaxPool2d)


# (M = B*OH*OW, Cout, KH, KW, Cin): the seven strided convolutions of ResNet-50 at B = 128, 256 x 128, and the small cases
SHAPES = [(128 * 128 * 64, 64, 7, 7, 3), (128 * 32 * 16, 128, 3, 3, 128), (128 * 16 * 8, 256, 3, 3, 256), (128 * 8 * 4, 512, 3, 3, 512),
          (128 * 32 * 16, 512, 1, 1, 256), (128 * 16 * 8, 1024, 1, 1, 512), (128 * 8 * 4, 2048, 1, 1, 1024), (12, 64, 1, 1, 64), (1, 64, 3, 3, 64),
          (15, 64, 7, 7, 3)]


def test_strided_wgrad_slices_and_workspace(L):
    for (M, cout, kh, kw, cin) in SHAPES:
        n = L.ssg_conv_wgrad_strided_num_slices(M, cout, kh, kw, cin, 2)
        assert n >= 1 and n == L.ssg_conv_wgrad_strided_num_slices(M, cout, kh, kw, cin, 2)        # a function of the shape alone
        row = 13 * 64 if kh == 7 else kh * kw * cin                                                  # the stem: 13 K tiles of 16 taps x RGB0
        assert L.ssg_conv_wgrad_strided_workspace_bytes(M, cout, kh, kw, cin, 2) == 4 * n * cout * row
        assert n <= (M + 31) // 32                                                                   # no slice without a pixel
    assert L.ssg_conv_wgrad_strided_num_slices(15, 64, 7, 7, 3, 2) == 1
    assert L.ssg_conv_wgrad_strided_num_slices(128 * 128 * 64, 64, 7, 7, 3, 2) >= 64                 # the stem at B = 128 is cut into many
    # the GPU suite's multi-slice cases exist: some B <= 64 gives three slices with a ragged last one
    for (H, W, cin, cout, k, _) in ref.MULTI.values():
        B = ref.multi_slice_batch(L, H, W, cin, cout, k)
        assert B is not None and B <= 64
        OH, OW = ref.out_hw(H, W, k)
        n = L.ssg_conv_wgrad_strided_num_slices(B * OH * OW, cout, k, k, cin, 2)
        assert n >= 3 and (B * OH * OW) % n != 0
    # the real-width cases: three slices with a shorter last one, ragged last tiles of 128 output and of 64 input pixels per class
    for (B, H, W, cin, cout, k, _) in ref.REAL.values():
        OH, OW = ref.out_hw(H, W, k)
        M = B * OH * OW
        assert H % 2 == 0 and W % 2 == 0 and 512 < M < 768 and M % 64 != 0
        assert L.ssg_conv_wgrad_strided_num_slices(M, cout, k, k, cin, 2) == 3


def test_the_bound_sees_a_missing_chunk_stage_or_pixels_at_real_widths():
    """tests/test_conv_train_host.py's sharpness condition on the stride-2 real-width cases: each of the three mutated float64
    references (one 32-channel chunk of one tap missing from y, one 32-output-channel stage of one tap from dX, the last 32 output
    pixels from dW) breaks (L + 2) 2^-24 A on at least 3/4 of the elements it touches; torch's float32 CPU convolution meets the bound"""
    tc.check_sensitivity(ref.reference, ref.outputs, ref.REAL, 2)


def test_strided_packing_restatement():
    """pack_dgrad_s2 is [tap][Cout][Cin] with tap = r KW + s: element by element on a weight whose value names its index, and as the
    GEMM operand it is -- dY[oh, ow] wp[tap] added into dX[2 oh + r - 1, 2 ow + s - 1] gives the float64 data gradient"""
    cout, cin, k = 64, 128, 3
    idx = torch.arange(cout * cin * k * k, dtype=torch.float64).reshape(cout, cin, k, k)
    p = ref.pack_dgrad_s2(idx)
    assert tuple(p.shape) == (k * k, cout, cin) and p.is_contiguous()
    for (co, ci, r, s) in [(0, 0, 0, 0), (cout - 1, cin - 1, k - 1, k - 1), (33, 35, 1, 0), (5, 63, 0, 2)]:
        assert float(p[r * k + s, co, ci]) == float(idx[co, ci, r, s])
    B, H, W, cin, cout, k, seed = ref.CASES["3x3_even"]
    d, r64, _, _ = ref.reference(*ref.CASES["3x3_even"])
    wp, gy = ref.pack_dgrad_s2(d["w"].double()), d["gy"].double()
    OH, OW = ref.out_hw(H, W, k)
    dx = torch.zeros(B, cin, H, W, dtype=torch.float64)
    for r in range(k):
        for s in range(k):
            for oh in range(OH):
                for ow in range(OW):
                    ih, iw = 2 * oh + r - 1, 2 * ow + s - 1
                    if 0 <= ih < H and 0 <= iw < W:
                        dx[:, :, ih, iw] += gy[:, :, oh, ow] @ wp[r * k + s]
    assert float((dx - r64["dx"]).abs().max()) <= 1e-12 * float(r64["dx"].abs().max())


def test_bad_shapes_are_refused_before_any_launch(L):
    for (M, cout, kh, kw, cin, stride) in [(0, 64, 1, 1, 64, 2), (32, 64, 1, 1, 64, 1), (32, 64, 3, 3, 64, 3), (32, 96, 1, 1, 64, 2), (32, 64, 3, 3, 96, 2),
                                           (32, 64, 7, 7, 64, 2), (32, 128, 7, 7, 3, 2), (32, 64, 3, 3, 3, 2), (32, 64, 5, 5, 64, 2), (32, 64, 1, 3, 64, 2)]:
        assert L.ssg_conv_wgrad_strided_num_slices(M, cout, kh, kw, cin, stride) == -1
        assert L.ssg_conv_wgrad_strided_workspace_bytes(M, cout, kh, kw, cin, stride) == 0
    assert b"ssg_conv_wgrad_strided_workspace_bytes" in L.ssg_last_error()
    # the stride-1 entry points still refuse what they refused
    assert L.ssg_conv_wgrad_num_slices(32, 64, 7, 7, 64) == -1
    # NULL pointers / bad arguments come back as -1 with nothing launched (no GPU here)
    assert L.ssg_conv_pack_strided_f32(None, 1, 1, 1, 1, 64, 64, 3, 3, None, None, None) == -1
    assert L.ssg_conv_pack_strided_f32(None, 1, 1, 1, 1, 64, 96, 3, 3, None, None, None) == -1
    assert L.ssg_conv_pack_strided_f32(None, 1, 1, 1, 1, 64, 3, 7, 7, None, None, None) == -1
    assert L.ssg_conv_dgrad_strided_f32(None, None, None, 2, 4, 4, 64, 64, 3, 3, 2, None) == -1 and b"NULL" in L.ssg_last_error()
    assert L.ssg_conv_dgrad_strided_f32(None, None, None, 2, 4, 4, 64, 64, 3, 3, 1, None) == -1 and b"stride" in L.ssg_last_error()
    assert L.ssg_conv_dgrad_strided_f32(None, None, None, 2, 4, 4, 3, 64, 7, 7, 2, None) == -1 and b"no data gradient" in L.ssg_last_error()
    assert L.ssg_conv_dgrad_strided_f32(None, None, None, 0, 4, 4, 64, 64, 3, 3, 2, None) == -1
    assert L.ssg_conv_wgrad_strided_f32(None, None, 2, 4, 4, 64, 64, 3, 3, 2, None, 1, 1, 1, 1, None, 0, 3, None) == -1
    assert L.ssg_conv_wgrad_strided_f32(None, None, 2, 4, 4, 64, 64, 3, 3, 2, None, 1, 1, 1, 1, None, 0, 0, None) == -1
    assert L.ssg_conv_wgrad_strided_f32(None, None, 2, 4, 4, 64, 64, 3, 3, 1, None, 1, 1, 1, 1, None, 0, 3, None) == -1
    assert b"ssg_conv_wgrad_strided_f32" in L.ssg_last_error()
    assert L.ssg_maxpool3x3s2_idx_nhwc(None, None, None, 1, 4, 4, 6, None) == -1 and b"C % 4" in L.ssg_last_error()
    assert L.ssg_maxpool3x3s2_idx_nhwc(None, None, None, 1, 4, 4, 8, None) == -1 and b"NULL" in L.ssg_last_error()
    assert L.ssg_maxpool3x3s2_bwd_nhwc(None, None, None, 1, 0, 4, 8, None) == -1
    assert L.ssg_maxpool3x3s2_bwd_nhwc(None, None, None, 1, 4, 4, 8, None) == -1 and b"ssg_maxpool3x3s2_bwd_nhwc" in L.ssg_last_error()


def test_use_device_conv_strided_leaves_only_the_head():
    import ssg_amd
    m = _model()
    before = dict(m.named_parameters())
    keys = list(m.state_dict().keys())
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    ssg_amd.use_device_conv(m)                                                   # the default is unchanged: the same four layers stay
    assert sorted(m._ssg_conv_skipped) == sorted(["conv1", "layer2.0.conv2", "layer2.0.downsample.0", "head"])
    assert not any(isinstance(c, ssg_amd.StridedConv2d) for c in m.modules())
    assert ssg_amd.use_device_conv(m, strided=True) is m
    assert m._ssg_conv_skipped == ["head"]
    strided = sorted(n for n, c in m.named_modules() if isinstance(c, ssg_amd.StridedConv2d))
    assert strided == sorted(["conv1", "layer2.0.conv2", "layer2.0.downsample.0"])
    unit = [n for n, c in m.named_modules() if isinstance(c, ssg_amd.Conv2d)]
    assert len(unit) == 9 and type(m.head) is torch.nn.Conv2d
    after = dict(m.named_parameters())
    assert list(after) == list(before) and all(after[k] is before[k] for k in before)      # the same Parameter objects
    assert list(m.state_dict().keys()) == keys
    assert all(any(p is q for q in after.values()) for g in opt.param_groups for p in g["params"])
    c = m.conv1
    assert c.kernel_size == (7, 7) and c.stride == (2, 2) and c.padding == (3, 3) and c.bias is None and c.weight.device.type == "cpu"
    # a second call changes nothing
    mods = dict(m.named_modules())
    ssg_amd.use_device_conv(m, strided=True)
    assert m._ssg_conv_skipped == ["head"] and all(v is mods[k] for k, v in m.named_modules())
    # a later call without the keyword leaves the strided modules on the device path and off the list
    ssg_amd.use_device_conv(m)
    assert m._ssg_conv_skipped == ["head"] and all(v is mods[k] for k, v in m.named_modules())
    # from scratch in one call, and under DataParallel
    m2 = torch.nn.DataParallel(_model())
    ssg_amd.use_device_conv(m2, strided=True)
    assert m2._ssg_conv_skipped == ["module.head"] and isinstance(m2.module.conv1, ssg_amd.StridedConv2d)


def test_use_device_maxpool():
    import ssg_amd
    nn = torch.nn
    m = nn.Sequential(nn.MaxPool2d(3, 2, 1), nn.MaxPool2d(2), nn.Sequential(nn.MaxPool2d(kernel_size=3, stride=2, padding=1), nn.MaxPool2d(3, 2, 1, ceil_mode=True)),
                      nn.MaxPool2d(3, 1, 1), nn.AvgPool2d(3, 2, 1))
    assert ssg_amd.use_device_maxpool(m) is m
    assert m._ssg_maxpool_skipped == ["1", "2.1", "3"]
    assert isinstance(m[0], ssg_amd.MaxPool2d) and isinstance(m[2][0], ssg_amd.MaxPool2d) and type(m[1]) is nn.MaxPool2d
    assert m[0].kernel_size == 3 and m[0].stride == 2 and m[0].padding == 1
    ssg_amd.use_device_maxpool(m)                                                # a second call changes nothing
    assert m._ssg_maxpool_skipped == ["1", "2.1", "3"]
    d = nn.DataParallel(nn.Sequential(nn.MaxPool2d(3, 2, 1), nn.MaxPool2d(2)))
    ssg_amd.use_device_maxpool(d)
    assert isinstance(d.module[0], ssg_amd.MaxPool2d) and d._ssg_maxpool_skipped == ["module.1"]
    for args in [(2,), (3, 1, 1), (3, 2, 0), (3, 2, 1, 2)]:
        with pytest.raises(ValueError):
            ssg_amd.MaxPool2d(*args)
    with pytest.raises(ValueError):
        ssg_amd.MaxPool2d(3, 2, 1, ceil_mode=True)


def test_unsupported_shapes_raise_valueerror_naming_the_rule():
    import ssg_amd
    x = torch.zeros(1, 64, 4, 4)
    w1, w3 = torch.zeros(64, 64, 1, 1), torch.zeros(64, 64, 3, 3)
    stem_w = torch.zeros(64, 3, 7, 7)
    for args, kwargs, word in [
            ((x, w1, 1, 0), {}, "stride"), ((x, w3, 2, 0), {}, "padding"), ((x, w1, 2, 1), {}, "padding"),
            ((torch.zeros(1, 96, 4, 4), torch.zeros(64, 96, 1, 1), 2, 0), {}, "Cin"), ((torch.zeros(1, 3, 4, 4), torch.zeros(64, 3, 3, 3), 2, 1), {}, "Cin"),
            ((x, torch.zeros(64, 64, 7, 7), 2, 3), {}, "stem"), ((torch.zeros(1, 3, 8, 8), torch.zeros(128, 3, 7, 7), 2, 3), {}, "stem"),
            ((x, torch.zeros(64, 64, 5, 5), 2, 2), {}, "kernel"), ((x, torch.zeros(64, 32, 1, 1), 2, 0), dict(groups=2), "groups"),
            ((x, w1, 2, 0), dict(bias=torch.zeros(64)), "bias"), ((x, w1, 2, 0), dict(dilation=2), "dilation"),
            ((torch.zeros(1, 128, 4, 4), w1, 2, 0), {}, "channels"), ((x.double(), w1.double(), 2, 0), {}, "float32"),
            ((torch.zeros(1, 3, 8, 8, requires_grad=True), stem_w, 2, 3), {}, "data gradient")]:
        with pytest.raises(ValueError, match=word):
            ssg_amd.conv2d_train_strided(*args, **kwargs)
    for args in [(64, 64, 3, 1, 1), (64, 64, 1, 1, 0), (64, 64, 7, 2, 3), (3, 128, 7, 2, 3), (96, 64, 1, 2, 0), (64, 64, 3, 2, 0)]:
        with pytest.raises(ValueError):
            ssg_amd.StridedConv2d(*args)
    with pytest.raises(ValueError):
        ssg_amd.StridedConv2d(64, 64, 1, 2, 0, bias=True)
    for args in [(64, 64, 3, 2, 1), (64, 128, 1, 2, 0), (3, 64, 7, 2, 3)]:
        c = ssg_amd.StridedConv2d(*args)
        assert c.bias is None and list(c.state_dict()) == ["weight"]
    for kwargs, word in [(dict(kernel_size=2), "kernel_size"), (dict(stride=1), "stride"), (dict(padding=0), "padding"), (dict(ceil_mode=True), "ceil_mode")]:
        with pytest.raises(ValueError, match=word):
            ssg_amd.max_pool2d_train(torch.zeros(1, 4, 4, 4), **kwargs)
    with pytest.raises(ValueError, match="C % 4"):
        ssg_amd.max_pool2d_train(torch.zeros(1, 6, 4, 4))
    # the stride-1 surface is where it was
    with pytest.raises(ValueError, match="stride"):
        ssg_amd.conv2d_train(x, w3, stride=2, padding=1)
    with pytest.raises(ValueError):
        ssg_amd.Conv2d(64, 64, 3, 2, 1)
