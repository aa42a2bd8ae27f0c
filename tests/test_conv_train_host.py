"""Host half of the train-mode Conv2d tests (no GPU): the index formula of the two weight packings, the pure host functions of the
weight gradient's slice cut, the argument checks that come before any launch, use_device_conv on a hand-built model, and what the
GPU suite's bounds see of a plausible kernel fault at the real widths (mutated float64 references)."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_train_ref as ref  # noqa: E402
import train_common as tc  # noqa: E402


@pytest.fixture(scope="module")
def L():
    from ssg_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", ["3x3_border", "3x3_cin192", "3x3_cout192", "1x1_ragged"])
def test_packings_reproduce_forward_and_dgrad(name):
    """a plain matmul over the packed K order gives the float64 forward (w_fwd on x) and data gradient (w_dgrad on dY): pins
    k = ((c/32) KH KW + r KW + s) 32 + c%32 and the transposition with its 180 degree rotation"""
    B, H, W, cin, cout, k, seed = ref.CASES[name]
    d, r64, _, _ = ref.reference(*ref.CASES[name])
    x, w, gy = d["x"].double(), d["w"].double(), d["gy"].double()
    wf, wd = ref.pack_fwd(w), ref.pack_dgrad(w)
    assert tuple(wf.shape) == (cout, k * k * cin) and tuple(wd.shape) == (cin, k * k * cout)
    y = (ref.im2col_packed(x, k) @ wf.t()).reshape(B, H, W, cout).permute(0, 3, 1, 2)
    dx = (ref.im2col_packed(gy, k) @ wd.t()).reshape(B, H, W, cin).permute(0, 3, 1, 2)
    assert float((y - r64["y"]).abs().max()) <= 1e-12 * float(r64["y"].abs().max())
    assert float((dx - r64["dx"]).abs().max()) <= 1e-12 * float(r64["dx"].abs().max())
    # and the element formula itself, on a weight whose value names its index
    idx = torch.arange(cout * cin * k * k, dtype=torch.float64).reshape(cout, cin, k, k)
    pf, pd = ref.pack_fwd(idx), ref.pack_dgrad(idx)
    T = k * k
    for (co, ci, r, s) in [(0, 0, 0, 0), (cout - 1, cin - 1, k - 1, k - 1), (33, 35, k // 2, 0), (5, 63, 0, k - 1)]:
        v = float(idx[co, ci, r, s])
        assert float(pf[co, ((ci // 32) * T + r * k + s) * 32 + ci % 32]) == v
        assert float(pd[ci, ((co // 32) * T + (k - 1 - r) * k + (k - 1 - s)) * 32 + co % 32]) == v


SHAPES = [(30, 64, 1, 1, 64), (30, 64, 3, 3, 64), (1, 64, 3, 3, 64), (32, 192, 3, 3, 64), (32, 64, 3, 3, 192), (544, 64, 1, 1, 64),
          (262144, 256, 1, 1, 64), (262144, 64, 1, 1, 256), (262144, 64, 3, 3, 64), (4096, 512, 3, 3, 512), (4096, 2048, 1, 1, 512)]


def test_wgrad_slices_and_workspace(L):
    for (M, cout, kh, kw, cin) in SHAPES:
        n = L.ssg_conv_wgrad_num_slices(M, cout, kh, kw, cin)
        assert n >= 1
        assert n == L.ssg_conv_wgrad_num_slices(M, cout, kh, kw, cin)                 # a function of the shape alone
        assert L.ssg_conv_wgrad_workspace_bytes(M, cout, kh, kw, cin) == 4 * n * cout * kh * kw * cin
        assert n <= (M + 31) // 32                                                    # no slice without a pixel
    # small inputs are one slice; layer1 at B = 128 (64 x 256 result, M = 262 144) is cut into many, layer4's 3x3 into few
    assert L.ssg_conv_wgrad_num_slices(30, 64, 3, 3, 64) == 1
    assert L.ssg_conv_wgrad_num_slices(262144, 256, 1, 1, 64) >= 128
    assert 1 <= L.ssg_conv_wgrad_num_slices(4096, 512, 3, 3, 512) <= 4
    # the GPU suite's multi-slice cases exist: some B <= 64 gives three slices, with a ragged last one
    for (H, W, cin, cout, k, _) in ref.MULTI.values():
        B = ref.multi_slice_batch(L, H, W, cin, cout, k)
        assert B is not None and B <= 64
        n = L.ssg_conv_wgrad_num_slices(B * H * W, cout, k, k, cin)
        assert n >= 3 and (B * H * W) % n != 0
    # the real-width cases: three slices with a shorter last one, a ragged last 128-row tile
    for (B, H, W, cin, cout, k, _) in ref.REAL.values():
        M = B * H * W
        assert 512 < M < 768 and M % 128 != 0 and L.ssg_conv_wgrad_num_slices(M, cout, k, k, cin) == 3


def test_the_bound_sees_a_missing_chunk_stage_or_pixels_at_real_widths():
    """the yardstick of the real-width GPU cases is sharp there: a forward without one 32-channel chunk of one tap, a data gradient
    without one 32-output-channel stage of one tap and a weight gradient without its last 32 pixels each break (L + 2) 2^-24 A on at
    least 3/4 of the elements they touch -- a condition on the cases' data and shapes, not a measurement (seen on the CPU: 0.90 ... 1.00);
    torch's float32 CPU convolution meets the same bound everywhere"""
    tc.check_sensitivity(ref.reference, ref.outputs, ref.REAL, 1)


@pytest.mark.parametrize("name", sorted(ref.TRAINER))
def test_the_slice_aware_bound_sees_a_missing_stage_at_the_trainers_batch(L, name):
    """the dW bound of test_gpu_conv_train.py::test_trainer_batch_1x1_against_float64_matmul, (L_s + 2) 2^-24 A with L_s the slice
    length bound from the public slice count, against a weight gradient without one 32-pixel stage (the last of the first slice):
    broken on at least 3/4 of dW; the usual (M + 2) 2^-24 A would not notice"""
    B, H, W, cin, cout, _ = ref.TRAINER[name]
    M = B * H * W
    d, r64, A = ref.gemm_reference(name)
    n = L.ssg_conv_wgrad_num_slices(M, cout, 1, 1, cin)
    Ls = ref.slice_length_bound(M, n)
    assert n >= 256 and 256 <= Ls <= 2 * M // n + 2
    gm = d["gy"].double()
    m0 = (M // n) // 32 * 32 - 32                                     # inside the first slice, whatever the cut
    gm[m0:m0 + 32] = 0
    delta = (gm.t() @ d["x"].double() - r64["dw"]).abs()
    seen = float((delta > ref.bound(Ls, A["dw"])).double().mean())
    blind = float((delta > ref.bound(M, A["dw"])).double().mean())
    print("%s: n = %d, L_s = %d, seen by the slice-aware bound %.3f, by (M + 2) 2^-24 A %.3f" % (name, n, Ls, seen, blind))
    assert seen >= 0.75 and blind == 0.0


def test_bad_shapes_are_refused_before_any_launch(L):
    for (M, cout, kh, kw, cin) in [(0, 64, 1, 1, 64), (-5, 64, 1, 1, 64), (32, 96, 1, 1, 64), (32, 64, 1, 1, 96), (32, 64, 1, 1, 3),
                                   (32, 64, 7, 7, 64), (32, 64, 1, 3, 64), (32, 0, 1, 1, 64)]:
        assert L.ssg_conv_wgrad_num_slices(M, cout, kh, kw, cin) == -1
        assert L.ssg_conv_wgrad_workspace_bytes(M, cout, kh, kw, cin) == 0
    # NULL pointers / bad arguments come back as -1 with nothing launched (no GPU here)
    assert L.ssg_conv_pack_train_f32(None, 1, 1, 1, 1, 64, 64, 1, 1, None, None, None) == -1
    assert L.ssg_conv_pack_train_f32(None, 1, 1, 1, 1, 64, 96, 1, 1, None, None, None) == -1
    assert L.ssg_conv_wgrad_f32(None, None, 2, 4, 4, 64, 64, 3, 3, None, 1, 1, 1, 1, None, 0, 3, None) == -1
    assert L.ssg_conv_wgrad_f32(None, None, 2, 4, 4, 64, 64, 3, 3, None, 1, 1, 1, 1, None, 0, 0, None) == -1
    assert b"ssg_conv_wgrad_f32" in L.ssg_last_error()


def _model():
    nn = torch.nn
    m = nn.Module()
    m.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)            # the stem: 7x7 stride 2, Cin = 3
    m.bn1 = nn.BatchNorm2d(64)
    m.layer1 = nn.Sequential(ref.Bottleneck(64, 64, 1, ref.downsample(64, 256, 1)), ref.Bottleneck(256, 64))
    m.layer2 = nn.Sequential(ref.Bottleneck(256, 128, 2, ref.downsample(256, 512, 2)))   # a stride-2 3x3 and a stride-2 1x1
    m.head = nn.Conv2d(512, 64, 1, bias=True)                                 # a bias
    return m


def test_use_device_conv_swaps_exactly_the_supported_class():
    import ssg_amd
    m = _model()
    before = dict(m.named_parameters())
    keys = list(m.state_dict().keys())
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    out = ssg_amd.use_device_conv(m)
    assert out is m
    assert sorted(m._ssg_conv_skipped) == sorted(["conv1", "layer2.0.conv2", "layer2.0.downsample.0", "head"])
    swapped = [n for n, c in m.named_modules() if isinstance(c, ssg_amd.Conv2d)]
    assert sorted(swapped) == sorted(["layer1.0.conv1", "layer1.0.conv2", "layer1.0.conv3", "layer1.0.downsample.0", "layer1.1.conv1",
                                      "layer1.1.conv2", "layer1.1.conv3", "layer2.0.conv1", "layer2.0.conv3"])
    for n, c in m.named_modules():
        if isinstance(c, torch.nn.Conv2d) and not isinstance(c, ssg_amd.Conv2d):
            assert n in m._ssg_conv_skipped and type(c) is torch.nn.Conv2d
    after = dict(m.named_parameters())
    assert list(after) == list(before) and all(after[k] is before[k] for k in before)      # the same Parameter objects
    assert list(m.state_dict().keys()) == keys
    assert all(any(p is q for q in after.values()) for g in opt.param_groups for p in g["params"])
    c = m.layer1[0].conv2
    assert isinstance(c, torch.nn.Conv2d) and c.kernel_size == (3, 3) and c.padding == (1, 1) and c.bias is None and c.weight.device.type == "cpu"
    # a second call changes nothing
    ssg_amd.use_device_conv(m)
    assert [n for n, c in m.named_modules() if isinstance(c, ssg_amd.Conv2d)] == swapped and len(m._ssg_conv_skipped) == 4


def test_use_device_conv_walks_through_dataparallel():
    import ssg_amd
    m = torch.nn.DataParallel(_model())
    ssg_amd.use_device_conv(m)
    assert isinstance(m.module.layer1[1].conv1, ssg_amd.Conv2d)
    assert "module.conv1" in m._ssg_conv_skipped and "module.layer2.0.conv2" in m._ssg_conv_skipped


def test_unsupported_shapes_raise_valueerror_naming_the_rule():
    import ssg_amd
    x = torch.zeros(1, 64, 4, 4)
    w1 = torch.zeros(64, 64, 1, 1)
    for kwargs, xs, ws, word in [
            (dict(stride=2), x, w1, "stride"), (dict(padding=1), x, w1, "padding"), (dict(), torch.zeros(1, 3, 4, 4), torch.zeros(64, 3, 1, 1), "Cin"),
            (dict(), torch.zeros(1, 96, 4, 4), torch.zeros(64, 96, 1, 1), "Cin"), (dict(groups=2), x, torch.zeros(64, 32, 1, 1), "groups"),
            (dict(bias=torch.zeros(64)), x, w1, "bias"), (dict(dilation=2), x, w1, "dilation"), (dict(padding=3), x, torch.zeros(64, 64, 7, 7), "kernel")]:
        with pytest.raises(ValueError, match=word):
            ssg_amd.conv2d_train(xs, ws, **kwargs)
    for args in [(64, 64, 3, 2, 1), (3, 64, 1), (96, 64, 1), (64, 64, 7, 1, 3)]:
        with pytest.raises(ValueError):
            ssg_amd.Conv2d(*args)
    with pytest.raises(ValueError):
        ssg_amd.Conv2d(64, 64, 1, bias=True)
    with pytest.raises(ValueError):
        ssg_amd.Conv2d(64, 64, 1, groups=2)
