"""CPU checks of the device TripletLoss surface (ssg_amd.triplet.TripletLoss, hard_pairs, triplet_loss_from_dist): the
reference's attributes and errors, raised before any GPU work, and the argument validation of the new C entry points."""
import pytest

torch = pytest.importorskip("torch")

import ssg_amd  # noqa: E402
from ssg_amd import _lib, triplet  # noqa: E402


def test_constructor_attributes():
    crit = triplet.TripletLoss(margin=0.5, num_instances=4, use_semi=False)
    assert (crit.margin, crit.K, crit.use_semi) == (0.5, 4, False)
    default = triplet.TripletLoss()
    assert (default.margin, default.K, default.use_semi) == (0, 0, True)
    assert isinstance(default, torch.nn.Module)
    assert ssg_amd.TripletLoss is triplet.TripletLoss


def test_reference_errors_before_any_gpu_work():
    x = torch.zeros(8, 16)
    t = torch.arange(8) // 4
    for semi in (True, False):                                   # P = n // K comes first in both branches
        with pytest.raises(ZeroDivisionError):
            triplet.TripletLoss(num_instances=0, use_semi=semi)(x, t, 0)
        with pytest.raises(ZeroDivisionError):
            triplet.triplet_loss_from_dist(torch.zeros(8, 8), t, 0, use_semi=semi)
        with pytest.raises(ZeroDivisionError):
            triplet.hard_pairs(torch.zeros(8, 8), t, 0, semi)
    for n, K in ((8, 1), (3, 4)):                                # semi with M == 0: the reference's torch.cat([])
        with pytest.raises(RuntimeError):
            triplet.TripletLoss(num_instances=K, use_semi=True)(torch.zeros(n, 16), torch.zeros(n), 0)
        with pytest.raises(RuntimeError):
            triplet.hard_pairs(torch.zeros(n, n), torch.zeros(n), K, True)
    with pytest.raises(ValueError):
        triplet.TripletLoss(num_instances=4)(torch.zeros(4100, 8), torch.arange(4100) // 4, 0)
    with pytest.raises(ValueError):
        triplet.triplet_loss_from_dist(torch.zeros(4100, 4100), torch.arange(4100) // 4, 4, use_semi=False)
    with pytest.raises(ValueError):
        triplet.hard_pairs(torch.zeros(8, 7), t, 4)


def test_no_cpu_fallback_without_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ssg_amd.SSGError):
        triplet.TripletLoss(num_instances=4)(torch.zeros(8, 16), torch.arange(8) // 4, 0)


def test_argument_validation_without_gpu():
    L = _lib.lib()
    mine, gdist, gw = L.ssg_triplet_mine_f32, L.ssg_triplet_grad_dist_f32, L.ssg_triplet_grad_weights_rec
    # (in, ld, is_sq, lo, targets, n, K, semi, M, margin, weighted, rec_f, rec_i, loss, prec, stream)
    bad = [
        ((None, 4200, 1, 1e-12, None, 4097, 4, 1, 6144, 0.0, 0), b"n=4097"),
        ((None, 0, 1, 1e-12, None, 0, 4, 1, 0, 0.0, 0), b"n=0"),
        ((None, 100, 1, 1e-12, None, 128, 4, 1, 192, 0.0, 0), b"pitch"),
        ((None, 128, 2, 1e-12, None, 128, 4, 1, 192, 0.0, 0), b"is_sq"),
        ((None, 128, 1, 1e-12, None, 128, 4, 2, 192, 0.0, 0), b"mode"),
        ((None, 128, 1, 1e-12, None, 128, 4, 1, 192, 0.0, 3), b"weighted"),
        ((None, 128, 1, 1e-12, None, 128, 0, 1, 192, 0.0, 0), b"K=0"),
        ((None, 128, 1, 1e-12, None, 128, 4, 1, 191, 0.0, 0), b"M=191"),
        ((None, 128, 1, 1e-12, None, 128, 4, 0, 192, 0.0, 0), b"M=192"),
        ((None, 3, 1, 1e-12, None, 3, 4, 1, 0, 0.0, 0), b"M=0"),
        ((None, 4096, 1, 1e-12, None, 4096, 64, 1, 129024, 0.0, 1), b"w branch"),
        ((None, 128, 1, 1e-12, None, 128, 4, 1, 192, 0.0, 0), b"NULL"),
    ]
    for args, msg in bad:
        assert mine(*args, None, None, None, None, None) == -1, args
        assert msg in L.ssg_last_error(), (args, L.ssg_last_error())
        if msg != b"NULL":
            assert gdist(*args[:9], args[10], None, None, None, None, None, None, None) == -1, args
            assert msg in L.ssg_last_error(), (args, L.ssg_last_error())
    assert gdist(None, 128, 0, 1e-12, None, 128, 4, 0, 128, 0, None, None, None, None, None, None, None) == -1
    assert b"NULL" in L.ssg_last_error()
    # (sq, ldq, lo, targets, n, K, semi, M, weighted, rec_f, rec_i, gloss, x, d, ldS, dp, S, rowsum, xt, zeros, stream)
    assert gw(None, 128, 1e-12, None, 128, 4, 3, 192, 0, None, None, None, None, 2048, 128, 2048, None, None, None, None, None) == -1
    assert b"mode" in L.ssg_last_error()
    assert gw(None, 128, 1e-12, None, 128, 4, 1, 192, 0, None, None, None, None, 2048, 120, 2048, None, None, None, None, None) == -1
    assert b"ldS=120" in L.ssg_last_error()
    assert gw(None, 128, 1e-12, None, 128, 4, 1, 192, 0, None, None, None, None, 2048, 128, 2000, None, None, None, None, None) == -1
    assert b"dp=2000" in L.ssg_last_error()
    assert gw(None, 128, 1e-12, None, 128, 4, 1, 192, 0, None, None, None, None, 2048, 128, 2048, None, None, None, None, None) == -1
    assert b"NULL" in L.ssg_last_error()
