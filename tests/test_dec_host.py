"""CPU suite of the DEC head (--dce-loss): the yardstick tests/dec_ref.py against the reference's own numbers
(tests/golden/dec_cases.npz, tools/make_golden_dec.py), the host surface of ssg_amd.dce / ssg_amd.trainers /
ssg_amd.create(cluster=True), and the argument validation of the four entry points of csrc/dec.hip (nothing is launched)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dec_ref  # noqa: E402

import ssg_amd  # noqa: E402
from ssg_amd import _lib, dce, trainers  # noqa: E402


def test_dec_ref_float64_matches_the_reference_goldens(golden):
    """dec_ref in float64 against the reference's ClusterAssignment / target_distribution / KLDivLoss in float64: within 1e-12 of each
    array's largest magnitude (float64 rounding of a 2048-term sum is <= 2048 * 2^-53 ~ 2.3e-13).  At B = 1 the exact loss and
    gradients are 0 and the stored ones are rounding residue (|loss| ~ 2e-16), so there the bound gets the absolute floor K^2 * 2^-52:
    p = q / sum(q) with sum(q) within K half-ulps of 1, passed through at most K terms per gradient entry."""
    g = golden("dec_cases.npz")
    assert int(g["cases"]) == 4
    assert [tuple(int(v) for v in g["case_%d" % ci][:3]) for ci in range(4)] == [(5, 3, 40), (6, 32, 2048), (1, 32, 2048), (16, 32, 2048)]
    for ci in range(4):
        B, K, D, seed = (int(v) for v in g["case_%d" % ci])
        x, c = dec_ref.case_inputs(B, K, D, seed, float(g["scale_%d" % ci]))
        assert x.dtype == torch.float32 and float(x.min()) >= 0.0
        assert np.array_equal(dec_ref.sha_bytes(x, c), g["sha_%d" % ci]), "case %d: the regenerated inputs are not the golden's" % ci
        out = dec_ref.chain(x, c, torch.float64)
        cols = torch.from_numpy(g["cols_%d" % ci])
        floor = K * K * 2.0 ** -52 if B == 1 else 0.0
        for name, got, fl in (("q", out["q"], 0.0), ("p", out["p"], 0.0), ("loss", out["loss"], floor), ("gx", out["gx"][:, cols], floor),
                              ("gc", out["gc"][:, cols], floor)):
            ref = torch.from_numpy(np.asarray(g["%s_%d" % (name, ci)], dtype=np.float64))
            assert got.shape == ref.shape, (ci, name)
            err = float((got - ref).abs().max())
            assert err <= 1e-12 * float(ref.abs().max()) + fl, (ci, name, err, float(ref.abs().max()))
        # the pieces the GPU tests use one by one agree with the chain
        p, loss, gq = dec_ref.loss_grad_q(out["q"], torch.float64)
        gx, gc = dec_ref.assign_grad(x, c, gq, torch.float64)
        assert torch.equal(p, out["p"]) and torch.equal(loss, out["loss"])
        for got, ref in ((gx, out["gx"]), (gc, out["gc"])):
            assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()) + floor


def test_dec_ref_trainer_totals_match_the_references_forward(golden):
    """dec_ref.trainer_totals in float64 against what FinedTrainer2._forward / JointTrainer2._forward returned for the stub model and
    criterions of tools/make_golden_dec.py"""
    g = golden("dec_cases.npz")
    kl = []
    for ci in (int(v) for v in g["trainer_cases"]):
        B, K, D, seed = (int(v) for v in g["case_%d" % ci])
        x, c = dec_ref.case_inputs(B, K, D, seed, float(g["scale_%d" % ci]))
        kl.append(dec_ref.chain(x, c, torch.float64)["loss"])
    tot = dec_ref.trainer_totals(kl[0], kl[1], torch.tensor(float(g["tri"][0]), dtype=torch.float64), torch.tensor(float(g["global"][0]), dtype=torch.float64))
    for name, v in tot.items():
        ref = float(g[name + "_loss"])
        assert abs(float(v) - ref) <= 1e-12 * abs(ref), (name, float(v), ref)
    assert float(g["fined_tensor_prec"]) == float(g["global"][1]) and float(g["joint_tensor_prec"]) == 2 * float(g["global"][1])


def test_cluster_assignment_constructor_mirrors_the_reference():
    torch.manual_seed(5)
    m = dce.ClusterAssignment(cluster_number=32, embedding_dimension=2048, alpha=3.0)
    torch.manual_seed(5)
    ref = torch.zeros(32, 2048, dtype=torch.float)
    torch.nn.init.xavier_uniform_(ref)
    assert (m.cluster_number, m.embedding_dimension, m.alpha) == (32, 2048, 1.0)          # alpha ignored, dce.py:27
    assert isinstance(m.cluster_centers, torch.nn.Parameter) and m.cluster_centers.requires_grad
    assert torch.equal(m.cluster_centers.detach(), ref)
    assert list(m.state_dict()) == ["cluster_centers"] and [n for n, _ in m.named_parameters()] == ["cluster_centers"]
    given = torch.arange(12, dtype=torch.float32).view(3, 4)
    m2 = ssg_amd.ClusterAssignment(3, 4, cluster_centers=given)
    assert torch.equal(m2.cluster_centers.detach(), given) and m2.alpha == 1.0
    with pytest.raises(ValueError):
        m2(torch.zeros(2, 5))           # the width is checked before the device is asked for


def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    m = dce.ClusterAssignment(3, 4)
    q = torch.full((2, 3), 1.0 / 3)
    for call in (lambda: m(torch.zeros(2, 4)), lambda: ssg_amd.kl_loss(q), lambda: ssg_amd.target_distribution(q),
                 lambda: ssg_amd.soft_assignment(torch.zeros(2, 4), torch.zeros(3, 4))):
        with pytest.raises(ssg_amd.SSGError, match="GPU"):
            call()
    for bad in (torch.zeros(3), torch.zeros(2, 3, 4)):
        with pytest.raises(ValueError):
            dce.kl_loss(bad)
        with pytest.raises(ValueError):
            dce.target_distribution(bad)


def test_use_device_assignment_keeps_the_parameter():
    class Old(torch.nn.Module):                       # stands for reid.models.dce.ClusterAssignment inside the reference's ResNet
        def __init__(self):
            super().__init__()
            self.cluster_centers = torch.nn.Parameter(torch.randn(32, 16, generator=torch.Generator().manual_seed(0)))

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.feat = torch.nn.Linear(4, 4)
            self.assignment = Old()

    class Wrapped(object):                            # nn.DataParallel's .module
        def __init__(self, m):
            self.module = m

    for wrap in (False, True):
        net = Net()
        par = net.assignment.cluster_centers
        opt = torch.optim.SGD(net.parameters(), lr=0.1)
        keys = list(net.state_dict())
        model = Wrapped(net) if wrap else net
        assert ssg_amd.use_device_assignment(model) is model
        assert isinstance(net.assignment, dce.ClusterAssignment) and net.assignment.cluster_centers is par
        assert (net.assignment.cluster_number, net.assignment.embedding_dimension, net.assignment.alpha) == (32, 16, 1.0)
        assert list(net.state_dict()) == keys and "assignment.cluster_centers" in keys
        assert any(p is par for grp in opt.param_groups for p in grp["params"])
    with pytest.raises(ValueError, match="assignment"):
        dce.use_device_assignment(torch.nn.Linear(2, 2))


def test_create_cluster_state_dict_surface():
    key = "assignment.cluster_centers"
    m = ssg_amd.create("resnet50", num_classes=0, num_split=1, cluster=True, pretrained=False, seed=3)
    plain = ssg_amd.create("resnet50", num_classes=0, num_split=1, cluster=False, pretrained=False, seed=3)
    sd, sd0 = m.state_dict(), plain.state_dict()
    assert m.cluster is True and list(sd)[-1] == key and list(sd)[:-1] == list(sd0)              # registered last, as in the reference
    assert sd[key].shape == (32, 2048) and sd[key].dtype == torch.float32
    bound = (6.0 / (32 + 2048)) ** 0.5                                                             # Xavier uniform
    assert float(sd[key].abs().max()) <= bound and float(sd[key].abs().max()) > 0.99 * bound and abs(float(sd[key].mean())) < 1e-3
    assert all(torch.equal(sd[k], sd0[k]) for k in sd0)                                            # the backbone is the cluster=False one
    assert torch.equal(ssg_amd.create("resnet50", num_classes=0, cluster=True, pretrained=False, seed=3).state_dict()[key], sd[key])
    assert not torch.equal(ssg_amd.create("resnet50", num_classes=0, cluster=True, pretrained=False, seed=4).state_dict()[key], sd[key])
    # round trip, strict: plain keys, nn.DataParallel's prefix, the whole checkpoint
    new = sd[key] * 0.5 + 0.01
    for form in (lambda d: d, lambda d: {"module." + k: v for k, v in d.items()}, lambda d: {"state_dict": d, "epoch": 7}):
        m2 = ssg_amd.create("resnet50", num_classes=0, num_split=1, cluster=True, pretrained=False, seed=9)
        d = dict(sd)
        d[key] = new
        missing, unexpected = m2.load_state_dict(form(d), strict=True)
        assert not missing and not unexpected and torch.equal(m2.state_dict()[key], new)
    # strictness sees the key from both sides
    with pytest.raises(RuntimeError, match="assignment.cluster_centers"):
        plain.load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError, match="assignment.cluster_centers"):
        m.load_state_dict(sd0, strict=True)
    with pytest.raises(RuntimeError, match="size mismatch"):
        m.load_state_dict({key: torch.zeros(32, 1024)}, strict=False)
    # the f32 twin inherits the head
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = m._f32_twin()
    assert t.cluster is True and t.precision == "f32" and torch.equal(t._sd[key], m._sd[key])


def test_create_cluster_with_splits_names_the_references_shape_mismatch():
    """resnet.py:129: with num_split > 1 and for_eval=False the reference concatenates (S+1) * 2048 columns against 2048-wide centres and
    dies in broadcasting; here a ValueError that says so, raised before any GPU work (the model is still on the CPU)."""
    m = ssg_amd.create("resnet50", num_classes=0, num_split=2, cluster=True, pretrained=False)
    with pytest.raises(ValueError, match="6144.*2048.*resnet.py:129"):
        m(torch.zeros(1, 3, 64, 32))
    with pytest.raises(ValueError, match="shape mismatch"):
        m(torch.zeros(1, 3, 64, 32), for_eval=False)


def test_entry_points_validate_without_gpu():
    """1 <= B <= 4096, 1 <= K <= 64, D >= 1, pitch >= D, alpha > 0, no NULL pointer: refused before a launch, with a message that
    names the entry point and the offending value"""
    L = _lib.lib()
    one = (torch.zeros(1).data_ptr(),)       # any non-NULL address: nothing is dereferenced
    P = one[0]

    def refused(rc, name, what):
        msg = L.ssg_last_error().decode()
        assert rc == -1 and name in msg and what in msg, (rc, msg)

    for B, K, what in ((0, 32, "B=0"), (-1, 32, "B=-1"), (4097, 32, "B=4097"), (8, 0, "K=0"), (8, 65, "K=65"), (8, -2, "K=-2")):
        refused(L.ssg_dec_assign_f32(P, 2048, P, B, K, 2048, 1.0, P, None, None), "ssg_dec_assign_f32", what)
        refused(L.ssg_dec_kl_loss_f32(P, B, K, None, P, None), "ssg_dec_kl_loss_f32", what)
        refused(L.ssg_dec_kl_loss_grad_f32(P, B, K, P, P, None), "ssg_dec_kl_loss_grad_f32", what)
        refused(L.ssg_dec_assign_grad_f32(P, 2048, P, P, P, B, K, 2048, 1.0, P, P, P, None), "ssg_dec_assign_grad_f32", what)
    for D, ldx, alpha, what in ((0, 8, 1.0, "D=0"), (-4, 8, 1.0, "D=-4"), (40, 39, 1.0, "ldx=39"), (40, 40, 0.0, "alpha=0"), (40, 40, -1.0, "alpha=-1"),
                                (40, 40, float("nan"), "alpha=nan"), (40, 40, float("inf"), "alpha=inf")):
        refused(L.ssg_dec_assign_f32(P, ldx, P, 5, 3, D, alpha, P, None, None), "ssg_dec_assign_f32", what)
        refused(L.ssg_dec_assign_grad_f32(P, ldx, P, P, P, 5, 3, D, alpha, P, P, P, None), "ssg_dec_assign_grad_f32", what)
    refused(L.ssg_dec_assign_f32(None, 40, P, 5, 3, 40, 1.0, P, None, None), "ssg_dec_assign_f32", "NULL")
    refused(L.ssg_dec_assign_f32(P, 40, P, 5, 3, 40, 1.0, None, None, None), "ssg_dec_assign_f32", "NULL")
    refused(L.ssg_dec_kl_loss_f32(P, 5, 3, None, None, None), "ssg_dec_kl_loss_f32", "NULL")
    refused(L.ssg_dec_kl_loss_grad_f32(P, 5, 3, None, P, None), "ssg_dec_kl_loss_grad_f32", "NULL")
    refused(L.ssg_dec_assign_grad_f32(P, 40, P, P, P, 5, 3, 40, 1.0, None, P, P, None), "ssg_dec_assign_grad_f32", "NULL")
    with pytest.raises(ValueError, match="ssg_dec_kl_loss_f32"):
        _lib.check(L.ssg_dec_kl_loss_f32(P, 5000, 3, None, P, None), "ssg_dec_kl_loss_f32")


def test_trainer_mixins_keep_the_references_branches():
    """the mixins in front of stand-ins for reid.trainers.FinedTrainer2 / JointTrainer2; with a two-output model (cluster=False) there is
    no DEC term and nothing touches the device: which criterion sees which output and which labels, and the precision returned"""
    class Base(object):
        def __init__(self, model, criterions, beta=0.5):
            self.model, self.criterions, self.beta = model, criterions, beta

        def _forward(self, *a, **k):
            raise AssertionError("the mixin's _forward must come first")

    class Fined(ssg_amd.DECFinedTrainer2Mixin, Base):
        pass

    class Joint(ssg_amd.DECJointTrainer2Mixin, Base):
        pass

    assert Fined._forward is trainers.DECFinedTrainer2Mixin._forward and Joint._forward is trainers.DECJointTrainer2Mixin._forward
    seen = []

    def crit(tag, loss, prec):
        def f(out, pids, epoch, w=None):
            seen.append((tag, float(out.sum()), int(pids[0])))
            return torch.tensor(loss), prec
        return f

    crits = [crit("tri", 0.25, 0.1), crit("glob", 0.5, 0.7)]
    feats = [torch.full((2, 3), float(v)) for v in (1, 2, 3)]
    pids = [torch.tensor([10, 10]), torch.tensor([11, 11]), torch.tensor([12, 12])]
    loss, prec = Fined(lambda imgs: (feats, feats[0] * 5), crits)._forward([None], pids, 0)
    assert float(loss) == 0.5 + 3 * 0.25 and prec == 0.7
    assert seen == [("glob", 30.0, 10), ("tri", 6.0, 10), ("tri", 12.0, 11), ("tri", 18.0, 12)]
    del seen[:]
    loss, prec = Fined(lambda imgs: (feats[1], feats[0]), crits)._forward([None], pids, 0)
    assert float(loss) == 0.75 and prec == 0.7 and seen == [("glob", 6.0, 10), ("tri", 12.0, 10)]
    del seen[:]
    eug_pids = torch.tensor([20, 20])
    loss, prec = Joint(lambda imgs: (feats, feats[0] * 5), crits)._forward([None], pids, [None], eug_pids, 0)
    assert float(loss) == 2 * (0.5 + 3 * 0.25) and prec == 1.4
    assert seen == [("glob", 30.0, 10), ("tri", 6.0, 10), ("tri", 12.0, 11), ("tri", 18.0, 12),
                    ("glob", 30.0, 20), ("tri", 6.0, 20), ("tri", 12.0, 20), ("tri", 18.0, 20)]
