"""GPU suite of the DEC head (--dce-loss, csrc/dec.hip): the four entry points through the C ABI, the autograd modules of
ssg_amd.dce, ssg_amd.create(cluster=True) and the trainer mixins, against tests/dec_ref.py.

Accuracy criterion (every output, every case): with err(v) = max |v - ref64| / max |ref64| and ref64 = dec_ref in float64,

    err(device) <= F * err(dec_ref in float32 on the CPU) + 2^-24

-- the float32 run is the reference's own arithmetic (the torch op chain a user runs without the kernels), not the code under test;
2^-24 is the rounding of the float32 output itself.  F = 1: the next power of two above the worst ratio measured on the MI355X, 0.54
(the loss of the autograd chain at (5, 3, 40), where q crosses from the module to the loss as float32; the entry points on their own
stay below 0.06: profiles/dec_errors.txt, written by tools/dec_errors.py from `measure()` / `measure_chain()` below).  By the issue F
may not exceed 4."""
import os
import sys
from functools import lru_cache

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dec_ref  # noqa: E402

pytestmark = pytest.mark.gpu

F = 1.0
FLOOR = 2.0 ** -24

# name -> (B, K, D, scale, row pitch (0: D), first centre := first row, seed)
CASES = {
    "workload_s005": (128, 32, 2048, 0.05, 0, False, 301),       # the workload's own shape, features of the pooled layer4 map's size
    "workload_s1": (128, 32, 2048, 1.0, 0, False, 302),
    "small_batch": (6, 32, 2048, 0.05, 0, False, 303),
    "odd": (5, 3, 40, 1.0, 0, False, 304),
    "k64_d100": (37, 64, 100, 1.0, 0, False, 305),              # K at its limit, D % 4 != 0, more rows than waves of the loss kernel
    "single_row": (1, 32, 2048, 1.0, 0, False, 306),
    "pitch": (9, 5, 70, 0.05, 96, False, 307),
    "ns_zero": (7, 4, 50, 1.0, 0, True, 308),
}


def _inputs(name):
    B, K, D, scale, pitch, at_centre, seed = CASES[name]
    x, c = dec_ref.case_inputs(B, K, D, seed, scale)
    if at_centre:
        c[0] = x[0]                       # ns[0, 0] == 0 exactly
    return x, c


@lru_cache(maxsize=None)
def _refs(name):
    """the yardsticks of one case, computed once: the whole chain in float64 and in float32, then the loss and the assignment gradient
    from the float32 inputs the device entry points get (q_in, gq_in), again in both precisions"""
    B, K = CASES[name][:2]
    x, c = _inputs(name)
    r64, r32 = dec_ref.chain(x, c, torch.float64), dec_ref.chain(x, c, torch.float32)
    q_in = r64["q"].float()
    l64, l32 = dec_ref.loss_grad_q(q_in, torch.float64), dec_ref.loss_grad_q(q_in, torch.float32)
    if B == 1:      # the loss gradient is exactly 0 there: a seeded dense upstream gradient instead
        gq_in = torch.randn(B, K, generator=torch.Generator().manual_seed(CASES[name][6]))
    else:
        gq_in = l64[2].float()
    a64, a32 = dec_ref.assign_grad(x, c, gq_in, torch.float64), dec_ref.assign_grad(x, c, gq_in, torch.float32)
    return dict(x=x, c=c, r64=r64, r32=r32, q_in=q_in, l64=l64, l32=l32, gq_in=gq_in, a64=a64, a32=a32)


def _on_device(name):
    """x on the GPU at the case's row pitch (a view of a wider buffer filled with NaN: a kernel that reads the padding shows it)"""
    r = _refs(name)
    B, K, D, _, pitch = CASES[name][:5]
    if pitch:
        buf = torch.full((B, pitch), float("nan"), device="cuda")
        buf[:, :D] = r["x"].cuda()
        xd = buf[:, :D]
        assert xd.stride(0) == pitch
    else:
        xd = r["x"].cuda()
    return xd, r["c"].cuda()


def _abi(name):
    """every entry point once through the C ABI -> [(output name, device value, ref64, ref32)]"""
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr, stream
    L = _lib.lib()
    r = _refs(name)
    B, K, D = CASES[name][:3]
    xd, cd = _on_device(name)

    def new(*shape, dtype=torch.float32):
        return torch.full(shape, float("nan"), dtype=dtype, device="cuda")
    q, ns = new(B, K), new(B, K)
    check(L.ssg_dec_assign_f32(ptr(xd), xd.stride(0), ptr(cd), B, K, D, 1.0, ptr(q), ptr(ns), stream()), "ssg_dec_assign_f32")
    q_only = new(B, K)
    check(L.ssg_dec_assign_f32(ptr(xd), xd.stride(0), ptr(cd), B, K, D, 1.0, ptr(q_only), None, stream()), "ssg_dec_assign_f32")
    assert torch.equal(q_only, q)
    q_in = r["q_in"].cuda()
    p, loss, loss_only = new(B, K), new(), new()
    check(L.ssg_dec_kl_loss_f32(ptr(q_in), B, K, ptr(p), ptr(loss), stream()), "ssg_dec_kl_loss_f32")
    check(L.ssg_dec_kl_loss_f32(ptr(q_in), B, K, None, ptr(loss_only), stream()), "ssg_dec_kl_loss_f32")
    assert torch.equal(loss_only, loss)
    gq, gq3, one, three = new(B, K), new(B, K), torch.ones((), device="cuda"), torch.full((), 3.0, device="cuda")
    check(L.ssg_dec_kl_loss_grad_f32(ptr(q_in), B, K, ptr(one), ptr(gq), stream()), "ssg_dec_kl_loss_grad_f32")
    check(L.ssg_dec_kl_loss_grad_f32(ptr(q_in), B, K, ptr(three), ptr(gq3), stream()), "ssg_dec_kl_loss_grad_f32")
    gq_in = r["gq_in"].cuda()
    gns, gx, gc = new(B, K, dtype=torch.float64), new(B, D), new(K, D)
    check(L.ssg_dec_assign_grad_f32(ptr(xd), xd.stride(0), ptr(cd), ptr(ns), ptr(gq_in), B, K, D, 1.0, ptr(gns), ptr(gx), ptr(gc), stream()),
          "ssg_dec_assign_grad_f32")
    torch.cuda.synchronize()
    out = [("q", q, r["r64"]["q"], r["r32"]["q"]), ("ns", ns, r["r64"]["ns"], r["r32"]["ns"]),
           ("p", p, r["l64"][0], r["l32"][0]), ("loss", loss, r["l64"][1], r["l32"][1]),
           ("gq", gq, r["l64"][2], r["l32"][2]), ("gq_x3", gq3, 3 * r["l64"][2], 3 * r["l32"][2]),
           ("gx", gx, r["a64"][0], r["a32"][0]), ("gc", gc, r["a64"][1], r["a32"][1])]
    return [(n, d.cpu(), a, b) for n, d, a, b in out]


def measure(name, outs=None):
    """[(output, err_dev, err_f32)] of one case; at B = 1 the outputs whose exact value is 0 (loss, gq) are left out"""
    rows = []
    for n, dev, r64, r32 in outs or _abi(name):
        if CASES[name][0] == 1 and n in ("loss", "gq", "gq_x3"):
            continue
        rows.append((n, dec_ref.rel_err(dev, r64), dec_ref.rel_err(r32, r64)))
    return rows


def _within(err_dev, err_f32):
    return err_dev <= F * err_f32 + FLOOR


@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_points_vs_float64_reference(name):
    """criterion of the module docstring for q, ns, p, loss, gq (upstream 1 and 3), gx, gc.  B = 1: loss and gradient are exactly 0 in
    exact arithmetic; there everything is finite and |loss| <= K * 2^-23 (p = q / sum(q), sum(q) within K half-ulps of 1), and the
    assignment's backward is checked with a dense random upstream gradient instead."""
    B, K = CASES[name][:2]
    outs = _abi(name)
    assert all(bool(torch.isfinite(dev).all()) for _, dev, _, _ in outs), name
    if B == 1:
        loss = dict((n, d) for n, d, _, _ in outs)["loss"]
        assert abs(float(loss)) <= K * 2.0 ** -23
    if CASES[name][5]:
        ns = dict((n, d) for n, d, _, _ in outs)["ns"]
        assert float(ns[0, 0]) == 0.0
    for n, err_dev, err_f32 in measure(name, outs):
        print("%-14s %-6s err_dev %.3e err_f32 %.3e" % (name, n, err_dev, err_f32))
        assert _within(err_dev, err_f32), (name, n, err_dev, err_f32)


def _module_run(name, weight=1.0):
    from ssg_amd import dce
    xd, cd = _on_device(name)
    B, K, D = CASES[name][:3]
    m = dce.ClusterAssignment(K, D, cluster_centers=cd.clone())
    x = xd.detach().requires_grad_(True)                                    # (the pitched view keeps its pitch)
    q = m(x)
    loss = dce.kl_loss(q)
    (weight * loss).backward()
    torch.cuda.synchronize()
    return q.detach(), loss.detach(), x.grad, m.cluster_centers.grad


@pytest.mark.parametrize("name", ["workload_s005", "k64_d100", "pitch"])
def test_two_runs_give_the_same_bits(name):
    a, b = _module_run(name), _module_run(name)
    for u, v in zip(a, b):
        assert u.dtype == torch.float32 and torch.equal(u.view(torch.int32), v.view(torch.int32))


CHAIN_CASES = ["workload_s005", "workload_s1", "small_batch", "odd", "k64_d100", "pitch", "ns_zero"]      # (B = 1: exactly 0, see above)


def measure_chain(name):
    """[(output, err_dev, err_f32)] of ClusterAssignment -> kl_loss -> (3 * loss).backward() against 3 x the unit-weight float64 chain;
    err_f32: the float32 chain, times 3.  Here q crosses from the module to the loss as float32, as it does in the torch chain."""
    r = _refs(name)
    q, loss, gx, gc = _module_run(name, 3.0)
    assert q.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32 and gx.shape == r["x"].shape and gc.shape == r["c"].shape
    rows = []
    for n, dev, r64, r32 in (("q", q, r["r64"]["q"], r["r32"]["q"]), ("loss", loss, r["r64"]["loss"], r["r32"]["loss"]),
                             ("gx", gx, 3 * r["r64"]["gx"], 3 * r["r32"]["gx"]), ("gc", gc, 3 * r["r64"]["gc"], 3 * r["r32"]["gc"])):
        rows.append(("chain " + n, dec_ref.rel_err(dev, r64), dec_ref.rel_err(r32, r64)))
    return rows


@pytest.mark.parametrize("name", CHAIN_CASES)
def test_autograd_chain_with_weight_3(name):
    """ClusterAssignment -> kl_loss -> (3 * loss).backward(): q, loss and the gradients that reach the batch and cluster_centers equal
    3 x the unit-weight gradients, under the module's criterion"""
    r = _refs(name)
    for n, err_dev, err_f32 in measure_chain(name):
        print("%-14s %-10s err_dev %.3e err_f32 %.3e" % (name, n, err_dev, err_f32))
        assert _within(err_dev, err_f32), (name, n, err_dev, err_f32)
    # a CPU batch gets its gradient back on the CPU, target_distribution is the p of the loss entry point
    from ssg_amd import dce
    xc = r["x"].clone().requires_grad_(True)
    m = dce.ClusterAssignment(r["c"].shape[0], r["c"].shape[1], cluster_centers=r["c"].clone())
    qc = m(xc)
    dce.kl_loss(qc).backward()
    assert qc.is_cuda and xc.grad.device.type == "cpu" and m.cluster_centers.grad.device.type == "cpu"
    p = dce.target_distribution(qc)
    assert _within(dec_ref.rel_err(p, r["r64"]["p"]), dec_ref.rel_err(r["r32"]["p"], r["r64"]["p"]))


def test_sgd_step_moves_the_parameter_use_device_assignment_kept():
    import ssg_amd
    x, c = _inputs("small_batch")

    class Old(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.cluster_centers = torch.nn.Parameter(c.clone())

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.assignment = Old()

        def forward(self, feats):
            return feats, feats, self.assignment(feats)

    net = Net().cuda()
    par = net.assignment.cluster_centers
    opt = torch.optim.SGD(net.parameters(), lr=1e3)
    ssg_amd.use_device_assignment(net)
    before = par.detach().clone()
    opt.zero_grad()
    loss = ssg_amd.kl_loss(net(x.cuda())[2])
    loss.backward()
    opt.step()
    assert net.assignment.cluster_centers is par and par.is_cuda and par.grad is not None
    assert torch.allclose(par.detach(), before - 1e3 * par.grad, rtol=1e-5, atol=1e-9) and not torch.equal(par.detach(), before)
    assert torch.equal(net.state_dict()["assignment.cluster_centers"], par.detach())
    r = _refs("small_batch")
    assert _within(dec_ref.rel_err(par.grad, r["r64"]["gc"]), dec_ref.rel_err(r["r32"]["gc"], r["r64"]["gc"]))


@pytest.mark.parametrize("precision", ["split", "f32"])
def test_model_returns_the_triple_where_the_reference_does(precision):
    import ssg_amd
    from ssg_amd import _lib
    from ssg_amd._lib import check, ptr, stream
    imgs = torch.randn(3, 3, 64, 32, generator=torch.Generator().manual_seed(7))
    kw = dict(num_classes=0, num_split=1, pretrained=False, seed=2, precision=precision)
    m = ssg_amd.create("resnet50", cluster=True, **kw).cuda().eval()
    plain = ssg_amd.create("resnet50", cluster=False, **kw).cuda().eval()
    ref = plain(imgs)
    assert len(ref) == 2
    centres = m.state_dict()["assignment.cluster_centers"].cuda()
    for for_eval in (False, True):
        out = m(imgs, for_eval)
        assert isinstance(out, tuple) and len(out) == 3
        x1, x2, x3 = out
        assert torch.equal(x1, ref[0]) and torch.equal(x2, ref[1])
        assert x3.shape == (3, 32) and x3.dtype == torch.float32 and x3.is_cuda
        x1c = x1.contiguous()
        q = torch.empty_like(x3)
        check(_lib.lib().ssg_dec_assign_f32(ptr(x1c), 2048, ptr(centres), 3, 32, 2048, 1.0, ptr(q), None, stream()), "ssg_dec_assign_f32")
        assert torch.equal(x3, q)
        q64 = dec_ref.soft_assignment(x1.cpu().double(), centres.cpu().double())[0]
        q32 = dec_ref.soft_assignment(x1.cpu(), centres.cpu())[0]
        assert _within(dec_ref.rel_err(x3, q64), dec_ref.rel_err(q32, q64))
        assert abs(float(x3.sum()) - 3.0) < 1e-5
    assert torch.equal(m.embed_with_flip(imgs), plain.embed_with_flip(imgs))


def test_model_with_splits_keeps_the_eval_path():
    import ssg_amd
    from ssg_amd import evaluators
    imgs = torch.randn(3, 3, 64, 32, generator=torch.Generator().manual_seed(8))
    kw = dict(num_classes=0, num_split=2, pretrained=False, seed=2)
    m = ssg_amd.create("resnet50", cluster=True, **kw).cuda().eval()
    plain = ssg_amd.create("resnet50", cluster=False, **kw).cuda().eval()
    out, ref = m(imgs, True), plain(imgs, True)
    assert len(out) == 2 and out[0].shape == (3, 3 * 2048) and torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])
    assert torch.equal(m.embed_with_flip(imgs), plain.embed_with_flip(imgs))
    assert torch.equal(m.embed_with_flip(imgs, for_eval=True), plain.embed_with_flip(imgs, for_eval=True))
    assert torch.equal(evaluators.extract_cnn_feature(m, imgs, True), evaluators.extract_cnn_feature(plain, imgs, True))
    with pytest.raises(ValueError, match="shape mismatch"):
        m(imgs)


def test_trainer_mixins_vs_the_references_forward(golden):
    """the mixins in front of stand-ins for reid.trainers.FinedTrainer2 / JointTrainer2, on the stub model and criterions of
    tools/make_golden_dec.py (x3 = the device assignment of the stored cases' batches), against the loss and precision the reference's
    own _forward returned in float64; err_f32: the same totals formed in float32 from dec_ref's float32 DEC terms"""
    import ssg_amd
    from ssg_amd import dce
    g = golden("dec_cases.npz")
    tri, glob = tuple(float(v) for v in g["tri"]), tuple(float(v) for v in g["global"])
    qs, kl32 = [], []
    for ci in (int(v) for v in g["trainer_cases"]):
        B, K, D, seed = (int(v) for v in g["case_%d" % ci])
        x, c = dec_ref.case_inputs(B, K, D, seed, float(g["scale_%d" % ci]))
        qs.append(dce.ClusterAssignment(K, D, cluster_centers=c.cuda())(x.cuda()))
        kl32.append(dec_ref.chain(x, c, torch.float32)["loss"])
    tot32 = dec_ref.trainer_totals(kl32[0], kl32[1], torch.tensor(tri[0]), torch.tensor(glob[0]))

    class Base(object):
        def __init__(self, model, criterions, beta=0.5):
            self.model, self.criterions, self.beta = model, criterions, beta

    class Fined(ssg_amd.DECFinedTrainer2Mixin, Base):
        pass

    class Joint(ssg_amd.DECJointTrainer2Mixin, Base):
        pass

    def crit(pair):
        return lambda out, pids, epoch, w=None: (torch.tensor(pair[0], device="cuda"), pair[1])

    def stub_model(as_list):
        calls = []

        def model(imgs):
            q = qs[len(calls) % 2]
            calls.append(1)
            feat = torch.zeros(q.shape[0], 4, device="cuda")
            return ([feat, feat, feat], feat, [q, q * 1.0]) if as_list else (feat, feat, q)
        return model

    pids = [torch.zeros(1, dtype=torch.long)] * 3
    for tag, as_list in (("tensor", False), ("list", True)):
        for who, cls, args in (("fined", Fined, ([None], pids, 0)), ("joint", Joint, ([None], pids, [None], pids[0], 0))):
            loss, prec = cls(stub_model(as_list), [crit(tri), crit(glob)])._forward(*args)
            assert loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32
            ref = float(g["%s_%s_loss" % (who, tag)])
            err_dev, err_f32 = abs(float(loss) - ref) / abs(ref), abs(float(tot32["%s_%s" % (who, tag)]) - ref) / abs(ref)
            print("%s %s: loss %.9e ref %.9e err_dev %.3e err_f32 %.3e" % (who, tag, float(loss), ref, err_dev, err_f32))
            assert _within(err_dev, err_f32), (who, tag, err_dev, err_f32)
            assert prec == float(g["%s_%s_prec" % (who, tag)])
