"""GPU: Type-1 CVAEs whose layer lists hold tanh / sigmoid / softplus as layers of their own (graph.UnaryUnit) -- at the
heads, inside every net, writing concat slices, behind a residual block, at the end of a p_y_in network with L = 2 --
against the float64 oracle and the reference's fixture (tests/unary_cases.py, tests/golden/unary.npz).

Limits are those of tests/test_gpu_dense.py for the same quantities: losses and batch-norm running statistics 2e-5,
x_mu / z_mu / z_log_var / samples 1e-4, gradients 5e-3 against the fp32 reference and max(4 x float32 noise floor, 5e-3)
against the oracle; the parameters of the layer directly in front of each saturating layer additionally
max(4 x floor, 2e-4) against the oracle.  The noise floors are the fixture's (``floor/<name>``)."""
import copy
import os

import numpy as np
import pytest
import torch

from baryon_painter_amd.models.graph import ConvUnit, UnaryUnit
from baryon_painter_amd.utils import synthetic as syn
from oracle.cvae_oracle import CVAEOracle

import gpu_util as G
import unary_cases as UC

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unary.npz"))
TAGS = ["heads", "interior", "ytanh"]


def _model(tag, arch, **kw):
    from baryon_painter_amd.models.cvae import CVAE
    m = CVAE(arch, "cuda:0", **kw)
    m.alpha_var = UC.ALPHA_VAR[tag]
    P = UC.parameters({k: tuple(p.shape) for k, p in m.named_parameters()})
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(torch.from_numpy(P[k]))
    m._bump_param_versions()
    return m, P


def _crop_rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((a - ref) ** 2).sum() / (ref ** 2).sum()))


def _units(plan):
    return plan.flat_units([u for us in plan.q_units + [plan.p_units] + plan.g_units
                            + [plan.mu_units, plan.var_units, plan.y_units] for u in us])


@pytest.mark.parametrize("tag", TAGS)
def test_forward_and_backward_match_oracle_and_reference(tag):
    arch = UC.architectures()[tag]
    m, P = _model(tag, arch)
    assert ",".join(m.state_dict().keys()) == str(GOLD[f"{tag}/state_keys"])
    assert m.count_parameters() == int(GOLD[f"{tag}/n_params"])
    x, y, aux, eps, eps1, zfix = UC.inputs(arch)
    ora = CVAEOracle(arch, dtype=np.float64)
    ora.alpha_var = UC.ALPHA_VAR[tag]
    ora.load_params(P)
    m._eps_override = eps
    m.train(True)
    elbo = m(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
    (-elbo).backward()
    torch.cuda.synchronize()
    ora.forward(x, y, aux, eps)
    g = ora.backward(seed=-1.0)
    # the saturating layers are units of the plan, one per layer of the lists (the mean head's trailing softplus excepted)
    plan = m._last
    got_units = sorted(u.name for u in _units(plan) if isinstance(u, UnaryUnit))
    want = sorted(n for n, kind in UC.unary_layers(arch)
                  if not (n.startswith("p_mu_out.") and kind == "softplus"))
    assert got_units == want
    assert plan.mu_softplus == (tag != "heads") and plan.ll.mu_softplus == int(tag != "heads")
    assert plan.mu_head.pw is None and (plan.var_head is None or plan.var_head.pw is None)
    # the epilogue fusions of a producer's batch-norm / activation backward need a ConvUnit on BOTH sides of the slot:
    # none is set up across a unary unit, in either direction
    for u in _units(plan):
        if isinstance(u, ConvUnit) and isinstance(getattr(u.inp, "producer", None), UnaryUnit):
            assert not u._fused_producer and not u._act_producer, u.name
        if isinstance(u, UnaryUnit) and isinstance(getattr(u.inp, "producer", None), ConvUnit):
            assert not u.inp.producer._sums_ready and not u.inp.producer._g_ready, u.name
    # losses
    got = np.array(m.get_stats())
    for ref in (np.array(ora.get_stats()), GOLD[f"{tag}/stats"]):
        print(tag, "stats", got, ref)
        assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max(), (got, ref)
    # batch-norm running statistics after the step, against the reference
    names = str(GOLD[f"{tag}/buffer_names"]).split(",")
    bufs = dict(m.named_buffers())
    off, flat = 0, GOLD[f"{tag}/buffers"]
    for k in names:
        b = bufs[k].detach().cpu().numpy().astype(np.float64).reshape(-1)
        ref = flat[off:off + b.size]
        off += b.size
        assert np.abs(b - ref).max() <= 2e-5 * max(np.abs(ref).max(), 1e-30), k
    assert off == flat.size
    # x_mu and the latent heads
    xm = m.x_mu.cpu().numpy()
    assert xm.shape == tuple(GOLD[f"{tag}/x_mu_shape"])
    print(tag, "x_mu", G.rel_err(xm, ora.x_mu), _crop_rel_l2(UC.crop(xm), GOLD[f"{tag}/x_mu_crop"]))
    assert G.rel_err(xm, ora.x_mu) < 1e-4
    assert _crop_rel_l2(UC.crop(xm), GOLD[f"{tag}/x_mu_crop"]) <= 1e-4
    assert abs(np.sqrt((xm.astype(np.float64) ** 2).sum()) - GOLD[f"{tag}/x_mu_l2"]) <= 1e-4 * GOLD[f"{tag}/x_mu_l2"]
    for name, ours, theirs in (("z_mu", m.z_mu, ora.z_mu), ("z_log_var", m.z_log_var, ora.z_log_var)):
        v = ours.cpu().numpy()
        print(tag, name, G.rel_err(v, theirs), G.rel_err(v, GOLD[f"{tag}/{name}"]))
        assert G.rel_err(v, theirs) < 1e-4 and G.rel_err(v, GOLD[f"{tag}/{name}"]) < 1e-4
    if tag == "heads":
        assert np.abs(xm).max() < 1.0 and (m.x_var.cpu().numpy() >= 1.0).all()        # tanh mean, softplus log-variance
    # every parameter gradient against the oracle, in units of max(4 x stored noise floor, 5e-3)
    grads = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
    assert sorted(grads) == sorted(g)
    floor = {k: float(GOLD[f"{tag}/floor/{k}"]) for k in g}
    errs = sorted(((G.rel_err(grads[k], g[k]) / max(4 * floor[k], 5e-3), k) for k in g), reverse=True)
    print(tag, "worst gradient errors vs float64 oracle, in units of max(4 x noise floor, 5e-3):", errs[:5])
    assert errs[0][0] < 1.0, errs[:4]
    # ... and against the reference's fp32 run, flat 5e-3: the norm of every gradient
    names = str(GOLD[f"{tag}/params"]).split(",")
    worst = sorted(((abs(np.sqrt((grads[k].astype(np.float64) ** 2).sum()) - ref) / ref, k)
                    for k, ref in zip(names, GOLD[f"{tag}/grad_norm"])), reverse=True)
    print(tag, "worst gradient norms vs reference:", worst[:4])
    assert worst[0][0] <= 5e-3, worst[:4]
    # the layers directly in front of a saturating layer: max(4 x floor, 2e-4) against the oracle, and, where the fixture
    # holds the reference's gradient whole, 5e-3 against it
    front = UC.front_names(arch, names)
    assert front
    for k in front:
        eo = G.rel_err(grads[k], g[k])
        er = G.rel_err(grads[k], GOLD[f"{tag}/grad/{k}"]) if f"{tag}/grad/{k}" in GOLD.files else None
        print(tag, k, "vs oracle", eo, "floor", floor[k], "vs reference", er)
        assert eo <= max(4 * floor[k], 2e-4), k
        assert er is None or er <= 5e-3, k
    # sample_P in eval mode: injected eps (the reference has no such sample for L > 1), then a given z
    m.train(False)
    ora.training = False
    m._eps_override = eps1
    s = m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux)).cpu().numpy()
    assert s.shape == (UC.BATCH, 1, UC.SIZE, UC.SIZE)
    assert G.rel_err(s, ora.sample_P(y, aux, eps=eps1)) < 1e-4
    if arch.get("L", 1) == 1:
        assert _crop_rel_l2(UC.crop(s), GOLD[f"{tag}/sample_P_crop"]) <= 1e-4
    s = m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux), z=zfix).cpu().numpy()
    assert G.rel_err(s, ora.sample_P(y, aux, z=zfix)) < 1e-4
    assert _crop_rel_l2(UC.crop(s), GOLD[f"{tag}/sample_P_z_crop"]) <= 1e-4
    if tag == "heads":
        mu, var = m.sample_P(torch.from_numpy(y), return_var=True, aux_label=torch.from_numpy(aux), z=zfix)
        rm, rv = ora.sample_P(y, aux, z=zfix, return_var=True)
        assert G.rel_err(mu.cpu().numpy(), rm) < 1e-4 and G.rel_err(var.cpu().numpy(), rv) < 1e-4
    # the captured paint graph runs the same units
    m._eps_override = None
    sg = m.sample_P_graphed(torch.from_numpy(y), aux_label=torch.from_numpy(aux), z=zfix).cpu().numpy()
    assert np.array_equal(sg, s)


@pytest.mark.parametrize("tag", TAGS)
def test_training_step_is_bitwise_reproducible(tag):
    """Three repeats of the same step from the same state give the same bits, and the same bits as the single-stream
    schedule."""
    arch = UC.architectures()[tag]
    m, _ = _model(tag, arch)
    x, y, aux, eps, _, _ = UC.inputs(arch)
    x, y, aux = (torch.from_numpy(t) for t in (x, y, aux))
    m._eps_override = eps
    state = {k: v.clone() for k, v in m.state_dict().items()}

    def grads():
        m.load_state_dict(state)
        m._bump_param_versions()
        m.zero_grad()
        (-m(x, y, aux)).backward()
        return m._flat_grads.clone()

    ref = grads()
    assert m._last.side is not None
    for _ in range(3):
        assert torch.equal(grads(), ref)
    m.overlap_weight_gradients(False)
    assert torch.equal(grads(), ref)
    m.overlap_weight_gradients(True)


def test_graphed_train_step_equals_eager_steps():
    """The procedure of tests/test_gpu_dense.py::test_graphed_train_step_equals_eager_steps on case ``interior``: eleven
    unary units, forward and backward, run inside the captured step."""
    from baryon_painter_amd.models.cvae import CVAE
    from baryon_painter_amd.optim import FlatAdam
    tile, n = UC.SIZE, 4
    arch = UC.architectures()["interior"]
    torch.manual_seed(3)
    ma = CVAE(arch, "cuda:0")
    mb = CVAE(arch, "cuda:0")
    mb.load_state_dict(ma.state_dict())
    mb._bump_param_versions()
    oa, ob = FlatAdam(ma, lr=1e-3), FlatAdam(mb, lr=1e-3)
    ma.train(True); mb.train(True)
    step = ma.make_graphed_train_step(oa, n)
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(pa, pb), "capturing the graph must not change the training state"
    for it in range(3):
        x, y, aux = syn.synthetic_batch(n, tile, tile, seed=40 + it)
        x, y, aux = torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux)
        if it == 2:
            for o in (oa, ob):
                o.param_groups[0]["lr"] = 3e-4
        elbo_a = step(x, y, aux)
        mb._eps_override = step.last_eps().clone()
        elbo_b = mb(x, y, aux)
        ob.zero_grad()
        (-elbo_b).backward()
        ob.step()
        assert torch.equal(elbo_a.cpu(), elbo_b.detach().cpu())
        assert ma.get_stats() == mb.get_stats()
    assert oa.n_steps == ob.n_steps == 3
    for (ka, pa), (kb, pb) in zip(ma.state_dict().items(), mb.state_dict().items()):
        assert ka == kb and torch.equal(pa, pb), ka
    assert torch.equal(oa.exp_avg, ob.exp_avg) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(pa.grad, pb.grad)
    ma.train(False); mb.train(False)
    z = torch.zeros((n, *arch["dim_z"]))
    assert torch.equal(ma.sample_P(y, aux_label=aux, z=z), mb.sample_P(y, aux_label=aux, z=z))


def test_bf16_model_with_unit_terminated_heads():
    """dtype="bf16" builds and trains case ``heads``: the heads' last convolutions write fp32, so the tanh / softplus units
    behind them read and write fp32 slots.  The recognition and prior chains are fp32 in both modes, so the KL term, which
    only they feed, agrees to the fp32 loss limit (tests/test_gpu_dense.py, the bf16 test)."""
    arch = UC.architectures()["heads"]
    x, y, aux, eps, _, _ = UC.inputs(arch)
    x, y, aux = (torch.from_numpy(t) for t in (x, y, aux))
    kl, xm = {}, {}
    for dtype in ("f32", "bf16"):
        m, _ = _model("heads", arch, dtype=dtype)
        m._eps_override = eps
        m.train(True)
        elbo = m(x, y, aux)
        (-elbo).backward()
        torch.cuda.synchronize()
        assert np.isfinite(float(elbo.detach())) and all(torch.isfinite(p.grad).all() for p in m.parameters())
        kl[dtype], xm[dtype] = float(m.KL_term), m.x_mu.cpu().numpy()
        plan = m._last
        assert any(u.bf16 for u in plan.flat_units(plan.g_units[1])) == (dtype == "bf16")
        heads = [u for u in plan.mu_units + plan.var_units if isinstance(u, UnaryUnit)]
        assert [u.name for u in heads] == ["p_mu_out.5", "p_var_out.5"]
        assert all(u.inp.dt == 0 and u.out.dt == 0 for u in heads)
        assert np.abs(xm[dtype]).max() < 1.0
    print("KL", kl, "x_mu f32 vs bf16", G.rel_err(xm["bf16"], xm["f32"]))
    assert abs(kl["bf16"] - kl["f32"]) <= 2e-5 * abs(kl["f32"])


def test_bf16_model_with_a_unit_on_a_heads_inner_fp32_slot():
    """dtype="bf16": the slot behind a head's SECOND convolution is fp32 (``_Plan.bf16_out_of``), so a unit may stand
    there; behind the first convolution it is refused (test_refusals_come_before_any_device_allocation).  The unit reads
    and writes fp32, the step is finite, the head's first convolution receives a gradient through the unit, and the KL
    term agrees with the fp32 build as in the test above.  (How far a bf16 trunk moves x_mu is printed, not judged: no
    test of the bf16 mode sets a limit for it.)"""
    arch = copy.deepcopy(UC.architectures()["heads"])
    mu, var = arch["p_y_z_out"]
    arch["p_y_z_out"] = (mu[:4] + [("sigmoid",)] + mu[4:], var)
    x, y, aux, eps, _, _ = UC.inputs(arch)
    x, y, aux = (torch.from_numpy(t) for t in (x, y, aux))
    kl, xm = {}, {}
    for dtype in ("f32", "bf16"):
        m, _ = _model("heads", arch, dtype=dtype)
        m._eps_override = eps
        m.train(True)
        elbo = m(x, y, aux)
        (-elbo).backward()
        torch.cuda.synchronize()
        assert np.isfinite(float(elbo.detach())) and all(torch.isfinite(p.grad).all() for p in m.parameters())
        kl[dtype], xm[dtype] = float(m.KL_term), m.x_mu.cpu().numpy()
        units = [u for u in m._last.mu_units if isinstance(u, UnaryUnit)]
        assert [u.name for u in units] == ["p_mu_out.4", "p_mu_out.6"]
        assert all(u.inp.dt == 0 and u.out.dt == 0 for u in units)
        assert float(m.get_parameter("p_mu_out.0.weight").grad.abs().max()) > 0
    print("KL", kl, "x_mu f32 vs bf16", G.rel_err(xm["bf16"], xm["f32"]))
    assert abs(kl["bf16"] - kl["f32"]) <= 2e-5 * abs(kl["f32"])


def test_units_first_in_a_net():
    """A unit as the first layer of a net, where the plan treats the first layer specially.  On data (q_x_in, prior_z_y:
    no gradient is wanted, and the convolution behind the unit computes none either), and on the generator's
    concatenated input p_in (p_y_z_in: the gradient of its h_z slice reaches p_z_in through the wide buffer, not through
    the dense buffer that a first CONVOLUTION restricted to those channels writes).  Against the float64 oracle, with the
    limits of the cases above: losses 2e-5, x_mu / z_mu / z_log_var 1e-4, every parameter gradient max(4 x noise floor,
    5e-3), p_z_in's -- which only h_z's gradient feeds -- max(4 x floor, 2e-4).  No fixture holds this case, so its noise
    floors are computed here as the generator computes them (``unary_cases.noise_floors``)."""
    arch = copy.deepcopy(UC.architectures()["heads"])
    arch["q_x_in"] = [("sigmoid",)] + list(arch["q_x_in"])
    arch["prior_z_y"] = [("tanh",)] + list(arch["prior_z_y"])
    arch["p_y_z_in"] = [("tanh",)] + list(arch["p_y_z_in"])
    m, P = _model("heads", arch)
    x, y, aux, eps, _, _ = UC.inputs(arch)
    ora = CVAEOracle(arch, dtype=np.float64)
    ora.alpha_var = UC.ALPHA_VAR["heads"]
    ora.load_params(P)
    m._eps_override = eps
    m.train(True)
    (-m(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))).backward()
    torch.cuda.synchronize()
    ora.forward(x, y, aux, eps)
    g = ora.backward(seed=-1.0)
    plan = m._last
    for us in (plan.q_units[0], plan.p_units):
        assert isinstance(us[0], UnaryUnit) and not us[0].need_dgrad and us[0].out.grad is None
        assert isinstance(us[1], ConvUnit) and not us[1].need_dgrad
    first = plan.g_units[1][0]
    assert isinstance(first, UnaryUnit) and first.name == "p_y_z_in.0" and first.need_dgrad
    got, ref = np.array(m.get_stats()), np.array(ora.get_stats())
    assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max(), (got, ref)
    for name, ours, theirs in (("x_mu", m.x_mu, ora.x_mu), ("z_mu", m.z_mu, ora.z_mu),
                               ("z_log_var", m.z_log_var, ora.z_log_var)):
        print(name, G.rel_err(ours.cpu().numpy(), theirs))
        assert G.rel_err(ours.cpu().numpy(), theirs) < 1e-4
    grads = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
    assert sorted(grads) == sorted(g)
    floor = UC.noise_floors(arch, P, x, y, aux, eps, g, UC.ALPHA_VAR["heads"])
    errs = sorted(((G.rel_err(grads[k], g[k]) / max(4 * floor[k], 5e-3), k) for k in g), reverse=True)
    print("worst gradient errors vs float64 oracle, in units of max(4 x noise floor, 5e-3):", errs[:5])
    assert errs[0][0] < 1.0, errs[:4]
    for k in g:
        if k.startswith("p_z_in."):
            assert G.rel_err(grads[k], g[k]) <= max(4 * floor[k], 2e-4), k


def _refused(arch, exc, match, **kw):
    """``CVAE(arch)`` raises ``exc`` without allocating device memory."""
    from baryon_painter_amd.models.cvae import CVAE
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(exc, match=match):
        CVAE(arch, "cuda:0", **kw)
    assert torch.cuda.memory_allocated() == before


def test_refusals_come_before_any_device_allocation():
    torch.zeros(1, device="cuda")                     # (the context exists)
    A = UC.architectures()
    # a bf16 model with a saturating layer inside the generator trunk, or inside a head in front of its last convolution
    _refused(A["interior"], NotImplementedError, r"p_y_z_in\.2.*sigmoid.*bf16", dtype="bf16")
    bad = copy.deepcopy(A["heads"])
    mu, var = bad["p_y_z_out"]
    bad["p_y_z_out"] = (mu[:2] + [("tanh",)] + mu[2:], var)
    _refused(bad, NotImplementedError, r"p_mu_out\.2.*tanh.*bf16", dtype="bf16")
    # inside a residual block's branch
    bad = copy.deepcopy(A["heads"])
    i = [k for k, layer in enumerate(bad["p_y_z_in"]) if layer[0] == "residual block"][0]
    body, tail = bad["p_y_z_in"][i][1]
    bad["p_y_z_in"][i] = ("residual block", (body[:3] + [("softplus",)] + body[3:], tail))
    _refused(bad, NotImplementedError, rf"p_y_z_in\.{i}\.res_block\.3.*softplus")
