"""GPU: Type-1 CVAEs with a fully connected bottleneck -- (s) dense tails behind the recognition and prior stacks with a
spatial latent, (v) a vector latent with two linear layers in q_x_y_out and a linear + unflatten in front of p_z_in --
against the float64 oracle and the reference's fixture (tests/golden/dense.npz, make_goldens_dense.py).

Limits are those of tests/test_gpu_cond_net.py for the same quantities: losses 2e-5, x_mu / samples 1e-4, gradients 5e-3
against the fp32 reference and max(4 x float32 noise floor, 5e-3) against the oracle; the dense layers' gradients in full
additionally max(4 x floor, 2e-4) against the oracle.  The noise floors are the fixture's (``floor/<name>``: the oracle's
gradient under four 2^-20 parameter perturbations), so a case needs one oracle pass."""
import copy
import os

import numpy as np
import pytest
import torch

from baryon_painter_amd.utils import synthetic as syn
from golden import make_goldens_dense as DN
from oracle.cvae_oracle import CVAEOracle

import gpu_util as G

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense.npz"))


def _model(arch, **kw):
    from baryon_painter_amd.models.cvae import CVAE
    m = CVAE(arch, "cuda:0", **kw)
    P = DN.parameters({k: tuple(p.shape) for k, p in m.named_parameters()})
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(torch.from_numpy(P[k]))
    m._bump_param_versions()
    return m, P


def _crop_rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((a - ref) ** 2).sum() / (ref ** 2).sum()))


@pytest.mark.parametrize("tag", ["s", "v"])
def test_forward_and_backward_match_oracle_and_reference(tag):
    arch = DN.architectures()[tag]
    m, P = _model(arch)
    assert ",".join(m.state_dict().keys()) == str(GOLD[f"{tag}/state_keys"])
    assert m.count_parameters() == int(GOLD[f"{tag}/n_params"])
    x, y, aux, eps, eps1 = DN.inputs(arch)
    ora = CVAEOracle(arch, dtype=np.float64)
    ora.load_params(P)
    m._eps_override = eps
    m.train(True)
    elbo = m(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
    (-elbo).backward()
    torch.cuda.synchronize()
    ora.forward(x, y, aux, eps)
    g = ora.backward(seed=-1.0)
    # losses
    got = np.array(m.get_stats())
    for ref in (np.array(ora.get_stats()), GOLD[f"{tag}/stats"]):
        print(tag, "stats", got, ref)
        assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max(), (got, ref)
    # x_mu
    xm = m.x_mu.cpu().numpy()
    assert xm.shape == tuple(GOLD[f"{tag}/x_mu_shape"])
    print(tag, "x_mu", G.rel_err(xm, ora.x_mu), _crop_rel_l2(DN.crop(xm), GOLD[f"{tag}/x_mu_crop"]))
    assert G.rel_err(xm, ora.x_mu) < 1e-4
    assert _crop_rel_l2(DN.crop(xm), GOLD[f"{tag}/x_mu_crop"]) <= 1e-4
    assert abs(np.sqrt((xm.astype(np.float64) ** 2).sum()) - GOLD[f"{tag}/x_mu_l2"]) <= 1e-4 * GOLD[f"{tag}/x_mu_l2"]
    assert m.z_mu.shape == (DN.BATCH, *G_latent(arch))
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
    # the dense layers' gradients in full: max(4 x floor, 2e-4) against the oracle, 5e-3 against the reference
    dense = DN.dense_names(arch, names)
    assert len(dense) == {"s": 4, "v": 7}[tag]
    for k in dense:
        eo, er = G.rel_err(grads[k], g[k]), G.rel_err(grads[k], GOLD[f"{tag}/grad/{k}"])
        print(tag, k, "vs oracle", eo, "floor", floor[k], "vs reference", er)
        assert eo <= max(4 * floor[k], 2e-4), k
        assert er <= 5e-3, k
    # sample_P in eval mode: injected eps, then a given z
    m.train(False)
    ora.training = False
    m._eps_override = eps1
    s = m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux)).cpu().numpy()
    assert s.shape == (DN.BATCH, 1, DN.SIZE, DN.SIZE)
    assert G.rel_err(s, ora.sample_P(y, aux, eps=eps1)) < 1e-4
    assert _crop_rel_l2(DN.crop(s), GOLD[f"{tag}/sample_P_crop"]) <= 1e-4
    zfix = syn.synthetic_eps((DN.BATCH, *arch["dim_z"]), seed=101)
    assert zfix.shape == ((DN.BATCH, 12) if tag == "v" else (DN.BATCH, 1, 2, 2))
    s = m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux), z=zfix).cpu().numpy()
    assert G.rel_err(s, ora.sample_P(y, aux, z=zfix)) < 1e-4
    with pytest.raises(ValueError, match="expected"):
        m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux), z=np.zeros((DN.BATCH, 5), np.float32))


def G_latent(arch):
    return tuple(arch["dim_z"]) if len(arch["dim_z"]) == 3 else (arch["dim_z"][0], 1, 1)


@pytest.mark.parametrize("tag", ["s", "v"])
def test_training_step_is_bitwise_reproducible(tag):
    """Three repeats of the same step from the same state give the same bits, and the same bits as the single-stream
    schedule (the linear layers' weight gradients run on the weight-gradient streams like the convolutions')."""
    arch = DN.architectures()[tag]
    m, _ = _model(arch)
    x, y, aux, eps, _ = DN.inputs(arch)
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
    """The procedure of tests/test_gpu_painter.py::test_graphed_train_step_equals_eager_steps on case (v): q_x_y_out's
    dense block runs inside the captured step."""
    from baryon_painter_amd.models.cvae import CVAE
    from baryon_painter_amd.optim import FlatAdam
    tile, n = DN.SIZE, 4
    arch = DN.architectures()["v"]
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
        assert step.last_eps().shape == (1, n, 12)
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


def test_bf16_model_keeps_the_dense_chains_in_fp32():
    """dtype="bf16" builds and trains case (v); the recognition and prior chains -- dense blocks included -- are fp32 in
    both modes, so the KL term, which only they feed, agrees to the fp32 loss limit."""
    arch = DN.architectures()["v"]
    x, y, aux, eps, _ = DN.inputs(arch)
    x, y, aux = (torch.from_numpy(t) for t in (x, y, aux))
    kl = {}
    for dtype in ("f32", "bf16"):
        m, _ = _model(arch, dtype=dtype)
        m._eps_override = eps
        m.train(True)
        elbo = m(x, y, aux)
        (-elbo).backward()
        torch.cuda.synchronize()
        assert np.isfinite(float(elbo.detach())) and all(torch.isfinite(p.grad).all() for p in m.parameters())
        kl[dtype] = float(m.KL_term)
        assert all(not u.bf16 for us in m._last.q_units for u in us) and all(not u.bf16 for u in m._last.p_units)
        assert any(u.bf16 for u in m._last.flat_units(m._last.g_units[1])) == (dtype == "bf16")
    print("KL", kl)
    assert abs(kl["bf16"] - kl["f32"]) <= 2e-5 * abs(kl["f32"])


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
    A = DN.architectures()
    lin = ("linear", {"in_features": 4, "out_features": 4})
    # linear in any other net
    for key in ("q_x_in", "q_y_in", "p_y_in", "p_y_z_in"):
        bad = copy.deepcopy(A["s"])
        bad[key] = list(bad[key] or []) + [("flatten",), lin]
        _refused(bad, NotImplementedError, f"{key}.*linear")
    bad = copy.deepcopy(A["s"])
    bad["p_y_z_out"] = (list(bad["p_y_z_out"][0]) + [("flatten",), lin],)
    _refused(bad, NotImplementedError, r"p_y_z_out\[0\].*p_mu_out\.\d+.*linear")
    # ... in front of a convolution in a tail net, behind one in p_z_in
    bad = copy.deepcopy(A["s"])
    bad["prior_z_y"] = bad["prior_z_y"][9:] + bad["prior_z_y"][:9]
    _refused(bad, NotImplementedError, r"prior_z_y.*prior_network\.1.*in front of a convolution")
    bad = copy.deepcopy(A["v"])
    bad["p_z_in"] = bad["p_z_in"][2:5] + bad["p_z_in"][:2] + bad["p_z_in"][5:]
    _refused(bad, NotImplementedError, r"p_z_in.*behind other layers")
    # linear on an input that is neither flat nor behind flatten
    bad = copy.deepcopy(A["s"])
    bad["q_x_y_out"] = bad["q_x_y_out"][1:]
    _refused(bad, NotImplementedError, "neither flat nor directly behind")
    # tanh / sigmoid / softplus / batchnorm behind a linear layer or behind its unflatten
    for extra in (("tanh",), ("sigmoid",), ("softplus",), ("batchnorm", {"num_features": 24})):
        bad = copy.deepcopy(A["v"])
        bad["q_x_y_out"] = bad["q_x_y_out"] + [extra]                                  # behind the unflatten
        _refused(bad, NotImplementedError, rf"q_x_y_out.*q_out\.5.*{extra[0]}")
        bad = copy.deepcopy(A["v"])
        bad["prior_z_y"] = bad["prior_z_y"][:11] + [extra] + bad["prior_z_y"][11:]      # directly behind the linear
        _refused(bad, NotImplementedError, rf"prior_z_y.*prior_network\.11.*{extra[0]}")
    # data parallelism
    _refused(A["v"], NotImplementedError, "data parallel", sync=object())
    _refused(A["s"], NotImplementedError, "data parallel", sync=object())
    # shapes that do not fit
    bad = copy.deepcopy(A["s"])
    bad["q_x_y_out"][1] = ("linear", {"in_features": 255, "out_features": 8})
    _refused(bad, ValueError, "in_features")
    bad = copy.deepcopy(A["s"])
    bad["q_x_y_out"][1] = ("linear", {"in_features": 256, "out_features": 10})
    _refused(bad, ValueError, "unflatten")
    bad = copy.deepcopy(A["v"])
    bad["p_z_in"] = bad["p_z_in"][2:]
    _refused(bad, ValueError, "p_z_in must begin with a linear")
