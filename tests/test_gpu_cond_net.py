"""GPU: Type-1 CVAEs with a p_y_in network (L = 1 and L = 2) and without a prior network -- forward, losses, every
parameter gradient and p_y_in's running statistics against the float64 oracle and the reference's fixture
(tests/golden/cond_net.npz); the repeat-over-L kernel and its adjoint; sampling the standard-normal prior.

Tolerances are those of tests/test_gpu_model.py for the same quantities: losses 2e-5, x_mu / samples 1e-4, gradients
5e-3 against the fp32 reference and max(4 x float32 noise floor, 5e-3) against the oracle, running statistics 2e-5.
The three cases are well conditioned (softened activations around a ReLU p_y_in: the noise floors are 1e-3 class)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from baryon_painter_amd import _lib as L
from baryon_painter_amd.utils import synthetic as syn
from golden import make_goldens_cond_net as CN
from golden_util import check
from oracle.cvae_oracle import CVAEOracle

import gpu_util as G

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cond_net.npz"))


def _model(arch):
    from baryon_painter_amd.models.cvae import CVAE
    m = CVAE(arch, "cuda:0")
    P = CN.parameters({k: tuple(p.shape) for k, p in m.named_parameters()})
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(torch.from_numpy(P[k]))
    return m, P


def _crop_rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((a - ref) ** 2).sum() / (ref ** 2).sum()))


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_forward_and_backward_match_oracle_and_reference(tag):
    arch = CN.architectures()[tag]
    m, P = _model(arch)
    assert ",".join(m.state_dict().keys()) == str(GOLD[f"{tag}/state_keys"])
    assert m.count_parameters() == int(GOLD[f"{tag}/n_params"])
    x, y, aux, eps, eps1 = CN.inputs(arch)
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
    print(tag, "x_mu", G.rel_err(xm, ora.x_mu), _crop_rel_l2(CN.crop(xm), GOLD[f"{tag}/x_mu_crop"]))
    assert G.rel_err(xm, ora.x_mu) < 1e-4
    assert _crop_rel_l2(CN.crop(xm), GOLD[f"{tag}/x_mu_crop"]) <= 1e-4
    assert abs(np.sqrt((xm.astype(np.float64) ** 2).sum()) - GOLD[f"{tag}/x_mu_l2"]) <= 1e-4 * GOLD[f"{tag}/x_mu_l2"]
    # every parameter gradient against the oracle: the float32 noise floor of tests/test_gpu_model.py
    # (test_batch_sizes_L_and_eval_mode_against_oracle): how far the TRUE gradient moves under 2^-20 perturbations
    floor = {k: 0.0 for k in g}
    rng = np.random.default_rng(7)
    for _ in range(4):
        pert = CVAEOracle(arch, dtype=np.float64)
        pert.load_params({k: np.asarray(v, np.float64) * (1.0 + 2.0 ** -20 * rng.uniform(-1, 1, np.shape(v)))
                          for k, v in P.items()})
        pert.forward(x, y, aux, eps)
        gp = pert.backward(seed=-1.0)
        for k in g:
            floor[k] = max(floor[k], G.rel_err(gp[k], g[k]))
    grads = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
    assert sorted(grads) == sorted(g)
    errs = sorted(((G.rel_err(grads[k], g[k]) / max(4 * floor[k], 5e-3), k) for k in g), reverse=True)
    print(tag, "worst gradient errors vs float64 oracle, in units of max(4 x noise floor, 5e-3):", errs[:5])
    assert errs[0][0] < 1.0, errs[:4]
    # ... and against the reference's fp32 run, flat 5e-3 (tests/test_gpu_model.py against the fp32 reference): the norm
    # of every gradient and p_y_in's gradients in full.  The cases are the well-conditioned ones of
    # make_goldens_cond_net.architectures(); the reference's own gradients lie within 4e-5 of the float64 truth there.
    names = str(GOLD[f"{tag}/params"]).split(",")
    worst = sorted(((abs(np.sqrt((grads[k].astype(np.float64) ** 2).sum()) - ref) / ref, k)
                    for k, ref in zip(names, GOLD[f"{tag}/grad_norm"])), reverse=True)
    print(tag, "worst gradient norms vs reference:", worst[:4])
    assert worst[0][0] <= 5e-3, worst[:4]
    y_names = [k for k in names if k.startswith("p_y_in.")]
    assert (tag != "c") == bool(y_names)
    for k in y_names:
        print(tag, k, "vs reference", check(f"{tag}/grad/{k}", grads[k], GOLD, 5e-3, what="grad "),
              "vs oracle", G.rel_err(grads[k], g[k]), "floor", floor[k])
    # batch-norm running statistics of p_y_in after the step (statistics over n samples, whatever L is)
    for k, b in m.named_buffers():
        if k.startswith("p_y_in."):
            check(f"{tag}/buf/{k}", b.cpu().numpy(), GOLD, 2e-5)
            assert G.rel_err(b.cpu().numpy(), ora.P[k]) <= 2e-5, k
    # sample_P in eval mode: one latent draw per input whatever L is
    m.train(False)
    ora.training = False
    m._eps_override = eps1
    s = m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux)).cpu().numpy()
    assert s.shape == (CN.BATCH, 1, CN.SIZE, CN.SIZE)
    assert G.rel_err(s, ora.sample_P(y, aux, eps=eps1)) < 1e-4
    if f"{tag}/sample_P_crop" in GOLD:
        assert _crop_rel_l2(CN.crop(s), GOLD[f"{tag}/sample_P_crop"]) <= 1e-4
    zfix = syn.synthetic_eps((CN.BATCH, *arch["dim_z"]), seed=101)
    s = m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux), z=zfix).cpu().numpy()
    assert G.rel_err(s, ora.sample_P(y, aux, z=zfix)) < 1e-4


def test_training_step_is_bitwise_reproducible_with_p_y_in_beside_the_encoders():
    """p_y_in runs on the weight-gradient stream during the forward pass: the same step from the same state gives the
    same bits, and the same bits as the single-stream schedule."""
    arch = CN.architectures()["b"]
    m, _ = _model(arch)
    x, y, aux, eps, _ = CN.inputs(arch)
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
    assert m._last.y_beside and m._last.hy_one is not None
    for _ in range(3):
        assert torch.equal(grads(), ref)
    m.overlap_weight_gradients(False)
    assert torch.equal(grads(), ref)
    m.overlap_weight_gradients(True)


# ---------------------------------------------------------------- repeat over L and its adjoint
# channel offset 1 of a stride-7 buffer (one float per access) and an aligned slice (16-byte accesses)
@pytest.mark.parametrize("c,cs_src,co_src,cs_dst,co_dst", [(3, 7, 1, 7, 1), (4, 4, 0, 8, 4), (4, 8, 4, 4, 0), (2, 7, 1, 8, 4)])
def test_repeat_over_L_and_adjoint(c, cs_src, co_src, cs_dst, co_dst):
    lib = L.load()
    Ls, n, h, w = 3, 2, 8, 8
    rng = np.random.default_rng(5)
    src = rng.standard_normal((n, c, h, w)).astype(np.float32)
    sbuf, sv = G.to_nhwc(src, cs_src, co_src)
    dbuf = torch.full((Ls * n, h, w, cs_dst), -3.25, dtype=torch.float32, device="cuda")
    dv = L.View(dbuf.data_ptr(), Ls * n, h, w, c, cs_dst, co_dst)
    L.check(lib.bp_repeat_samples(C.byref(sv), Ls, C.byref(dv), G.stream()), "repeat")
    got = dbuf.cpu().numpy()
    assert np.array_equal(G.from_nhwc(dbuf, c, co_dst), np.tile(src, (Ls, 1, 1, 1)))            # exact, order l * n + m
    other = np.ones(cs_dst, bool)
    other[co_dst:co_dst + c] = False
    assert (got[..., other] == -3.25).all()                                                  # nothing else is touched
    # adjoint: d_src[m] = (d[m] + d[n + m]) + d[2 n + m] in float32
    d = rng.standard_normal((Ls * n, c, h, w)).astype(np.float32)
    gbuf, gv = G.to_nhwc(d, cs_dst, co_dst)
    obuf = torch.full((n, h, w, cs_src), 9.5, dtype=torch.float32, device="cuda")
    ov = L.View(obuf.data_ptr(), n, h, w, c, cs_src, co_src)
    L.check(lib.bp_repeat_samples_adjoint(C.byref(gv), Ls, C.byref(ov), G.stream()), "adjoint")
    ref = d[:n].copy()
    for l in range(1, Ls):
        ref = ref + d[l * n:(l + 1) * n]
    assert np.array_equal(G.from_nhwc(obuf, c, co_src), ref)
    other = np.ones(cs_src, bool)
    other[co_src:co_src + c] = False
    assert (obuf.cpu().numpy()[..., other] == 9.5).all()
    # shapes that do not fit are refused before anything is written
    bad = L.View(dbuf.data_ptr(), Ls * n + 1, h, w, c, cs_dst, co_dst)
    assert lib.bp_repeat_samples(C.byref(sv), Ls, C.byref(bad), G.stream()) == L.BP_EINVAL
    assert lib.bp_repeat_samples_adjoint(C.byref(gv), 0, C.byref(ov), G.stream()) == L.BP_EINVAL


# ---------------------------------------------------------------- standard-normal sampling
@pytest.mark.parametrize("Ls", [1, 2])
def test_latent_forward_without_a_source_samples_the_standard_normal(Ls):
    lib = L.load()
    n, zc, zh, zw, mzv = 3, 2, 3, 5, 1e-3
    lt = L.Latent(n, Ls, zc, zh, zw, mzv)
    rng = np.random.default_rng(9)
    eps = rng.standard_normal((Ls, n, zc, zh, zw)).astype(np.float32)
    eps[0, 0, 0, 0, :2] = (0.0, -0.0)
    ed = G.dev(eps)
    st4 = torch.full((4, n, zc, zh, zw), float("nan"), device="cuda")
    zbuf, zv = G.empty_nhwc(Ls * n, zh, zw, zc)
    kl = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.zeros(256, dtype=torch.float64, device="cuda")
    L.check(lib.bp_latent_forward(C.byref(lt), None, None, None, None, L.ptr(ed), L.ptr(st4), C.byref(zv), L.ptr(kl),
                                  L.ptr(ws), ws.numel() * 8, G.stream()), "latent forward")
    ref = eps * (np.float32(1.0) + np.float32(mzv))                  # float32: eps * (1 + min_z_var)
    got = G.from_nhwc(zbuf, zc).reshape(Ls, n, zc, zh, zw)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), ref.view(np.int32))      # bitwise
    assert (st4.cpu().numpy() == 0).all() and float(kl) == 0.0
    # a prior head without a sample source has no meaning
    pbuf, pv = G.empty_nhwc(n, zh, zw, 2 * zc)
    assert lib.bp_latent_forward(C.byref(lt), None, None, C.byref(pv), None, L.ptr(ed), L.ptr(st4), C.byref(zv),
                                 L.ptr(kl), L.ptr(ws), ws.numel() * 8, G.stream()) == L.BP_EINVAL
