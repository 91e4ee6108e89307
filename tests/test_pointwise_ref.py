"""CPU: the float64 references of tests/pointwise_ref.py against independent statements of the same operations.

Every hand-derived gradient is compared with central differences of its float64 forward, the batch-norm coefficient map
with oracle.ops.batchnorm_bwd, Adam with torch.optim.Adam.  The GPU tests (test_gpu_pointwise.py) then rest on
references that do not share the kernels' algebra."""
import numpy as np
import pytest
import torch

import pointwise_ref as R
from oracle import ops

RTOL_FD = 1e-6          # central differences with h = 1e-6: truncation O(h^2), rounding O(1e-16 / h)


def _pick(rng, size, k=24):
    return rng.choice(size, size=min(k, size), replace=False)


def test_bn_coefficient_map_matches_oracle_backward():
    rng = np.random.default_rng(1)
    n, h, w, c = 3, 5, 7, 6
    x = rng.standard_normal((n, h, w, c)) * 1.7 + 0.4
    dy = rng.standard_normal((n, h, w, c))
    gamma, beta = rng.uniform(0.5, 1.5, c), rng.uniform(-0.3, 0.3, c)
    fin = R.bn_finalize(R.channel_sums(x), n * h * w, gamma, beta, eps=1e-5)
    _, (xhat, invstd, mean, var) = ops.batchnorm_train_fwd(x.transpose(0, 3, 1, 2), gamma, beta, eps=np.float32(1e-5))
    assert np.allclose(fin["mean"], mean, rtol=1e-13, atol=1e-14)
    assert np.allclose(fin["invstd"], invstd, rtol=1e-11)
    s = np.stack([dy.reshape(-1, c).sum(0), (dy * x).reshape(-1, c).sum(0)])
    bw = R.bn_backward_finalize(s, n * h * w, gamma, fin["mean"], fin["invstd"], pscale=0.5)
    dx = R.bn_apply(dy, x, bw["coef"])
    dx_o, dg_o, db_o = ops.batchnorm_bwd(dy.transpose(0, 3, 1, 2), xhat, invstd, gamma)
    assert np.allclose(dx, dx_o.transpose(0, 2, 3, 1), rtol=1e-10, atol=1e-12)
    assert np.allclose(bw["dgamma"], 0.5 * dg_o, rtol=1e-11)
    assert np.allclose(bw["dbeta"], 0.5 * db_o, rtol=1e-12)


def test_bn_backward_matches_central_differences():
    rng = np.random.default_rng(2)
    n, h, w, c = 2, 4, 5, 3
    x = rng.standard_normal((n, h, w, c)) + 0.3
    dy = rng.standard_normal((n, h, w, c))
    gamma, beta = rng.uniform(0.5, 1.5, c), rng.uniform(-0.3, 0.3, c)
    eps = float(np.float32(1e-5))

    def loss(xx, gg=gamma, bb=beta):
        f = R.bn_finalize(R.channel_sums(xx), n * h * w, gg, bb, eps=eps)
        return float(np.sum(dy * (xx * f["scale"] + f["shift"])))

    fin = R.bn_finalize(R.channel_sums(x), n * h * w, gamma, beta, eps=eps)
    s = np.stack([dy.reshape(-1, c).sum(0), (dy * x).reshape(-1, c).sum(0)])
    bw = R.bn_backward_finalize(s, n * h * w, gamma, fin["mean"], fin["invstd"])
    dx = R.bn_apply(dy, x, bw["coef"])
    idx = _pick(rng, x.size)
    assert np.allclose(dx.flat[idx], R.central_diff(loss, x, idx), rtol=RTOL_FD, atol=1e-8)
    assert np.allclose(bw["dgamma"], R.central_diff(lambda g: loss(x, g), gamma, range(c)), rtol=RTOL_FD, atol=1e-8)
    assert np.allclose(bw["dbeta"], R.central_diff(lambda b: loss(x, gamma, b), beta, range(c)), rtol=RTOL_FD)


def test_bn_finalize_running_statistics():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 3, 3, 2)) * 2 + 1
    rm, rv = np.array([0.1, -0.2]), np.array([1.0, 2.0])
    f = R.bn_finalize(R.channel_sums(x), 36, None, None, eps=1e-5, momentum=0.1, running_mean=rm, running_var=rv)
    m = np.float64(np.float32(0.1))
    assert np.allclose(f["running_mean"], (1 - m) * rm + m * x.mean(axis=(0, 1, 2)), rtol=1e-14)
    assert np.allclose(f["running_var"], (1 - m) * rv + m * x.var(axis=(0, 1, 2), ddof=1), rtol=1e-13)


@pytest.mark.parametrize("with_aout", [False, True])
def test_act_backward_matches_central_differences(with_aout):
    rng = np.random.default_rng(4)
    n, h, w, c = 2, 3, 4, 5
    raw = rng.standard_normal((n, h, w, c))
    scale, shift, slope = rng.uniform(0.5, 1.5, c), rng.uniform(-0.3, 0.3, c), rng.uniform(0.0, 0.3, c)
    dout, dout2 = rng.standard_normal((n, h, w, c)), rng.standard_normal((n, h, w, c))
    t = raw * scale + shift
    skip = rng.standard_normal((n, h, w, c)) if with_aout else 0.0

    def loss(rr=raw, sl=slope):                 # sum (dout + dout2) * leaky(t [+ skip], slope)
        return float(np.sum((dout + dout2) * ops.leaky_relu(rr * scale + shift + skip, sl)))

    a_out = ops.leaky_relu(t + skip, slope) if with_aout else None
    g, sums, mags = R.act_backward(dout, raw, scale, shift, slope, dout2, a_out, f32_round=False)
    # d loss / d t = g; d loss / d raw = g * scale; d loss / d slope = third sum (when the sign is t's own)
    idx = _pick(rng, raw.size)
    assert np.allclose((g * scale).flat[idx], R.central_diff(lambda r: loss(r), raw, idx), rtol=RTOL_FD, atol=1e-9)
    assert np.allclose(sums[0], g.reshape(-1, c).sum(0), rtol=1e-14)
    assert np.allclose(sums[1], (g * raw).reshape(-1, c).sum(0), rtol=1e-13, atol=1e-13)
    assert (mags >= np.abs(sums) - 1e-12).all()
    if not with_aout:
        assert np.allclose(sums[2], R.central_diff(lambda s: loss(raw, s), slope, range(c)), rtol=RTOL_FD, atol=1e-9)


def test_act_backward_mask_edges():
    raw = np.array([[[[0.0, 1.0, -1.0, 2.0]]]])
    scale, shift, slope = np.ones(4), np.array([0.0, -1.0, 0.5, 0.0]), np.full(4, 0.25)
    aout = np.array([[[[1.0, 1.0, 1.0, -1.0]]]])      # opposite sign to t in channels 1 and 3
    dout = np.ones((1, 1, 1, 4))
    g, sums, _ = R.act_backward(dout, raw, scale, shift, slope)
    assert g.ravel().tolist() == [0.25, 0.25, 0.25, 1.0]            # t = 0 takes the negative branch
    g2, _, _ = R.act_backward(dout, raw, scale, shift, slope, act_out=aout)
    assert g2.ravel().tolist() == [1.0, 1.0, 1.0, 0.25]             # act_out's sign wins over t's
    assert sums[2].tolist() == [0.0, 0.0, -0.5, 0.0]


def test_residual_forward_restates_the_tail():
    rng = np.random.default_rng(5)
    c = 4
    raw, skip = rng.standard_normal((2, 3, 3, c)), rng.standard_normal((2, 3, 3, c))
    sc, sf, ksc, ksf, ksl = (rng.uniform(0.5, 1.5, c), rng.uniform(-.2, .2, c), rng.uniform(.5, 1.5, c),
                             rng.uniform(-.2, .2, c), rng.uniform(0, .3, c))
    out = R.residual_forward(raw, sc, sf, skip, ksc, ksf, ksl, 0.2, f32_round=False)
    t = raw * sc + sf + ops.leaky_relu(skip * ksc + ksf, ksl)
    assert np.allclose(out, ops.leaky_relu(t, np.float64(np.float32(0.2))), rtol=1e-15)


@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("L", [1, 2])
def test_latent_matches_central_differences(prior, L):
    rng = np.random.default_rng(6 + L + 2 * prior)
    n, zh, zw, zc = 2, 3, 2, 2
    q = rng.standard_normal((n, zh, zw, 2 * zc)) * 0.5
    p = rng.standard_normal((n, zh, zw, 2 * zc)) * 0.5 if prior else None
    eps = rng.standard_normal((L, n, zc, zh, zw))
    dz = rng.standard_normal((L * n, zh, zw, zc))
    seed, beta, mzv = -1.0, 0.7, 1e-3

    def F(qq, pp=p):        # sum dz * z + seed * ELBO's KL part
        _, z, kl = R.latent_forward(qq, eps, L, mzv, pp)
        return float(np.sum(dz * z) + seed * (-beta * 0.5 / n * kl))

    stats4, z, kl = R.latent_forward(q, eps, L, mzv, p)
    mu, lv = q[..., :zc].transpose(0, 3, 1, 2), q[..., zc:].transpose(0, 3, 1, 2)
    z_nchw = z.transpose(0, 3, 1, 2).reshape(L, n, zc, zh, zw)
    assert np.allclose(z_nchw, mu + eps * (np.exp(lv / 2) + np.float64(np.float32(mzv))), rtol=1e-15)
    dq, dp = R.latent_backward(dz, stats4, eps, L, seed, beta)
    idx = _pick(rng, q.size)
    assert np.allclose(dq.flat[idx], R.central_diff(F, q, idx), rtol=RTOL_FD, atol=1e-9)
    if prior:
        assert np.allclose(dp.flat[idx], R.central_diff(lambda pp: F(q, pp), p, idx), rtol=RTOL_FD, atol=1e-9)
    else:
        assert np.allclose(kl, np.sum(mu ** 2 + np.exp(lv) - lv - 1))


@pytest.mark.parametrize("predict_var,alpha", [(0, 1.0), (1, 0.3), (1, 1.0)])
@pytest.mark.parametrize("L,c", [(1, 1), (2, 2)])
def test_loglik_matches_central_differences(predict_var, alpha, L, c):
    rng = np.random.default_rng(10 + L + c + predict_var)
    M, h, w = 2, 3, 5
    x = rng.standard_normal((M, c, h, w))
    mu = rng.standard_normal((L * M, h, w, c)) * 2
    mu.flat[0] = 21.0                                          # above the softplus threshold
    var = rng.standard_normal((L * M, h, w, c)) * 0.5
    kw = dict(mu_softplus=1, predict_var=predict_var, alpha_var=alpha, likelihood_scaling=1.3)
    seed = -0.8

    def elbo(m, v=var):
        return R.loglik_forward(x, m, v, 4.0, L, beta_kl=0.6, **kw)[2][0]

    xm, lv, st = R.loglik_forward(x, mu, var, 4.0, L, beta_kl=0.6, **kw)
    assert np.isclose(st[1], 0.5 / M * 4.0)
    assert np.isclose(st[0], -st[1] * 0.6 + 1.3 * st[2:2 + c].sum())
    ref_fixed = -0.5 * np.log(2 * np.pi) - 0.5 * ((np.tile(x, (L, 1, 1, 1)) - xm) ** 2).sum(axis=(0, 2, 3)) / (M * L)
    assert np.allclose(st[2 + c:2 + 2 * c], ref_fixed, rtol=1e-13)
    dmu, dvar = R.loglik_backward(x, mu, var, L, seed, **{k: kw[k] for k in kw})
    idx = np.concatenate([[1], _pick(rng, mu.size, 16)])
    idx = idx[idx != 0]
    atol = R.fd_atol(st[0])
    assert np.allclose(dmu.flat[idx], seed * R.central_diff(elbo, mu, idx), rtol=RTOL_FD, atol=atol)
    assert dmu.flat[0] == pytest.approx(seed * 1.3 / (M * L) * (np.tile(x, (L, 1, 1, 1)).transpose(0, 2, 3, 1).flat[0]
                                        - 21.0) * ((1 - alpha) + alpha / np.exp(var.flat[0]) if predict_var else 1.0))
    if predict_var:
        assert np.allclose(dvar.flat[idx], seed * R.central_diff(lambda v: elbo(mu, v), var, idx), rtol=RTOL_FD,
                           atol=atol)


@pytest.mark.parametrize("target", [0.0, 1.0])
def test_bce_matches_central_differences(target):
    rng = np.random.default_rng(20)
    x = rng.standard_normal((4, 3, 3, 2)) * 4
    x[1, 0, 0, 0], x[2, 0, 0, 1] = 25.0, -25.0
    s, m = R.bce_logits(x, 1, 3, target)
    t = torch.from_numpy(x[1:3])
    ref = torch.nn.functional.binary_cross_entropy_with_logits(t, torch.full_like(t, target), reduction="sum")
    assert s == pytest.approx(float(ref), rel=1e-13) and m >= s
    g = R.bce_logits_grad(x, 1, 3, target, 0.3)
    idx = _pick(rng, g.size)
    fd = R.central_diff(lambda xx: 0.3 * R.bce_logits(np.concatenate([x[:1], xx, x[3:]]), 1, 3, target)[0],
                        x[1:3], idx)
    assert np.allclose(g.flat[idx], fd, rtol=RTOL_FD, atol=R.fd_atol(0.3 * s))


def test_tanh_l1_matches_central_differences():
    rng = np.random.default_rng(21)
    raw = rng.standard_normal((2, 3, 4, 2))
    x = rng.standard_normal((2, 2, 3, 4))
    dfake = rng.standard_normal(raw.shape)
    f = np.tanh(raw)

    def F(r):
        fk = np.tanh(r)
        return float(np.sum(dfake * fk) + 0.7 * R.l1_sum(fk, x))

    g = R.tanh_l1_backward(f, x, dfake, 0.7)
    idx = _pick(rng, raw.size)
    assert np.allclose(g.flat[idx], R.central_diff(F, raw, idx), rtol=RTOL_FD, atol=1e-9)
    # diff == 0: sign 0; d_fake None: the L1 term alone
    g0 = R.tanh_l1_backward(f, f.transpose(0, 3, 1, 2), None, 0.7)
    assert not g0.any()


def test_unary_and_paint_transforms():
    rng = np.random.default_rng(22)
    v = rng.standard_normal((2, 3, 3, 2)) * 3
    assert np.allclose(R.unary(v, 1), np.tanh(v)) and np.allclose(R.unary(v, 2), 1 / (1 + np.exp(-v)))
    raw = rng.uniform(0.0, 40.0, (2, 1, 4, 5))
    sk = np.array([[2.0, 4.0], [3.0, 1.5]])
    aux = np.array([[0.5], [1.0]])
    y = R.paint_load(raw, sk, aux)
    assert y.shape == (2, 4, 5, 2)
    assert np.array_equal(y[..., 1], np.broadcast_to(aux[:, :, None], (2, 4, 5)))
    # the store transform with (k, sigma) inverts the load transform
    back = R.paint_store(y[..., :1], sk[:, ::-1])
    assert np.allclose(back, raw, rtol=1e-12, atol=1e-12)
    big = np.full((1, 1, 1, 1), 25.0)
    assert R.paint_store(big, [[1.0, 1.0]], softplus=True)[0, 0, 0, 0] == pytest.approx(np.expm1(25.0), rel=1e-15)


def test_adam_matches_torch():
    rng = np.random.default_rng(23)
    p0, g = rng.standard_normal(50), rng.standard_normal(50)
    p, m, v = p0.copy(), np.zeros(50), np.zeros(50)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    for step in (1, 2, 3):
        tp.grad = torch.from_numpy(g * step)
        opt.step()
        p, m, v = R.adam(p, g * step, m, v, 1e-3, 0.9, 0.999, 1e-8, step)
    assert np.allclose(p, tp.detach().numpy(), rtol=1e-14, atol=1e-15)
    assert np.allclose(v, opt.state[tp]["exp_avg_sq"].numpy(), rtol=1e-14)
