"""CPU: the float64 restatements of tests/score_ref.py against ``torch.distributions.Normal(...).log_prob`` in float64,
the identities of the score (the K-draw bound is no lower than the ELBO, K = 1, the range of the effective sample size),
and the refusals of the Python layer that need no GPU."""
import math

import numpy as np
import pytest
import torch

import score_ref as S
from baryon_painter_amd.models import paint_graph as PG

N = 3


def _case(K, dim_z, c, h, w, prior, with_var, seed):
    rng = np.random.Generator(np.random.PCG64([seed, K, c, h]))
    f32 = lambda a: a.astype(np.float32)                                              # noqa: E731
    z = {"z_mu": f32(rng.standard_normal((N, *dim_z))), "z_log_var": f32(rng.standard_normal((N, *dim_z)) - 1.0),
         "p_mu": f32(rng.standard_normal((N, *dim_z)) * prior), "p_log_var": f32(rng.standard_normal((N, *dim_z)) * prior)}
    eps = f32(rng.standard_normal((K, N, *dim_z)))
    x = f32(rng.random((N, c, h, w)) * 2.0)
    x_mu = f32(rng.random((K * N, c, h, w)) * 2.0)
    x_lv = f32(rng.standard_normal((K * N, c, h, w)) - 2.0) if with_var else None
    return z, eps, x, x_mu, x_lv


@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("with_var", [False, True])
def test_loglik_samples_is_the_normal_log_density(K, with_var):
    _, _, x, x_mu, x_lv = _case(K, (1, 2, 2), 2, 6, 10, 1.0, with_var, seed=1)
    ll, mag = S.loglik_samples(x, x_mu, x_lv)
    xt = torch.from_numpy(x).double().repeat(K, 1, 1, 1)
    sd = torch.exp(0.5 * torch.from_numpy(x_lv).double()) if with_var else torch.ones_like(xt)
    ref = torch.distributions.Normal(torch.from_numpy(x_mu).double(), sd).log_prob(xt).sum(dim=(2, 3)).numpy()
    assert ll.shape == mag.shape == (K * N, 2)
    assert (np.abs(ll - ref) <= 1e-12 * mag).all()


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("prior", [0.0, 1.0])
@pytest.mark.parametrize("dim_z", [(1, 2, 2), (8, 1, 1)])
def test_log_ratio_is_the_difference_of_two_normal_log_densities(K, prior, dim_z):
    """... at z = z_mu + eps s_q, with the sampler's standard deviation s = exp(lv / 2) + min_z_var on both sides; without
    a prior network (zero planes) the prior is N(0, (1 + min_z_var)^2)."""
    mzv = 1e-3
    z, eps, *_ = _case(K, dim_z, 1, 2, 2, prior, False, seed=2)
    r, mag = S.log_ratio(z["z_mu"], z["z_log_var"], z["p_mu"], z["p_log_var"], eps, mzv)
    t = {k: torch.from_numpy(v).double() for k, v in z.items()}
    sq, sp = torch.exp(t["z_log_var"] / 2) + mzv, torch.exp(t["p_log_var"] / 2) + mzv
    if prior == 0.0:
        assert bool((sp == 1.0 + mzv).all())
    zk = t["z_mu"][None] + torch.from_numpy(eps).double() * sq[None]
    ref = (torch.distributions.Normal(t["p_mu"], sp).log_prob(zk)
           - torch.distributions.Normal(t["z_mu"], sq).log_prob(zk)).reshape(K, N, -1).sum(dim=2).numpy()
    assert r.shape == (K, N)
    assert (np.abs(r - ref) <= 1e-12 * np.maximum(1.0, mag)).all()


@pytest.mark.parametrize("K", [1, 2, 5, 17, 64])
def test_score_identities(K):
    rng = np.random.Generator(np.random.PCG64([3, K]))
    ll = rng.standard_normal((K, N)) * 50.0 - 1000.0
    ll[:, 1] += 1e4 * np.arange(K)                          # an unshifted logsumexp would overflow
    r = -np.abs(rng.standard_normal((K, N))) * 3.0
    lw = ll + r
    s = S.score(lw, ll, r)
    assert s.shape == (N, 5) and np.isfinite(s).all()
    assert (s[:, 0] >= s[:, 1] - 1e-12 * np.abs(s[:, 1])).all()                   # Jensen: the bound tightens
    assert (s[:, 4] >= 1.0 - 1e-12).all() and (s[:, 4] <= K + 1e-9).all()
    assert np.allclose(s[:, 1], s[:, 2] - s[:, 3], rtol=1e-13, atol=0)
    assert np.array_equal(s[:, 4], S.ess_of(lw))
    if K == 1:
        assert np.array_equal(s[:, 0], s[:, 1]) and np.array_equal(s[:, 0], lw[0]) and (s[:, 4] == 1.0).all()
    else:
        assert abs(s[1, 4] - 1.0) < 1e-9                   # one draw carries all the weight
    # equal weights: ess = K, bound = elbo
    same = S.score(np.full((K, N), -7.0), np.full((K, N), -6.0), np.full((K, N), -1.0))
    assert np.allclose(same[:, 4], K, rtol=1e-12) and np.allclose(same[:, 0], -7.0, rtol=1e-14)
    # all draws at -inf: bound -inf, ess NaN
    dead = S.score(np.full((K, N), -np.inf), np.full((K, N), -np.inf), np.zeros((K, N)))
    assert np.isneginf(dead[:, 0]).all() and np.isnan(dead[:, 4]).all()


def test_log_weights_put_the_parts_together():
    z, eps, x, x_mu, x_lv = _case(4, (1, 2, 2), 2, 6, 10, 1.0, True, seed=4)
    lw, ll_sum, r, mag = S.log_weights(x, x_mu, x_lv, z["z_mu"], z["z_log_var"], z["p_mu"], z["p_log_var"], eps, 1e-7)
    ll, _ = S.loglik_samples(x, x_mu, x_lv)
    assert lw.shape == (4, N) and np.array_equal(lw, ll_sum + r)
    assert np.array_equal(ll_sum[2, 1], ll[2 * N + 1].sum()) and (mag >= np.abs(lw)).all()
    assert S.C0 == -0.5 * math.log(2 * math.pi) and S.COLUMNS == ("bound", "elbo", "log_likelihood", "kl", "ess")


def test_draws_are_checked_without_a_gpu():
    assert PG.check_draws(1) == 1 and PG.check_draws(64) == 64
    for bad in (0, 65, -1, 2.5):
        with pytest.raises(ValueError):
            PG.check_draws(bad)


def test_painter_refusals_need_no_gpu():
    """``CVAEPainter.score`` checks ``draws`` and ``batch_size`` before it touches its model or its transforms, and its
    result keys are the columns of tests/score_ref.py."""
    from baryon_painter_amd import painter as P
    assert P.SCORE_KEYS == S.COLUMNS
    p = P.CVAEPainter.__new__(P.CVAEPainter)                # (no model, no data set: the checks come first)
    tiles = np.zeros((2, 8, 8), np.float32)
    for kw in ({"draws": 0}, {"draws": 65}, {"draws": 3, "batch_size": 8}, {"draws": 16, "batch_size": 8}):
        with pytest.raises(ValueError):
            p.score(tiles, tiles, 0.0, **kw)
