"""Float64 NumPy restatements of the score of a CVAE painter on tiles whose truth is known (the kernels
are csrc/score.hip): the per-sample Gaussian log-density, the log-ratio of prior and posterior at the sampled latent, the
five columns per tile, and a model-level helper that walks ``oracle.torch_ref.TorchRefCVAE`` in eval mode.  Every function
also returns the sum of the magnitudes of the terms it adds, which is what the tests' limits are relative to."""
import math

import numpy as np

C0 = -0.5 * math.log(2.0 * math.pi)
COLUMNS = ("bound", "elbo", "log_likelihood", "kl", "ess")


def loglik_samples(x, x_mu, x_lv=None):
    """ll (K n, c) float64 and the sum of |term| per entry: ``x`` (n, c, H, W), ``x_mu`` (K n, c, H, W) ALREADY
    activated, sample l n + m against x[m]; ``x_lv`` (K n, c, H, W) or None for unit variance.
      term = -log(2 pi)/2 - lv/2 - (x - x_mu)^2 exp(-lv) / 2"""
    x, x_mu = np.asarray(x, np.float64), np.asarray(x_mu, np.float64)
    n = x.shape[0]
    K = x_mu.shape[0] // n
    assert x_mu.shape == (K * n, *x.shape[1:])
    lv = np.zeros_like(x_mu) if x_lv is None else np.asarray(x_lv, np.float64)
    with np.errstate(all="ignore"):
        d = np.tile(x, (K, 1, 1, 1)) - x_mu
        term = C0 - 0.5 * lv - 0.5 * d * d * np.exp(-lv)
    return term.sum(axis=(2, 3)), np.abs(term).sum(axis=(2, 3))


def log_ratio(z_mu, z_log_var, p_mu, p_log_var, eps, min_z_var):
    """r (K, n) = log p(z_k | y) - log q(z_k | x, y) at z_k = z_mu + eps_k s_q, and the sum of |term| per entry, from
    the four planes (n, *dim_z) (zeros for a model without prior network) and ``eps`` (K, n, *dim_z):
      s(lv) = exp(lv / 2) + min_z_var
      term  = log s_q - log s_p + eps^2 / 2 - ((z_mu + eps s_q - p_mu) / s_p)^2 / 2"""
    z_mu, zlv, p_mu, plv = (np.asarray(v, np.float64) for v in (z_mu, z_log_var, p_mu, p_log_var))
    eps = np.asarray(eps, np.float64)
    n = z_mu.shape[0]
    K = eps.shape[0]
    mzv = float(min_z_var)
    sq, sp = np.exp(zlv / 2) + mzv, np.exp(plv / 2) + mzv
    u = (z_mu[None] + eps.reshape(K, *z_mu.shape) * sq[None] - p_mu[None]) / sp[None]
    term = (np.log(sq) - np.log(sp))[None] + 0.5 * eps.reshape(K, *z_mu.shape) ** 2 - 0.5 * u * u
    term = term.reshape(K, n, -1)
    return term.sum(axis=2), np.abs(term).sum(axis=2)


def logsumexp(a, axis=0):
    """Max-subtracted; a maximum that is not finite is not subtracted (all -inf gives -inf, not NaN)."""
    a = np.asarray(a, np.float64)
    with np.errstate(all="ignore"):
        m = a.max(axis=axis, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        return np.squeeze(m, axis) + np.log(np.exp(a - m).sum(axis=axis))


def score(log_w, ll_sum, r):
    """(n, 5) from (K, n) arrays: log w_k, sum_c ll_k[c] and r_k.  Columns: COLUMNS."""
    log_w, ll_sum, r = (np.asarray(v, np.float64) for v in (log_w, ll_sum, r))
    K = log_w.shape[0]
    with np.errstate(all="ignore"):
        lse1, lse2 = logsumexp(log_w), logsumexp(2.0 * log_w)
        return np.stack([lse1 - math.log(K), log_w.mean(axis=0), ll_sum.mean(axis=0), -r.mean(axis=0),
                         np.exp(2.0 * lse1 - lse2)], axis=1)


def ess_of(log_w):
    with np.errstate(all="ignore"):
        return np.exp(2.0 * logsumexp(log_w) - logsumexp(2.0 * np.asarray(log_w, np.float64)))


def log_weights(x, x_mu, x_lv, z_mu, z_log_var, p_mu, p_log_var, eps, min_z_var):
    """(log_w, ll_sum, r, sum of |term|), each (K, n): the definitions above put together."""
    n = np.asarray(x).shape[0]
    ll, ll_abs = loglik_samples(x, x_mu, x_lv)
    K = ll.shape[0] // n
    r, r_abs = log_ratio(z_mu, z_log_var, p_mu, p_log_var, eps, min_z_var)
    ll_sum = ll.sum(axis=1).reshape(K, n)
    return ll_sum + r, ll_sum, r, ll_abs.sum(axis=1).reshape(K, n) + r_abs


def oracle_samples(arch, state, x, y, aux, eps, dtype):
    """The tensors the score is made of from ``oracle.torch_ref.TorchRefCVAE`` in EVAL mode with L = K = eps.shape[0],
    through its ``_seq``, ``_merge`` and ``_P``: a dict of float64 arrays ``z_mu``, ``z_log_var``, ``p_mu``,
    ``p_log_var`` (n, *dim_z), ``x_mu`` (K n, cx, H, W) and ``x_lv`` (or None), computed in ``dtype`` (torch.float64: the
    true values; torch.float32: the CPU twin of the device arithmetic).  ``state``: the model's state_dict as arrays."""
    import torch
    from oracle.torch_ref import TorchRefCVAE, _seq
    params = {k: v for k, v in state.items() if "running_" not in k and "num_batches" not in k}
    ref = TorchRefCVAE(arch, params, {k: v for k, v in state.items() if "running_" in k}, dtype=dtype)
    ref.training = False
    ref.L = int(np.asarray(eps).shape[0])
    a, P = ref.a, ref.P
    dim_z = tuple(arch["dim_z"])
    with torch.no_grad():
        x, y, eps = (torch.as_tensor(np.asarray(v), dtype=dtype) for v in (x, y, eps))
        n = y.shape[0]
        y2 = ref._merge(y, torch.as_tensor(np.asarray(aux), dtype=dtype)) if a["aux_label"] else y
        h = torch.cat([_seq(a["q_x_in"], x, P, "q_x_in.", False), _seq(a["q_y_in"], y2, P, "q_y_in.", False)], 1)
        h = _seq(a["q_x_y_out"], h, P, "q_out.", False).reshape(n, 2, *dim_z)
        z_mu, z_lv = h[:, 0], h[:, 1]
        if "prior_z_y" in a and a["prior_z_y"] is not None:
            hp = _seq(a["prior_z_y"], y2, P, "prior_network.", False).reshape(n, 2, *dim_z)
            p_mu, p_lv = hp[:, 0], hp[:, 1]
        else:
            p_mu, p_lv = torch.zeros_like(z_mu), torch.zeros_like(z_mu)
        z = (z_mu[None] + eps.reshape(ref.L, n, *dim_z) * (torch.exp(z_lv / 2) + ref.min_z_var)[None])
        x_mu, x_lv = ref._P(z.reshape(-1, *dim_z), y2)
    f64 = lambda t: None if t is None else t.detach().to(torch.float64).numpy()       # noqa: E731
    return {"z_mu": f64(z_mu), "z_log_var": f64(z_lv), "p_mu": f64(p_mu), "p_log_var": f64(p_lv), "x_mu": f64(x_mu),
            "x_lv": f64(x_lv), "min_z_var": float(ref.min_z_var)}


def oracle_log_weights(arch, state, x, y, aux, eps, dtype):
    """``log_weights`` of ``oracle_samples``; x and eps enter as the float32 values the device reads."""
    s = oracle_samples(arch, state, x, y, aux, eps, dtype)
    return log_weights(np.asarray(x, np.float32), s["x_mu"], s["x_lv"], s["z_mu"], s["z_log_var"], s["p_mu"],
                       s["p_log_var"], np.asarray(eps, np.float32), s["min_z_var"]) + (s,)
