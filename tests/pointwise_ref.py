"""Float64 NumPy restatements of the streaming, batch-norm, loss-head, paint and optimiser contracts of include/bp_hip.h
(csrc/pointwise.hip, csrc/pointwise_bf16.hip, csrc/paint.hip).

Views are NHWC arrays (n, h, w, c); the NCHW arguments of the C ABI stay NCHW.  Every function evaluates its formula in
float64.  Where a contract rounds an intermediate to float32 (the pre-activation t = fmaf(raw, scale, shift), the sum of
two incoming gradients, a stored gradient), the fp32 forms below round at that point too (``f32_round=True``): those values
are what the kernel's float64 sums add up, so the sums can then be held to float64 accuracy.  The gradients are derived
by hand and pinned to central differences of the float64 forwards in tests/test_pointwise_ref.py, and the batch-norm
coefficient map to oracle.ops.batchnorm_bwd.
"""
import numpy as np

from oracle import ops

U32 = 2.0 ** -24            # unit roundoff of float32
UBF = 2.0 ** -8             # ... of bfloat16


def f32(a):
    """Round to float32, returned as float64."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _ch(v, c):
    return np.asarray(v, np.float64).reshape(c)


# ----------------------------------------------------------------------------------------------- pointwise transform
def pre_act(raw, scale, shift, f32_round=True):
    """t = raw * scale + shift per channel (the fmaf of bp_pointwise: one rounding to float32).  The product of two
    float32 values is exact in float64; the sum is formed in extended precision before the single rounding."""
    c = raw.shape[-1]
    t = np.asarray(raw, np.longdouble) * _ch(scale, c).astype(np.longdouble) + _ch(shift, c).astype(np.longdouble)
    return t.astype(np.float32).astype(np.float64) if f32_round else t.astype(np.float64)


def act(raw, scale, shift, slope, f32_round=True):
    """y = leaky(t, slope) of bp_pointwise; scale None: identity."""
    raw = np.asarray(raw, np.float64)
    if scale is None:
        return raw
    t = pre_act(raw, scale, shift, f32_round)
    y = ops.leaky_relu(t, _ch(slope, raw.shape[-1]))
    return f32(y) if f32_round else y


# ------------------------------------------------------------------------------------------------------ batch norm
def channel_sums(x):
    """{sum x, sum x^2} per channel over every pixel: (2, c)."""
    x = np.asarray(x, np.float64).reshape(-1, x.shape[-1])
    return np.stack([x.sum(axis=0), (x * x).sum(axis=0)])


def bn_finalize(sums, count, gamma=None, beta=None, eps=1e-5, momentum=0.1, running_mean=None, running_var=None):
    """bp_bn_finalize: batch mean, biased variance, scale = gamma*invstd, shift = beta - mean*scale, running
    statistics with the unbiased variance.  Returns a dict of float64 arrays."""
    s0, s1 = np.asarray(sums[0], np.float64), np.asarray(sums[1], np.float64)
    c = s0.size
    g = np.ones(c) if gamma is None else _ch(gamma, c)
    b = np.zeros(c) if beta is None else _ch(beta, c)
    mean = s0 / count
    var = np.maximum(s1 / count - mean * mean, 0.0)
    invstd = 1.0 / np.sqrt(var + np.float64(np.float32(eps)))
    out = dict(mean=mean, invstd=invstd, scale=g * invstd, shift=b - mean * g * invstd)
    m = np.float64(np.float32(momentum))
    if running_mean is not None:
        out["running_mean"] = (1 - m) * _ch(running_mean, c) + m * mean
    if running_var is not None:
        unb = var * (count / (count - 1.0)) if count > 1 else var
        out["running_var"] = (1 - m) * _ch(running_var, c) + m * unb
    return out


def bn_backward_finalize(sums, count, gamma, mean, invstd, pscale=1.0):
    """bp_bn_backward_finalize: from S0 = sum g, S1 = sum g*raw -> dgamma, dbeta (times pscale) and the coefficients
    {A, mg, B, mean} (4, c) of d_raw = A*(g - mg) + B*(raw - mean)."""
    s0, s1 = np.asarray(sums[0], np.float64), np.asarray(sums[1], np.float64)
    c = s0.size
    gm = np.ones(c) if gamma is None else _ch(gamma, c)
    mean, inv = _ch(mean, c), _ch(invstd, c)
    dg = inv * (s1 - mean * s0)                        # sum g * xhat
    coef = np.stack([gm * inv, s0 / count, -gm * inv * inv * dg / count, mean])
    return dict(dgamma=dg * pscale, dbeta=s0 * pscale, coef=coef)


def bn_apply(g, raw, coef):
    """out = A*(g - mg) + B*(raw - mean) per channel."""
    A, G, B, M = (np.asarray(v, np.float64) for v in coef)
    return A * (np.asarray(g, np.float64) - G) + B * (np.asarray(raw, np.float64) - M)


# ------------------------------------------------------------------------------------------- activation backward
def act_backward(dout, raw, scale=None, shift=None, slope=None, dout2=None, act_out=None, f32_round=True):
    """bp_act_backward: d = dout [+ dout2]; t = raw*scale + shift; the sign comes from act_out when given, else from t
    (t == 0 takes the negative branch); g = d * (1 if positive else slope).
    Returns g, sums (3, c) = {sum g, sum g*raw, sum d*t*[not positive]} and mags (3, c), the sums of |term|.
    f32_round: d, t and g rounded to float32 where the fp32 kernels round them."""
    raw = np.asarray(raw, np.float64)
    c = raw.shape[-1]
    d = np.asarray(dout, np.float64)
    if dout2 is not None:
        d = d + np.asarray(dout2, np.float64)
        if f32_round:
            d = f32(d)
    if scale is None:
        t, sl = raw, np.ones(c)
    else:
        t, sl = pre_act(raw, scale, shift, f32_round), _ch(slope, c)
    pos = (np.asarray(act_out, np.float64) if act_out is not None else t) > 0
    g = np.where(pos, d, d * sl)
    if f32_round:
        g = f32(g)
    terms = [g, g * raw, np.where(pos, 0.0, d * t)]
    flat = lambda a: a.reshape(-1, c)
    sums = np.stack([flat(a).sum(axis=0) for a in terms])
    mags = np.stack([np.abs(flat(a)).sum(axis=0) for a in terms])
    return g, sums, mags


def act_bn_backward_apply(dout, raw, coef, scale=None, shift=None, slope=None, dout2=None, act_out=None,
                          f32_round=True):
    g, _, _ = act_backward(dout, raw, scale, shift, slope, dout2, act_out, f32_round)
    return bn_apply(g, raw, coef)


def residual_forward(raw, scale, shift, skip, skip_scale, skip_shift, skip_slope, slope, f32_round=True):
    """bp_residual_forward: out = leaky(raw*scale + shift + act(skip), slope) (the slope of `pw` is not applied)."""
    raw = np.asarray(raw, np.float64)
    c = raw.shape[-1]
    t = raw if scale is None else pre_act(raw, scale, shift, f32_round)
    u = act(skip, skip_scale, skip_shift, skip_slope, f32_round)
    t = t + u
    if f32_round:
        t = f32(t)
    y = np.where(t > 0, t, t * np.float64(np.float32(slope)))
    return f32(y) if f32_round else y


# --------------------------------------------------------------------------------------------------- latent heads
def latent_forward(q_act, eps, L, min_z_var, p_act=None):
    """cvae.py:63-66, 126-130 on the ACTIVATED head outputs q_act / p_act (n, zh, zw, 2*zc): channels [0, zc) are the
    mean, [zc, 2*zc) the log-variance; no prior: standard normal.  eps (L, n, zc, zh, zw).
    Returns stats4 (4, n, zc, zh, zw), z (L*n, zh, zw, zc) and kl_sum (the sum inside cvae.py:129)."""
    q = np.asarray(q_act, np.float64)
    n, zh, zw, c2 = q.shape
    zc = c2 // 2
    nchw = lambda a: a.transpose(0, 3, 1, 2)
    mu, lv = nchw(q[..., :zc]), nchw(q[..., zc:])
    if p_act is None:
        pm, plv = np.zeros_like(mu), np.zeros_like(mu)
    else:
        p = np.asarray(p_act, np.float64)
        pm, plv = nchw(p[..., :zc]), nchw(p[..., zc:])
    pvar = np.exp(plv)
    kl = np.sum((pm - mu) ** 2 / pvar + np.exp(lv) / pvar + plv - lv - 1.0)
    e = np.asarray(eps, np.float64).reshape(L, n, zc, zh, zw)
    z = mu[None] + e * (np.exp(lv / 2.0)[None] + np.float64(np.float32(min_z_var)))
    z = z.reshape(L * n, zc, zh, zw).transpose(0, 2, 3, 1)
    return np.stack([mu, lv, pm, plv]), z, kl


def latent_backward(dz, stats4, eps, L, seed, beta_kl):
    """d(seed * ELBO)/d(activated q head) and /d(p head), with dz = dLoss/dz flowing in: the reparametrisation term
    plus -beta_kl * KL_term, KL_term = 0.5/n * kl_sum.  Returns dq, dp (n, zh, zw, 2*zc)."""
    mu, lv, pm, plv = (np.asarray(a, np.float64) for a in stats4)
    n, zc, zh, zw = mu.shape
    d = np.asarray(dz, np.float64).transpose(0, 3, 1, 2).reshape(L, n, zc, zh, zw)
    e = np.asarray(eps, np.float64).reshape(L, n, zc, zh, zw)
    k = -seed * beta_kl * 0.5 / n
    pvar, dm, ev = np.exp(plv), pm - mu, np.exp(lv)
    dmu = d.sum(axis=0) + k * (-2.0 * dm / pvar)
    dlv = (d * e).sum(axis=0) * 0.5 * np.exp(lv / 2.0) + k * (ev / pvar - 1.0)
    dpm = k * (2.0 * dm / pvar)
    dplv = k * (-dm * dm / pvar - ev / pvar + 1.0)
    nhwc = lambda a, b: np.concatenate([a, b], axis=1).transpose(0, 2, 3, 1)
    return nhwc(dmu, dlv), nhwc(dpm, dplv)


# ------------------------------------------------------------------------------------- Gaussian log-likelihood head
def loglik_forward(x, mu_raw, var_raw, kl_sum, L, mu_softplus, predict_var, alpha_var, beta_kl, likelihood_scaling):
    """cvae.py:132-146.  x NCHW (M, c, h, w); mu_raw / var_raw NHWC (L*M, h, w, c); the mean head ends in torch's
    Softplus(beta=1, threshold=20) when mu_softplus.  Returns x_mu NCHW (L*M, c, h, w), x_log_var (or None) and
    stats = [ELBO, KL_term, log_likelihood[c], fixed_var[c], free_var[c]] (free_var 0 without predict_var)."""
    x = np.asarray(x, np.float64)
    M, c, h, w = x.shape
    raw = np.asarray(mu_raw, np.float64).transpose(0, 3, 1, 2)
    xm = ops.softplus(raw) if mu_softplus else raw
    xr = np.tile(x, (L, 1, 1, 1))                        # x.repeat(L, 1, 1, 1)
    norm = M * L
    c0 = -0.5 * np.log(2 * np.pi)
    fixed = c0 + (-0.5 * (xr - xm) ** 2).sum(axis=(0, 2, 3)) / norm
    lv = None
    if predict_var:
        lv = np.asarray(var_raw, np.float64).transpose(0, 3, 1, 2)
        free = c0 + (-0.5 * lv - 0.5 * (xr - xm) ** 2 / np.exp(lv)).sum(axis=(0, 2, 3)) / norm
        llk = (1 - alpha_var) * fixed + alpha_var * free
    else:
        free = np.zeros(c)
        llk = fixed
    kl = 0.5 / M * kl_sum
    elbo = -kl * beta_kl + likelihood_scaling * llk.sum()
    return xm, lv, np.concatenate([[elbo, kl], llk, fixed, free])


def loglik_backward(x, mu_raw, var_raw, L, seed, mu_softplus, predict_var, alpha_var, likelihood_scaling):
    """d(seed * ELBO)/d mu_raw and /d var_raw, NHWC like the raw heads (d var None without predict_var)."""
    x = np.asarray(x, np.float64)
    M = x.shape[0]
    raw = np.asarray(mu_raw, np.float64)
    xm = ops.softplus(raw) if mu_softplus else raw
    dact = ops.softplus_grad(raw) if mu_softplus else 1.0
    d = np.tile(x, (L, 1, 1, 1)).transpose(0, 2, 3, 1) - xm
    s = seed * likelihood_scaling / (M * L)
    if predict_var:
        xv = np.exp(np.asarray(var_raw, np.float64))
        a = alpha_var
        return s * ((1 - a) * d + a * d / xv) * dact, s * a * (-0.5 + 0.5 * d * d / xv)
    return s * d * dact, None


# ------------------------------------------------------------------------------------------------------ GAN heads
def unary(v, kind):
    """bp_unary_forward on activated input: 0 identity, 1 tanh, 2 sigmoid."""
    v = np.asarray(v, np.float64)
    return {0: v, 1: np.tanh(v), 2: ops.sigmoid(v)}[kind]


def bce_logits(raw, n0, n1, target):
    """sum over samples [n0, n1) of BCE(sigmoid(raw), target) for target 0 or 1: softplus(x) - target*x, computed
    without overflow.  Returns (sum, sum of |term|)."""
    x = np.asarray(raw, np.float64)[n0:n1]
    terms = np.logaddexp(0.0, -x if target > 0.5 else x)
    return terms.sum(), np.abs(terms).sum()


def bce_logits_grad(raw, n0, n1, target, scale):
    """d(scale * bce_logits)/d raw for samples [n0, n1) (other samples: no value)."""
    x = np.asarray(raw, np.float64)[n0:n1]
    return scale * (ops.sigmoid(x) - target)


def l1_sum(fake, x_nchw):
    """sum |fake - x| with fake a view (n, h, w, c) and x NCHW."""
    d = np.asarray(fake, np.float64) - np.asarray(x_nchw, np.float64).transpose(0, 2, 3, 1)
    return np.abs(d).sum()


def tanh_l1_backward(fake, x_nchw, d_fake, l1_scale):
    """d_raw = (d_fake + l1_scale * sign(fake - x)) * (1 - fake^2): the gradient through fake = tanh(raw) of
    sum(d_fake * fake) + l1_scale * sum |fake - x| (sign(0) = 0)."""
    f = np.asarray(fake, np.float64)
    diff = f - np.asarray(x_nchw, np.float64).transpose(0, 2, 3, 1)
    g = (0.0 if d_fake is None else np.asarray(d_fake, np.float64)) + l1_scale * np.sign(diff)
    return g * (1.0 - f * f)


# -------------------------------------------------------------------------------------------------------- paint
def paint_load(raw_nchw, sigma_k, aux=None):
    """bp_paint_load: log(raw / sigma + 1) / k per sample (data_transforms.py:76), then merge_aux_label; NHWC
    (n, h, w, c + caux)."""
    x = np.asarray(raw_nchw, np.float64)
    sk = np.asarray(sigma_k, np.float64).reshape(-1, 2)
    y = np.log(x / sk[:, 0, None, None, None] + 1.0) / sk[:, 1, None, None, None]
    if aux is not None:
        y = ops.merge_aux_label(y, np.asarray(aux, np.float64).reshape(x.shape[0], -1))
    return y.transpose(0, 2, 3, 1)


def paint_store(v, k_sigma, softplus=False):
    """bp_paint_store on the activated head v (n, h, w, c): (exp([softplus](v) * k) - 1) * sigma, NCHW."""
    v = np.asarray(v, np.float64)
    if softplus:
        v = ops.softplus(v)
    ks = np.asarray(k_sigma, np.float64).reshape(-1, 2)
    out = (np.exp(v * ks[:, 0, None, None, None]) - 1.0) * ks[:, 1, None, None, None]
    return out.transpose(0, 3, 1, 2)


# --------------------------------------------------------------------------------------------------------- Adam
def adam(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step):
    """torch.optim.Adam (no weight decay, no amsgrad), one step: returns (param, exp_avg, exp_avg_sq)."""
    p, g = np.asarray(param, np.float64), np.asarray(grad, np.float64)
    m = beta1 * np.asarray(exp_avg, np.float64) + (1 - beta1) * g
    v = beta2 * np.asarray(exp_avg_sq, np.float64) + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    p = p - lr / bc1 * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return p, m, v


# ---------------------------------------------------------------------------------------------------- helpers
def fd_atol(f0, h=1e-6):
    """Rounding error of a central difference of a float64 scalar of size |f0| with step h (8 ulp of f0 over h)."""
    return 8 * 2.0 ** -52 * max(1.0, abs(f0)) / h


def central_diff(f, x, idx, h=1e-6):
    """Central difference of the scalar f at x along the flat coordinates idx (a step relative to |x|)."""
    x = np.array(x, np.float64)
    out = np.empty(len(idx))
    for k, i in enumerate(idx):
        hi = h * max(1.0, abs(x.flat[i]))
        xp, xm = x.copy(), x.copy()
        xp.flat[i] += hi
        xm.flat[i] -= hi
        out[k] = (f(xp) - f(xm)) / (2 * hi)
    return out
