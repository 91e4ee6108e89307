"""Float64 NumPy restatement of the split-scale (Gaussian pyramid) transform's contract
(``baryon_painter_amd.utils.data_transforms._SplitScale``, csrc/scales.hip): the weights and the radius of
``scipy.ndimage.gaussian_filter1d``, the folded "reflect" index, axis 0 before axis 1, and the subtraction chain.
Everything stays float64 (no rounding to float32 anywhere): it is the exact value the float32 pipelines approximate.
Plain loops over the taps, slow on purpose."""
import numpy as np

# (n_scale, step_size, include_original) of the fixtures in tests/golden/scales.npz
PARAMS = [(3, 4, True), (3, 4, False), (4, 2, True), (1, 4, False)]
SHAPES = [(16, 16), (24, 40), (64, 64)]


def tile(shape, seed):
    """A float32 test tile with a shift-log-like range: smooth structure plus pixel noise, positive and negative."""
    rng = np.random.Generator(np.random.PCG64([seed, shape[0], shape[1]]))
    yy, xx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    smooth = np.sin(0.37 * yy + 0.5) * np.cos(0.23 * xx - 0.2)
    return (0.6 * smooth + 0.5 * rng.standard_normal(shape) + 0.3).astype(np.float32)


def key(shape, params):
    n_scale, step, inc = params
    return f"{shape[0]}x{shape[1]}_n{n_scale}_s{step}_o{int(inc)}"


def radius(sigma, truncate=3.0):
    return int(truncate * float(sigma) + 0.5)


def weights(sigma, truncate=3.0):
    r = radius(sigma, truncate)
    k = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * k ** 2)
    return phi / phi.sum()


def reflect(i, n):
    """d c b a | a b c d | d c b a: index reflection with period 2n."""
    m = i % (2 * n)
    return 2 * n - 1 - m if m >= n else m


def filter_axis(a, w, axis):
    a = np.moveaxis(np.asarray(a, np.float64), axis, 0)
    n, r = a.shape[0], (len(w) - 1) // 2
    out = np.zeros_like(a)
    for i in range(n):
        for k in range(-r, r + 1):
            out[i] += w[k + r] * a[reflect(i + k, n)]
    return np.moveaxis(out, 0, axis)


def gaussian(a, sigma, truncate=3.0):
    w = weights(sigma, truncate)
    return filter_axis(filter_axis(a, w, 0), w, 1)


def split_scale(x, n_scale, step_size, include_original, truncate=3.0):
    """(levels, H, W) float64: the pyramid of the 2-d tile ``x`` in exact (float64) arithmetic."""
    x = np.asarray(x, np.float64)
    inc = int(bool(include_original))
    d = x.copy()
    out = np.zeros((n_scale + inc, *x.shape))
    if inc:
        out[0] = x
    for i in range(n_scale - 1, 0, -1):
        g = gaussian(d, step_size ** i / 2, truncate)
        out[i + inc] = g
        d = d - g
    out[inc] = d
    return out


def rounding_count(n_scale):
    """T of the limit |float32 pipeline - float64 restatement| <= T * 2^-24 * max|x|, per element, counted from the
    roundings of the contract.  Let e_j bound the error of the residual d_j entering the j-th filtered level
    (j = 1 .. n_scale-1, coarsest first) and M_j = 2^(j-1) max|x| bound |d_j| (a filtered value is a convex
    combination, so |g| <= max|d| and |d - g| <= 2 max|d|), all in units of u = 2^-24 max|x| (half an ulp of a
    float32 value of magnitude <= 2 max|x| is at most 2u; of one <= max|x|, u).
      * filtering carries e_j through unchanged (convex combination) and rounds to float32 twice, once per axis:
        err(g_j) <= e_j + 2 * 2^(j-1)          (|values| <= M_j: half an ulp <= 2^(j-1) u)
      * the float32 subtraction d_(j+1) = d_j - g_j rounds once, on a value <= 2 M_j:
        e_(j+1) <= e_j + err(g_j) + 2^j = 2 e_j + 2^j + 2^j
    with e_1 = 0 (x is exact).  The limit is the largest bound over the channels: the last residual's."""
    e = 0.0
    worst = 0.0
    for j in range(1, n_scale):
        m = 2.0 ** (j - 1)
        eg = e + 2 * m
        e = e + eg + 2 * m
        worst = max(worst, eg, e)
    return worst
