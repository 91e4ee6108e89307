"""Float64 NumPy restatement of ``scipy.ndimage.zoom(a, n_out / n, order=3, mode="mirror")`` for square arrays, the
arithmetic that csrc/ymap.hip follows: the cubic B-spline prefilter under whole-sample symmetric boundaries in two
forms -- the full line with SciPy's closed-form initialisations, and pieces of ``CHUNK`` samples that start ``WARM``
samples early on the mirrored extension, as the kernel's workgroups do -- and the tensor-product sampling.  Plain on
purpose; tests/test_ymap_host.py pins it to SciPy, and the GPU tests fall back to it where SciPy is missing."""
import numpy as np

Z = np.sqrt(3.0) - 2.0
WARM = 32
CHUNK = 224


def mirror(i, n):
    """Whole-sample symmetric index: i mod 2 (n - 1), then 2 (n - 1) - i above n - 1."""
    p = 2 * (n - 1)
    i = np.asarray(i) % p
    return np.where(i >= n, p - i, i)


def prefilter_lines(c):
    """Prefilter along axis 0 of a float64 (n, m) array (every column a line), SciPy's initialisations."""
    c = np.array(c, dtype=np.float64) * 6.0                     # gain (1 - z) (1 - 1/z)
    n = c.shape[0]
    z = Z
    zn = z ** (n - 1)
    c0 = c[0] + zn * c[n - 1]
    zi = z
    for i in range(1, n - 1):
        c0 = c0 + zi * (c[i] + zn * c[n - 1 - i])
        zi *= z
    c[0] = c0 / (1.0 - zn * zn)
    for i in range(1, n):
        c[i] += z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def prefilter_lines_chunked(c, chunk=CHUNK, warm=WARM):
    """The same in pieces of ``chunk`` samples: each piece runs the causal recursion from ``warm`` samples before it to
    ``warm`` samples after it on the mirrored extension, starting from c+ = x, and the anti-causal one back from the
    steady state z / (z - 1) c+.  Lines shorter than ``warm`` take the full-line form."""
    n = c.shape[0]
    if n < warm:
        return prefilter_lines(c)
    x = np.array(c, dtype=np.float64) * 6.0
    out = np.empty_like(x)
    z = Z
    for r0 in range(0, n, chunk):
        idx = mirror(np.arange(r0 - warm, r0 + chunk + warm), n)
        s = x[idx]                                              # (warm + chunk + warm, m)
        for i in range(1, len(s)):
            s[i] += z * s[i - 1]
        prev = s[-1] * (z / (z - 1.0))
        for i in range(len(s) - 2, warm - 1, -1):
            prev = z * (prev - s[i])
            s[i] = prev
        m = min(chunk, n - r0)
        out[r0:r0 + m] = s[warm:warm + m]
    return out


def prefilter(a, chunked=False):
    """Both axes, axis 0 first (scipy.ndimage.spline_filter's order)."""
    f = prefilter_lines_chunked if chunked else prefilter_lines
    return np.ascontiguousarray(f(f(np.asarray(a, dtype=np.float64)).T).T)


def axis_weights(n_in, n_out):
    """Tap indices (n_out, 4) and cubic B-spline weights (n_out, 4) of one axis."""
    k = np.arange(n_out, dtype=np.float64)
    cc = k * ((n_in - 1) / (n_out - 1))                         # SciPy's zoom: k times the rounded ratio
    f = np.floor(cc)
    t = cc - f
    u = 1 - t
    w0 = u * u * u / 6
    w1 = (4 - 6 * t * t + 3 * t * t * t) / 6
    w3 = t * t * t / 6
    w2 = 1 - w0 - w1 - w3
    taps = f.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :]
    return mirror(taps, n_in), np.stack([w0, w1, w2, w3], axis=1)


def sample(c, n_out):
    """Tensor-product sampling of the coefficients ``c`` (n, n) on the n_out x n_out grid i (n - 1) / (n_out - 1)."""
    ti, wi = axis_weights(c.shape[0], n_out)
    out = np.zeros((n_out, n_out))
    for p in range(4):                                          # taps of axis 0 outer, axis 1 inner, in tap order
        rows = c[ti[:, p]]
        inner = np.zeros((n_out, n_out))
        for q in range(4):
            inner += wi[None, :, q] * rows[:, ti[:, q]]
        out += wi[:, p, None] * inner
    return out


def zoom(a, n_out, chunked=False):
    """scipy.ndimage.zoom(a, n_out / a.shape[0], order=3, mode="mirror") of a square array, float64 result."""
    return sample(prefilter(a, chunked), n_out)


def project(planes, scales, resolution, y0=None, chunked=False):
    """The loop of lightcone.project_planes with ``zoom`` above in SciPy's place."""
    y = np.zeros((resolution, resolution)) if y0 is None else np.array(y0, dtype=np.float64)
    for d, s in zip(planes, scales):
        d = np.array(d, dtype=np.float64)
        d[np.isnan(d)] = 0
        d *= s
        y += zoom(d, resolution, chunked)
    return y
