"""Float64 NumPy restatement of ``scipy.ndimage.zoom(a, n_out / n, order=ORDER, mode="mirror")`` for square arrays and
ORDER in {2, 3, 4, 5}, the arithmetic that csrc/ymap.hip follows at every order it has (tests/ymap_ref.py is the
order-3 original and stays the fallback of the order-3 GPU tests): SciPy's poles and gain, the prefilter under
whole-sample symmetric boundaries as a full line with SciPy's closed-form initialisations (once per pole) and as the
kernel's workgroups run it -- pieces of ``CHUNK`` samples staged with a halo on the mirrored extension, every thread
a sub-chunk of ``SUB`` samples, four steps per pole -- and the tensor-product sampling with ORDER + 1 taps per axis.
The constants below are the kernel's own (csrc/ymap.hip: ``Spline<ORDER>``, SUB, CHUNK, SHORT)."""
import numpy as np

ORDERS = (2, 3, 4, 5)
SUB = 32                                          # samples per thread
CHUNK = 224                                       # samples a workgroup finishes per line
SHORT = 32                                        # lines shorter than this take the thread-per-line kernel
WARM = {2: (32,), 3: (32,), 4: (64, 32), 5: (64, 32)}       # warm-up samples per pole
TINY = 1e-18                                      # what a warm-up must have forgotten: |z| ** warm <= TINY


def poles(order):
    """SciPy's closed forms (ni_splines.c, get_filter_poles), evaluated in double."""
    s = np.sqrt
    if order == 2:
        return (s(8.0) - 3.0,)
    if order == 3:
        return (s(3.0) - 2.0,)
    if order == 4:
        return (s(664.0 - s(438976.0)) + s(304.0) - 19.0, s(664.0 + s(438976.0)) - s(304.0) - 19.0)
    if order == 5:
        return (s(67.5 - s(4436.25)) + s(26.25) - 6.5, s(67.5 + s(4436.25)) - s(26.25) - 6.5)
    raise ValueError(order)


def gain(order):
    """prod (1 - z) (1 - 1/z), SciPy's filter_gain.  The cubic's is 6: rounded as written it comes out 6 - 2e-15, and
    the kernel keeps the literal its order-3 form has always had."""
    if order == 3:
        return 6.0
    g = 1.0
    for z in poles(order):
        g *= (1.0 - z) * (1.0 - 1.0 / z)
    return g


def halo(order):
    return sum(WARM[order])


def span(order):
    return halo(order) + CHUNK + halo(order)


def mirror(i, n):
    """Whole-sample symmetric index: i mod 2 (n - 1), then 2 (n - 1) - i above n - 1."""
    p = 2 * (n - 1)
    i = np.asarray(i) % p
    return np.where(i >= n, p - i, i)


def prefilter_lines(c, order):
    """Prefilter along axis 0 of a float64 (n, m) array (every column a line): the gain, then per pole SciPy's causal
    initialisation, the causal recursion, the anti-causal initialisation and the anti-causal recursion."""
    c = np.array(c, dtype=np.float64) * gain(order)
    n = c.shape[0]
    for z in poles(order):
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


def _workgroup(s, zs, warms):
    """The kernel's steps on one staged piece ``s`` (span, m), in place.  Thread g owns the staged samples
    [warms[0] + g SUB, warms[0] + (g + 1) SUB).  The input of a pole is exact on [a, b); its threads run
      A  the causal warm-up over the ``w`` samples before their own (read only), from c+ = x
      B  the causal recursion over their own, in place                        (own within [a + w, b))
      C  the anti-causal warm-up over the ``w`` samples after their own (read only), from z / (z - 1) c+
      D  the anti-causal recursion over their own, in place                   (own within [a + w, b - w))
    and its output is exact on [a + w, b - w).  All threads of a step see what the step before left."""
    n_thr = (s.shape[0] - warms[0]) // SUB
    own = warms[0] + SUB * np.arange(n_thr)
    a, b = 0, s.shape[0]
    for z, w in zip(zs, warms):
        g = own[(own >= a + w) & (own >= warms[0]) & (own + SUB <= b)]
        prev = s[g - w].copy()                                    # A
        for i in range(-w + 1, 0):
            prev = s[g + i] + z * prev
        for i in range(SUB):                                      # B
            prev = s[g + i] + z * prev
            s[g + i] = prev
        g = g[g + SUB + w <= b]
        prev = s[g + SUB + w - 1] * (z / (z - 1.0))               # C
        for i in range(SUB + w - 2, SUB - 1, -1):
            prev = z * (prev - s[g + i])
        for i in range(SUB - 1, -1, -1):                          # D
            prev = z * (prev - s[g + i])
            s[g + i] = prev
        a, b = a + w, b - w


def prefilter_lines_chunked(c, order, warms=None):
    """The same as the kernel's workgroups do it (lines shorter than SHORT take the full-line form).  ``warms``: the
    warm-up per pole in samples, multiples of SUB (default: the kernel's)."""
    n = c.shape[0]
    if n < SHORT:
        return prefilter_lines(c, order)
    warms = WARM[order] if warms is None else tuple(warms)
    h = sum(warms)
    x = np.array(c, dtype=np.float64) * gain(order)
    out = np.empty_like(x)
    for r0 in range(0, n, CHUNK):
        s = x[mirror(np.arange(r0 - h, r0 + CHUNK + h), n)]       # (h + CHUNK + h, m)
        _workgroup(s, poles(order), warms)
        m = min(CHUNK, n - r0)
        out[r0:r0 + m] = s[h:h + m]
    return out


def prefilter(a, order, chunked=False):
    """Both axes, axis 0 first (scipy.ndimage.spline_filter's order)."""
    f = prefilter_lines_chunked if chunked else prefilter_lines
    return np.ascontiguousarray(f(f(np.asarray(a, dtype=np.float64), order).T, order).T)


def bspline_weights(t, order):
    """Centred B-spline of degree ``order`` at the ORDER + 1 tap distances of an offset ``t`` from the middle knot
    (odd orders: t = c - floor(c) in [0, 1); even orders: t = c - floor(c + 0.5) in [-0.5, 0.5)); the last weight is
    one minus the others.  (n_out,) -> (n_out, order + 1)."""
    u = 1.0 - t
    if order == 2:
        w = [0.5 * (0.5 - t) ** 2, 0.75 - t * t]
    elif order == 3:
        w0, w1, w3 = u * u * u / 6, (4 - 6 * t * t + 3 * t * t * t) / 6, t * t * t / 6
        return np.stack([w0, w1, 1 - w0 - w1 - w3, w3], axis=1)
    elif order == 4:
        def mid(y):                                               # 0.5 <= y <= 1.5
            return y * (y * (y * (5.0 - y) / 6.0 - 1.25) + 5.0 / 24.0) + 55.0 / 96.0
        q = t * t
        h = (0.5 - t) ** 2
        w = [h * h / 24.0, mid(1.0 + t), q * (q * 0.25 - 0.625) + 115.0 / 192.0, mid(u)]
    elif order == 5:
        def centre(y):                                            # 0 <= y <= 1
            q = y * y
            return q * (q * (0.25 - y / 12.0) - 0.5) + 0.55

        def mid(y):                                               # 1 <= y <= 2
            return y * (y * (y * (y * (y / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425
        u2 = u * u
        w = [u * u2 * u2 / 120.0, mid(1.0 + t), centre(t), centre(u), mid(1.0 + u)]
    else:
        raise ValueError(order)
    last = 1.0
    for x in w:
        last = last - x
    return np.stack(w + [last], axis=1)


def axis_weights(n_in, n_out, order):
    """Tap indices (n_out, order + 1) and weights (n_out, order + 1) of one axis."""
    k = np.arange(n_out, dtype=np.float64)
    cc = k * ((n_in - 1) / (n_out - 1))                           # SciPy's zoom: k times the rounded ratio
    f = np.floor(cc) if order & 1 else np.floor(cc + 0.5)
    taps = f.astype(np.int64)[:, None] - order // 2 + np.arange(order + 1)[None, :]
    return mirror(taps, n_in), bspline_weights(cc - f, order)


def sample(c, n_out, order):
    """Tensor-product sampling of the coefficients ``c`` (n, n) on the n_out x n_out grid i (n - 1) / (n_out - 1)."""
    ti, wi = axis_weights(c.shape[0], n_out, order)
    out = np.zeros((n_out, n_out))
    for p in range(order + 1):                                    # taps of axis 0 outer, axis 1 inner, in tap order
        rows = c[ti[:, p]]
        inner = np.zeros((n_out, n_out))
        for q in range(order + 1):
            inner += wi[None, :, q] * rows[:, ti[:, q]]
        out += wi[:, p, None] * inner
    return out


def zoom(a, n_out, order, chunked=False):
    """scipy.ndimage.zoom(a, n_out / a.shape[0], order=order, mode="mirror") of a square array, float64 result."""
    return sample(prefilter(a, order, chunked), n_out, order)


def project(planes, scales, resolution, order, y0=None, chunked=False):
    """The loop of lightcone.project_planes with ``zoom`` above in SciPy's place."""
    y = np.zeros((resolution, resolution)) if y0 is None else np.array(y0, dtype=np.float64)
    for d, s in zip(planes, scales):
        d = np.array(d, dtype=np.float64)
        d[np.isnan(d)] = 0
        d *= s
        y += zoom(d, resolution, order, chunked)
    return y
