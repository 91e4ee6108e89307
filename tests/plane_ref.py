"""Float64 NumPy restatement of the arithmetic that csrc/plane.hip follows: the cubic-spline zoom of
``scipy.ndimage.zoom(t, tile / cut, order=3, mode="reflect")`` (prefilter + sampling), and the host blend of
``lightcone.paint_plane`` with float64 tile statistics for ``regularise_std``.  Slow and plain on purpose: it pins the
order of operations, so that a test can compare it bit for bit with SciPy and the kernel can be compared with it."""
import numpy as np

Z = np.sqrt(3.0) - 2.0


def prefilter_line(c):
    """In-place cubic B-spline prefilter of one float64 line under half-sample symmetric boundaries."""
    n = len(c)
    if n == 1:
        return
    z = Z
    c *= 6.0                                     # gain (1 - z) (1 - 1/z)
    zn = z ** n
    c0 = c[0]
    s = c[0] + zn * c[n - 1]
    zi = z
    for i in range(1, n):
        if abs(zi) < 1e-18:
            break
        s += zi * (c[i] + zn * c[n - 1 - i])
        zi *= z
    c[0] = s * z / (1.0 - zn * zn) + c0
    for i in range(1, n):
        c[i] += z * c[i - 1]
    c[n - 1] *= z / (z - 1.0)
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])


def prefilter(a):
    """Both axes, axis 0 first (scipy.ndimage.spline_filter's order), in float64."""
    c = np.array(a, dtype=np.float64)
    for j in range(c.shape[1]):
        line = c[:, j].copy()
        prefilter_line(line)
        c[:, j] = line
    for i in range(c.shape[0]):
        line = c[i].copy()
        prefilter_line(line)
        c[i] = line
    return c


def _mirror(i, n):
    i = i % (2 * n)
    return np.where(i >= n, 2 * n - 1 - i, i)


def axis_weights(n_in, n_out):
    """Tap indices (n_out, 4) and cubic B-spline weights (n_out, 4) of one axis."""
    k = np.arange(n_out, dtype=np.float64)
    cc = k * (n_in - 1) / (n_out - 1)
    f = np.floor(cc)
    t = cc - f
    u = 1 - t
    w0 = u * u * u / 6
    w1 = (4 - 6 * t * t + 3 * t * t * t) / 6
    w3 = t * t * t / 6
    w2 = 1 - w0 - w1 - w3
    taps = f.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :]
    return _mirror(taps, n_in), np.stack([w0, w1, w2, w3], axis=1)


def zoom(a, n_out):
    """scipy.ndimage.zoom(a, n_out / a.shape[0], order=3, mode="reflect") of a square array, float64 result."""
    c = prefilter(a)
    n_in = a.shape[0]
    ti, wi = axis_weights(n_in, n_out)
    out = np.zeros((n_out, n_out))
    for p in range(4):                           # taps of axis 0 outer, axis 1 inner, in tap order
        rows = c[ti[:, p]]                       # (n_out, n_in)
        inner = np.zeros((n_out, n_out))
        for q in range(4):
            inner += wi[None, :, q] * rows[:, ti[:, q]]
        out += wi[:, p, None] * inner
    return out


def tile_stats(p):
    """Mean and population standard deviation of a tile, in float64."""
    p = np.asarray(p, np.float64)
    m = p.mean()
    return m, np.sqrt(((p - m) ** 2).mean())


def blend(tiles, dst, n_plane, weight_map, regularise_std=None):
    """The host loop of lightcone.paint_plane on painted float32 tiles with destination origins ``dst`` (n, 2);
    regularise_std uses float64 statistics (tile_stats) instead of NumPy's float32 ones."""
    t = tiles.shape[-1]
    acc, wsum = np.zeros((n_plane, n_plane)), np.zeros((n_plane, n_plane))
    for p, (x, y) in zip(tiles, dst):
        w = weight_map.copy()
        if regularise_std is not None:
            m, s = tile_stats(p)
            w[np.abs(p.astype(np.float64) - m) > s * regularise_std] = 0
        acc[x:x + t, y:y + t] += w * p
        wsum[x:x + t, y:y + t] += w
    with np.errstate(invalid="ignore"):
        return acc / wsum
