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


def exact_prefilter_line(s):
    """The spline coefficients of one line by a dense solve of (c[k-1] + 4 c[k] + c[k+1]) / 6 = s[k] with
    c[-1] = c[0] and c[n] = c[n-1] (half-sample symmetric boundaries).  For pinning prefilter_line only."""
    s = np.asarray(s, np.float64)
    n = len(s)
    if n == 1:
        return s.copy()
    m = np.zeros((n, n))
    for k in range(n):
        m[k, k] += 4.0
        m[k, max(k - 1, 0)] += 1.0
        m[k, min(k + 1, n - 1)] += 1.0
    return np.linalg.solve(m / 6.0, s)


def prefilter(a):
    """Both axes, axis 0 first (scipy.ndimage.spline_filter's order), in float64.  prefilter_line runs on all the
    lines of an axis at once (c[i] is then a row of elements, one per line, and every operation is elementwise), which
    leaves each line's operations and their order as they are."""
    c = np.array(a, dtype=np.float64)
    prefilter_line(c)                            # lines along axis 0
    c = np.ascontiguousarray(c.T)
    prefilter_line(c)                            # lines along axis 1
    return np.ascontiguousarray(c.T)


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


RB = 256                                         # tile_stats_kernel's workgroup


def _device_sum(v):
    """tile_stats_kernel's fixed-order sum of a float64 vector: partial sum k adds v[k], v[k + 256], ... in turn from
    0.0, then the halving tree red[i] += red[i + h], h = 128 ... 1."""
    red = np.zeros(RB)
    for a in range(0, len(v), RB):
        part = v[a:a + RB]
        red[:len(part)] = red[:len(part)] + part
    h = RB // 2
    while h > 0:
        red[:h] = red[:h] + red[h:2 * h]
        h //= 2
    return red[0]


def device_tile_stats(p):
    """Mean and population standard deviation of a tile as tile_stats_kernel (csrc/plane.hip) sums them, in float64:
    its strided partial sums and halving tree for the mean, then the same over (p - mean)^2."""
    p = np.asarray(p, np.float64).ravel()
    tt = float(len(p))
    with np.errstate(invalid="ignore", over="ignore"):
        mean = _device_sum(p) / tt
        d = p - mean
        return mean, np.sqrt(_device_sum(d * d) / tt)


def blend_box(tiles, dst, rows, cols, weight, box, acc0, wsum0, stats=None, regularise_std=None):
    """blend_kernel (csrc/plane.hip) pixel by pixel: over the pixels of box = (bx0, by0, bx1, by1) only, the tiles
    (n, tile, tile) in ascending t, a += w * p then s += w in float64 with the product and the sum rounded separately,
    starting from the prior content acc0 / wsum0 (rows, cols).  Tiles may lie partly or wholly outside the plane or the
    box.  regularise_std: w = 0 where |p - mean| > std * regularise_std with stats[t] = (mean, std), by default
    device_tile_stats of the tile (a comparison with a NaN is false: the weight is kept).  Returns (acc, wsum)."""
    t = tiles.shape[-1]
    bx0, by0, bx1, by1 = box
    assert 0 <= bx0 < bx1 <= rows and 0 <= by0 < by1 <= cols
    acc, wsum = np.array(acc0, np.float64), np.array(wsum0, np.float64)
    assert acc.shape == wsum.shape == (rows, cols)
    for k, (p, (x, y)) in enumerate(zip(tiles, dst)):
        x, y = int(x), int(y)
        p = p.astype(np.float64)
        w = np.array(weight, np.float64)
        if regularise_std is not None:
            m, s = device_tile_stats(p) if stats is None else stats[k]
            with np.errstate(invalid="ignore"):
                w[np.abs(p - m) > s * regularise_std] = 0.0
        x0, x1, y0, y1 = max(x, bx0), min(x + t, bx1), max(y, by0), min(y + t, by1)
        if x0 >= x1 or y0 >= y1:
            continue
        ws, ps = w[x0 - x:x1 - x, y0 - y:y1 - y], p[x0 - x:x1 - x, y0 - y:y1 - y]
        with np.errstate(invalid="ignore", over="ignore"):
            acc[x0:x1, y0:y1] = acc[x0:x1, y0:y1] + ws * ps
            wsum[x0:x1, y0:y1] = wsum[x0:x1, y0:y1] + ws
    return acc, wsum


def cut_ref(plane, x0, y0, cut):
    """lightcone.get_tile's wrap-around cut for any int32 origin: the cut x cut block of ``plane`` at (x0, y0), rows
    modulo plane.shape[0] and columns modulo plane.shape[1], with int64 index arithmetic.  (The indices are reduced
    before np.take sees them: its "wrap" walks an index into range one period at a time.)"""
    ix = (np.int64(x0) + np.arange(cut, dtype=np.int64)) % plane.shape[0]
    iy = (np.int64(y0) + np.arange(cut, dtype=np.int64)) % plane.shape[1]
    return plane.take(ix, axis=0, mode="wrap").take(iy, axis=1, mode="wrap")


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
