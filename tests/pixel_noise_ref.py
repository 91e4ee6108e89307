"""Reference of ``bp_likelihood_draw`` (csrc/paint.hip) for the pixel-noise tests: the noise lattice from the oracle's
Philox, and the float32 restatement of the draw.  No test; needs no GPU."""
import numpy as np

from oracle.philox import philox4x32_10


def lattice_normals(seed, ids, origins, h, w, c):
    """e of shape (n, h, w, c) float32: element (s, y, x, ch) is the (ch % 4)-th Box-Muller normal (in float64, as
    ``oracle.philox.tile_normals`` computes it) of the Philox4x32-10 block with key ``seed`` and counter
    (X + ((ch // 4) << 24), 0x80000000 | Y, id low, id high), Y = origins[s][0] + y, X = origins[s][1] + x,
    id = ids[s].  ``origins`` None: all zero."""
    ids = np.asarray(ids, dtype=np.int64).astype(np.uint64)
    n, groups = len(ids), (c + 3) // 4
    org = np.zeros((n, 2), np.int64) if origins is None else np.asarray(origins, dtype=np.int64).reshape(n, 2)
    Y = (org[:, 0, None] + np.arange(h)[None, :])[:, :, None, None]                 # (n, h, 1, 1)
    X = (org[:, 1, None] + np.arange(w)[None, :])[:, None, :, None]                 # (n, 1, w, 1)
    assert Y.min() >= 0 and Y.max() < 2 ** 31 and X.min() >= 0 and X.max() < 2 ** 24
    g = np.arange(groups, dtype=np.int64)[None, None, None, :]
    ctr = np.zeros((n, h, w, groups, 4), dtype=np.uint32)
    ctr[..., 0] = (X + (g << 24)).astype(np.uint32)
    ctr[..., 1] = np.broadcast_to((Y | 0x80000000).astype(np.uint32), (n, h, w, groups))
    ctr[..., 2] = (ids & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None, None, None]
    ctr[..., 3] = (ids >> np.uint64(32)).astype(np.uint32)[:, None, None, None]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.float64)
    out = np.empty((n, h, w, groups, 4))
    for half in range(2):
        u1, u2 = (x[..., 2 * half] + 1.0) / 4294967296.0, x[..., 2 * half + 1] / 4294967296.0
        rad = np.sqrt(-2.0 * np.log(u1))
        out[..., 2 * half] = rad * np.cos(2 * np.pi * u2)
        out[..., 2 * half + 1] = rad * np.sin(2 * np.pi * u2)
    return out.reshape(n, h, w, groups * 4)[..., :c].astype(np.float32)


def draw_ref(t, lv, e):
    """(out, p) in float32: p = float32(exp(float32(0.5) * lv) * e), out = float32(t + p); every step rounds once."""
    t, lv, e = (np.asarray(a, np.float32) for a in (t, lv, e))
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.exp(np.float32(0.5) * lv, dtype=np.float32) * e
        return (t + p).astype(np.float32), p.astype(np.float32)


def draw_bound(ref, p):
    """Per-element bound on |got - ref|: 2^-21 |p| + 2^-23 |ref|.  expf may differ from NumPy's by one ulp (2^-23
    relative, 2^-22 at worst after the product's own rounding moves with it), the sum rounds once (2^-24 |ref|, and a
    last-bit flip of it 2^-23 |ref|); the factor two on the first term is margin."""
    return 2.0 ** -21 * np.abs(p.astype(np.float64)) + 2.0 ** -23 * np.abs(ref.astype(np.float64))
