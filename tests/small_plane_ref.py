"""Plain NumPy restatement of the device small plane (csrc/window.hip, lightcone.paint_small_plane(on_device=True)):
the wrapped window, its minimum in the plane's dtype, ``ymap_ref.zoom`` in float64, ONE rounding to float32, and the
wrapped crop.  tests/test_small_plane_host.py pins it to ``lightcone.get_tile`` and SciPy; the GPU tests compare the
kernels with SciPy where it is installed and with this where it is not."""
import numpy as np

import ymap_ref as R


def wrapped_window(plane, x0, y0, size):
    """``size`` x ``size`` pixels of the periodic ``plane`` from (x0, y0): pixel (i, j) is plane[(x0 + i) mod rows,
    (y0 + j) mod cols], the modulo not negative."""
    rows, cols = plane.shape
    r = (x0 + np.arange(size)) % rows
    c = (y0 + np.arange(size)) % cols
    return plane[r[:, None], c[None, :]]


def zoom64(window, tile, subtract_minimum=False, chunked=False):
    """The float64 tile BEFORE its rounding: the minimum is subtracted in the window's own dtype (the reference's
    ``tile -= tile.min()`` is a float32 subtraction for a float32 plane), the rest is float64."""
    w = np.asarray(window)
    if subtract_minimum:
        w = w - w.min()
    return R.zoom(w.astype(np.float64), tile, chunked=chunked)


def tile32(window, tile, subtract_minimum=False, chunked=False):
    """The raw tile the network sees: ``zoom64`` rounded once to float32."""
    return zoom64(window, tile, subtract_minimum, chunked).astype(np.float32)


def crop(img, r0, c0, m):
    """(m, m) float64 pixels of the periodic float32 image from (r0, c0)."""
    return wrapped_window(np.asarray(img), r0, c0, m).astype(np.float64)


def geometry(n_mass, shift, delta_size, tile_size, mass_size, n_pixel_tile):
    """The integers of the reference's small-plane branch (process_SLICS.py:68-83 and 162-175), written out:
    (x0, y0, cut) of the window in the mass plane and (r0, c0, m) of the footprint in the painted tile."""
    rel = delta_size / mass_size                                 # get_tile(massplane, shift, rel, expansion)
    expansion = tile_size / delta_size
    cut = int(n_mass * rel * expansion)
    off = int(n_mass * rel * (expansion - 1) / 2)
    x0, y0 = int(n_mass * shift[0]) - off, int(n_mass * shift[1]) - off
    centre = (1 - delta_size / tile_size) / 2                    # get_tile(painted, (centre, centre), delta / tile)
    m = int(n_pixel_tile * (delta_size / tile_size) * 1)
    off2 = int(n_pixel_tile * (delta_size / tile_size) * (1 - 1) / 2)
    r0 = int(n_pixel_tile * centre) - off2
    return (x0, y0, cut), (r0, r0, m)


def ulp32(x):
    """The spacing of float32 in the binade of |x| (float64 in, float64 out): half of it is the most that one rounding
    of x to float32 moves it."""
    m, e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))     # |x| = m 2^e, m in [0.5, 1) (0, 0 for x = 0)
    return np.ldexp(1.0, np.where(m == 0, -149, np.maximum(e - 24, -149)))
