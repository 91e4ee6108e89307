"""Tiling / blending of large mass planes around ``painter.paint`` -- the production caller of
the hot path (/root/reference/baryon_painter/process_SLICS.py:68-126, 198-220).

Only the integer tiling, the wrap-around tile cut, the feathering weights and the blend are here;
the cosmology of ``create_y_map`` (pyccl / astropy) and the SLICS file handling are out of scope.
Unlike the reference's serial per-tile loop, ``paint_plane`` sends all tiles of a plane through
``CVAEPainter.paint_batch`` (hipGraph-captured batches).
"""
import numpy as np


def generate_tiling(n_pixel_plane, n_pixel_tile, min_tile_overlap=0.5):
    """Origins (as fractions of the plane) and slices of a regular grid of square tiles that covers
    the plane with at least ``min_tile_overlap`` relative overlap between neighbours
    (process_SLICS.py:102-126; known answers in the reference's tests/test_SLICS_tiling.py:72-81)."""
    rel = n_pixel_tile / n_pixel_plane
    n_inner = 0
    if rel < 1 - rel + rel * min_tile_overlap:                 # two tiles do not overlap enough
        step = rel * (1 - min_tile_overlap)
        gap = 1 - 2 * rel + rel * min_tile_overlap
        n_inner = 1 if gap <= step else int(np.ceil((gap - step) / step)) + 1
    origins = np.linspace(0, 1 - rel, n_inner + 2, endpoint=True)
    px = [int(o * n_pixel_plane) for o in origins]
    slices = [[np.s_[x:x + n_pixel_tile, y:y + n_pixel_tile] for y in px] for x in px]
    return origins, slices


def get_tile(m, shift, tile_relative_size, expansion_factor=1):
    """Square cut-out of a periodic plane starting at ``shift`` (fractions), wrapping around the
    edges (process_SLICS.py:68-83)."""
    if expansion_factor < 1:
        raise ValueError("Expension factors < 1 not supported.")
    n = m.shape[0]
    size = int(n * tile_relative_size * expansion_factor)
    off = int(n * tile_relative_size * (expansion_factor - 1) / 2)
    x0, y0 = int(n * shift[0]) - off, int(n * shift[1]) - off
    return m.take(range(x0, x0 + size), axis=0, mode="wrap").take(range(y0, y0 + size), axis=1, mode="wrap")


def make_weight_map(tile_shape, falloff=0.05, sigma=1):
    """Feathering weights: 1 inside, Gaussian roll-off over ``falloff`` of the tile size at every
    edge (process_SLICS.py:85-99)."""
    w = np.ones(tile_shape)
    n_edge = int(tile_shape[0] * falloff)
    s = n_edge * sigma
    for i in range(n_edge):
        f = np.exp(-0.5 * (n_edge - i) ** 2 / s ** 2)
        w[i] *= f
        w[-i - 1] *= f
        w[:, i] *= f
        w[:, -i - 1] *= f
    return w


def plane_geometry(n_delta, tile_relative_size, n_pixel_tile, min_tile_overlap=0.5):
    """The integers of ``paint_plane`` for a plane whose ``delta`` has ``n_delta`` rows, with the exact expressions of
    ``generate_tiling`` and ``get_tile``: ``n_plane``, the cut size ``cut`` (``get_tile``'s ``size``), ``n_side`` tiles per
    side and, per tile in tile-id order (tile (j, k) is ``j * n_side + k``), the cut origin in ``delta`` (``origins``) and
    the destination origin in the painted plane (``dst``), as (n_tiles, 2) int32 arrays."""
    n_plane = int(n_pixel_tile / tile_relative_size)
    origins, slices = generate_tiling(n_plane, n_pixel_tile, min_tile_overlap)
    cut = int(n_delta * tile_relative_size * 1)              # get_tile(expansion_factor=1): off = 0
    org = [(int(n_delta * xs), int(n_delta * ys)) for xs in origins for ys in origins]
    dst = [(s[0].start, s[1].start) for row in slices for s in row]
    return {"n_plane": n_plane, "cut": cut, "n_side": len(origins), "origins": np.asarray(org, np.int32).reshape(-1, 2),
            "dst": np.asarray(dst, np.int32).reshape(-1, 2)}


def paint_plane(painter, delta, tile_relative_size, n_pixel_tile, z, min_tile_overlap=0.5, falloff=0.05,
                sigma=0.5, regularise_std=None, batch_size=64, seed=None, first_tile_id=0, on_device=False, out=None):
    """Paint a periodic mass plane tile by tile and blend (the inner loop of ``process_SLICS``,
    process_SLICS.py:198-220): tiles are cut with wrap-around, resampled to the network's tile size
    if necessary, painted in batches, weighted by ``make_weight_map`` and accumulated.

    Painters with a ``paint_stream`` (CVAEPainter) paint all tiles of the plane through the pipelined device path;
    tile (j, k) of the plane draws its prior noise from Philox under the key ``seed`` and the counter
    ``first_tile_id + j * n_side + k``.  ``seed=None`` (default) draws a FRESH key from torch's global generator for
    every call: like the reference (fresh ``torch.randn`` per tile, cvae.py:64) two planes never share their latent
    noise unless asked to, and ``torch.manual_seed`` makes a whole light cone reproducible.  Pass an explicit ``seed``
    (+ distinct ``first_tile_id`` ranges) to reproduce one plane.  Painters / transforms the device pipeline has no
    form for (modes other than 'shift-log', no transform, several label fields, L != 1, no prior network) go through
    ``paint_batch`` as before.

    ``on_device=True`` (opt-in; needs ``painter.can_paint_stream(z)``, NotImplementedError otherwise, raised before any
    random number is drawn or any graph is captured): the plane is uploaded once -- or used in place if ``delta`` is a
    CUDA tensor -- and its tiles are cut, resampled (csrc/plane.hip), painted and blended on the device, with the same
    seeds, tile ids and batches as the host path; only the finished plane is downloaded.  ``out``: a CUDA float64
    (n_plane, n_plane) tensor that receives the plane instead (nothing is downloaded; ``out`` is returned).  The cut
    without resampling and the blend give the host path's bits; the resampling is within 1 ulp (float32) of SciPy's;
    with ``regularise_std`` the tile statistics are float64 sums where NumPy sums float32, so a pixel within about 1e-6
    of the threshold may be kept by one path and dropped by the other."""
    if on_device:
        return _paint_plane_device(painter, delta, tile_relative_size, n_pixel_tile, z, min_tile_overlap, falloff,
                                   sigma, regularise_std, batch_size, seed, first_tile_id, out)
    if out is not None:
        raise ValueError("out= needs on_device=True")
    n_plane = int(n_pixel_tile / tile_relative_size)
    origins, slices = generate_tiling(n_plane, n_pixel_tile, min_tile_overlap)
    tiles = []
    for xs in origins:
        for ys in origins:
            t = get_tile(delta, (xs, ys), tile_relative_size)
            if t.shape[0] != n_pixel_tile:
                import scipy.ndimage
                t = scipy.ndimage.zoom(t, zoom=n_pixel_tile / t.shape[0], mode="reflect")
            tiles.append(np.asarray(t, dtype=np.float32))
    painted = None
    # eligibility is decided UP FRONT (no capture attempted, no random number consumed): an error raised later, deep
    # inside the device pipeline, then propagates instead of silently selecting the slow host path
    if hasattr(painter, "paint_stream") and getattr(painter, "can_paint_stream", lambda z=0.0: True)(z):
        if seed is None:
            import torch
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        ids = first_tile_id + np.arange(len(tiles), dtype=np.int64)
        painted = painter.paint_stream(np.stack(tiles), z, batch_size=min(batch_size, len(tiles)), tile_ids=ids,
                                       seed=seed)
    if painted is None:
        painted = painter.paint_batch(np.stack(tiles), z, batch_size=batch_size)
    plane = np.zeros((n_plane, n_plane))
    weight = np.zeros((n_plane, n_plane))
    it = iter(painted)
    for j in range(len(origins)):
        for k in range(len(origins)):
            p = next(it)
            w = make_weight_map(p.shape, falloff=falloff, sigma=sigma)
            if regularise_std is not None:
                w[np.abs(p - p.mean()) > p.std() * regularise_std] = 0
            plane[slices[j][k]] += w * p
            weight[slices[j][k]] += w
    with np.errstate(invalid="ignore"):          # 0 / 0 where no tile reaches, as in the reference
        return plane / weight


def _paint_plane_device(painter, delta, tile_relative_size, n_pixel_tile, z, min_tile_overlap, falloff, sigma,
                        regularise_std, batch_size, seed, first_tile_id, out):
    if not (hasattr(painter, "_paint_plane_device") and painter.can_paint_stream(z)):
        raise NotImplementedError("paint_plane(on_device=True) needs a painter with a device paint pipeline "
                                  "(CVAEPainter.can_paint_stream)")
    geo = plane_geometry(delta.shape[0], tile_relative_size, n_pixel_tile, min_tile_overlap)
    n_plane, cut = geo["n_plane"], geo["cut"]
    if cut != n_pixel_tile and int(round(cut * (n_pixel_tile / cut))) != n_pixel_tile:
        raise ValueError(f"a {cut}-pixel cut does not zoom to {n_pixel_tile} pixels")
    if (geo["dst"] + n_pixel_tile > n_plane).any():
        raise ValueError("the tiling does not fit the plane")
    n_tiles = len(geo["origins"])
    if seed is None:
        import torch
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    ids = first_tile_id + np.arange(n_tiles, dtype=np.int64)
    w = make_weight_map((n_pixel_tile, n_pixel_tile), falloff=falloff, sigma=sigma)
    return painter._paint_plane_device(delta, geo, z, w, batch_size=min(batch_size, n_tiles), tile_ids=ids, seed=seed,
                                       regularise_std=regularise_std, out=out)
