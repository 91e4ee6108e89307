"""Tiling / blending of large mass planes around ``painter.paint`` -- the production caller of
the hot path (/root/reference/baryon_painter/process_SLICS.py:68-126, 198-220).

Only the integer tiling, the wrap-around tile cut, the feathering weights and the blend are here;
the cosmology of ``create_y_map`` (pyccl / astropy) and the SLICS file handling are out of scope.
Unlike the reference's serial per-tile loop, ``paint_plane`` sends all tiles of a plane through the
painter's ``paint_stream`` (hipGraph-captured batches; ``CVAEPainter`` or ``CGANPainter``) or ``paint_batch``.
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


def _need_pixel_noise(painter):
    """ValueError unless ``painter`` can paint draws from its likelihood (``Painter._need_pixel_noise``).  Draws no
    random number, captures nothing."""
    if not hasattr(painter, "_need_pixel_noise"):
        raise ValueError(f"pixel_noise=True: {type(painter).__name__} cannot draw from a likelihood")
    painter._need_pixel_noise()


class ProblematicTile:
    """One entry of ``TileReport.tiles``: a painted tile with a pixel more than ``regularise_std`` tile standard
    deviations from its tile mean, in any field.  ``tile`` is its number in its plane's tiling, ``position`` = (j, k)
    with ``tile = j * n_side + k``, ``tile_id`` the Philox counter it was painted under, ``plane`` the number of its
    plane in a light cone (None from ``paint_plane``), ``z`` its redshift, ``input`` the raw (tile, tile) float32 tile
    that was painted (resampled, where the plane is), ``painted`` the (tile, tile) -- (F, tile, tile) for a painter with
    F > 1 label fields -- float32 painting, ``n_outliers`` the (F,) int32 counts of offending pixels per field.
    ``as_tuple()`` is the tuple the reference appends (process_SLICS.py:214): (z, input, painted)."""
    __slots__ = ("tile", "position", "tile_id", "plane", "z", "input", "painted", "n_outliers")

    def __init__(self, tile, position, tile_id, plane, z, input, painted, n_outliers):
        self.tile, self.position, self.tile_id, self.plane, self.z = tile, position, tile_id, plane, z
        self.input, self.painted, self.n_outliers = input, painted, n_outliers

    def as_tuple(self):
        return self.z, self.input, self.painted


class TileReport:
    """What ``paint_plane`` / ``paint_light_cone`` (``return_problematic_tiles=True``) say about the painted tiles.
    Per tile and field, (n_tiles, F) arrays: ``mean`` and ``std`` (float64; the population std) and ``n_outliers``
    (int32), the number of pixels with ``abs(p - mean) > std * regularise_std`` -- the pixels ``regularise=True`` masks.
    A tile is problematic if any of its fields has one.  ``n_problematic`` counts all problematic tiles; ``tiles`` holds
    the first ``max_problematic_tiles`` of them as ``ProblematicTile``s, in ascending tile order.  From a light cone
    the three arrays are lists with one array per tiled plane, ``planes`` the numbers of those planes in the cone."""

    def __init__(self, regularise_std, mean, std, n_outliers, n_problematic, tiles, planes=None):
        self.regularise_std, self.mean, self.std, self.n_outliers = regularise_std, mean, std, n_outliers
        self.n_problematic, self.tiles, self.planes = n_problematic, tiles, planes


def _check_report(regularise_std, return_problematic_tiles, max_problematic_tiles):
    """The refusals of a report, before any random number is drawn: ValueError without a ``regularise_std``, for one
    that is negative or not finite, and for a negative cap."""
    if not return_problematic_tiles:
        return
    if regularise_std is None:
        raise ValueError("return_problematic_tiles=True needs a regularise_std: it defines what a problematic tile is")
    if not (np.isfinite(regularise_std) and regularise_std >= 0):
        raise ValueError(f"return_problematic_tiles=True needs a finite regularise_std >= 0, got {regularise_std}")
    if int(max_problematic_tiles) < 0:
        raise ValueError("max_problematic_tiles must not be negative")


def _entries(numbers, inputs, painted, n_outliers, n_side, first_tile_id, z, plane=None):
    """``ProblematicTile``s of one plane: tile numbers, their raw and painted tiles, the plane's (n_tiles, F) counts."""
    out = []
    for t, raw, p in zip(numbers, inputs, painted):
        t = int(t)
        out.append(ProblematicTile(t, divmod(t, n_side), int(first_tile_id) + t, plane, z, raw, p, n_outliers[t].copy()))
    return out


def _report_host(tiles, painted, regularise_std, cap, n_side, first_tile_id, z):
    """The report of the host path: NumPy's own statistics of the painted tiles (float32 sums, as ``_blend_host``'s
    mask), (N, H, W) or (N, F, H, W)."""
    p4 = painted[:, None] if np.ndim(painted) == 3 else painted
    n, F = p4.shape[:2]
    mean, std = np.empty((n, F)), np.empty((n, F))
    count = np.empty((n, F), dtype=np.int32)
    for t in range(n):
        for f in range(F):
            p = p4[t, f]
            mean[t, f], std[t, f] = p.mean(), p.std()
            count[t, f] = np.count_nonzero(np.abs(p - p.mean()) > p.std() * regularise_std)
    bad = np.flatnonzero((count != 0).any(axis=1))
    keep = bad[:cap]
    entries = _entries(keep, [np.asarray(tiles[t]) for t in keep], [np.asarray(painted[t]) for t in keep], count, n_side,
                       first_tile_id, z)
    return TileReport(regularise_std, mean, std, count, len(bad), entries)


def paint_plane(painter, delta, tile_relative_size, n_pixel_tile, z, min_tile_overlap=0.5, falloff=0.05,
                sigma=0.5, regularise_std=None, batch_size=64, seed=None, first_tile_id=0, on_device=False, out=None,
                pixel_noise=False, regularise=True, return_problematic_tiles=False, max_problematic_tiles=16):
    """Paint a periodic mass plane tile by tile and blend (the inner loop of ``process_SLICS``,
    process_SLICS.py:198-220): tiles are cut with wrap-around, resampled to the network's tile size
    if necessary, painted in batches, weighted by ``make_weight_map`` and accumulated.

    Painters with a ``paint_stream`` (CVAEPainter, CGANPainter) paint all tiles of the plane through the pipelined
    device path.  The CGAN has no latent noise: ``seed`` and ``first_tile_id`` are passed on and do not affect its planes.
    With a CVAEPainter, tile (j, k) of the plane draws its prior noise from Philox under the key ``seed`` and the counter
    ``first_tile_id + j * n_side + k``.  ``seed=None`` (default) draws a FRESH key from torch's global generator for
    every call: like the reference (fresh ``torch.randn`` per tile, cvae.py:64) two planes never share their latent
    noise unless asked to, and ``torch.manual_seed`` makes a whole light cone reproducible.  Pass an explicit ``seed``
    (+ distinct ``first_tile_id`` ranges) to reproduce one plane.  Painters / transforms the device pipeline has no
    form for (no transform, L != 1) go through ``paint_batch`` as before.

    A painter with F > 1 label fields paints (N, F, H, W) tiles on either path and the result is (F, n_plane, n_plane):
    field j's plane is blended from field j's tiles alone, with its own ``regularise_std`` mask; ``out`` has that
    shape too.

    ``on_device=True`` (opt-in; needs ``painter.can_paint_stream(z)``, NotImplementedError otherwise, raised before any
    random number is drawn or any graph is captured): the plane is uploaded once -- or used in place if ``delta`` is a
    CUDA tensor -- and its tiles are cut, resampled (csrc/plane.hip), painted and blended on the device, with the same
    seeds, tile ids and batches as the host path; only the finished plane is downloaded.  ``out``: a CUDA float64
    (n_plane, n_plane) tensor that receives the plane instead (nothing is downloaded; ``out`` is returned).  The cut
    without resampling and the blend give the host path's bits; the resampling is the exact cubic spline under
    half-sample symmetric boundaries, which for cuts of 12 pixels and more is SciPy's within 1 ulp (float32).  Below 12
    SciPy's own "reflect" prefilter departs from the exact solve and the two paths differ by that much, relative to the
    tile's largest value (measured on the CPU with SciPy 1.15.3, tests/test_plane_kernels_host.py): 6e-4, 1e-4, 7e-6,
    3e-7, 5e-8, 2e-9, 3e-10, 1e-11, 5e-13 at cuts of 2 ... 10 pixels, 7e-15 at 12 (real planes cut hundreds).  With
    ``regularise_std`` the tile statistics are float64 sums where NumPy sums float32, so a pixel within about 1e-6
    of the threshold may be kept by one path and dropped by the other.

    ``pixel_noise=True`` (a CVAEPainter whose model has a variance head; ValueError otherwise, before any random number
    is drawn or any graph is captured), on either path: every tile is a draw from the likelihood, x_mu + sqrt(x_var) e
    in network units, instead of its mean.  The plane has ONE noise lattice, ``first_tile_id`` under the key ``seed``,
    and every tile reads its window of it at its destination origin in the painted plane (``plane_geometry``'s ``dst``),
    so that overlapping tiles carry the same e at the same plane pixel: independent draws would be averaged by the
    feathered blend, which would lower the scatter wherever tiles overlap (about half the plane at
    ``min_tile_overlap=0.5``).  The blend runs in physical units, behind the non-linear inverse transform: a blended
    pixel is a weighted mean of two monotone functions of one normal (each tile's own mean and variance at that
    pixel), not exactly one draw.

    ``regularise`` (with a ``regularise_std``): True, the default here, zeroes the blend weights of the pixels beyond
    ``regularise_std`` tile standard deviations, as this function always has.  The reference's default is False
    (process_SLICS.py:179): there ``regularise_std`` alone only DETECTS.  ``regularise=False`` is that detect-only mode:
    the plane is blended unmasked and is the plane without ``regularise_std``, bit for bit.

    ``return_problematic_tiles=True`` (needs a finite ``regularise_std`` >= 0 and ``max_problematic_tiles`` >= 0;
    ValueError otherwise, before any random number is drawn or any graph is captured), on either path and for either
    value of ``regularise``: returns (plane, report), a ``TileReport`` with every tile's mean, std and number of
    offending pixels per field and the first ``max_problematic_tiles`` problematic tiles with their inputs and
    paintings (the reference's ``return_problematic_tiles``, process_SLICS.py:212-216).  On the device the counts
    are taken and the tiles set aside between the paint graph and the blend (``bp_tile_outliers``, ``bp_tile_keep``)
    and downloaded once behind the finished plane; the statistics are the blend's own float64 ones, the host path's
    NumPy's float32 sums, so the two reports agree outside the tie band above.  Without the flag nothing is added to the
    plane's launches."""
    _check_report(regularise_std, return_problematic_tiles, max_problematic_tiles)
    if pixel_noise:
        _need_pixel_noise(painter)
    if on_device:
        return _paint_plane_device(painter, delta, tile_relative_size, n_pixel_tile, z, min_tile_overlap, falloff,
                                   sigma, regularise_std, batch_size, seed, first_tile_id, out, pixel_noise, regularise,
                                   int(max_problematic_tiles) if return_problematic_tiles else None)
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
    noise = {}
    if pixel_noise:                              # one lattice, every tile's window at its place in the painted plane
        noise = dict(pixel_noise=True, noise_ids=np.full(len(tiles), first_tile_id, dtype=np.int64),
                     noise_origins=np.asarray([(s[0].start, s[1].start) for row in slices for s in row], dtype=np.int32))
    # eligibility is decided UP FRONT (no capture attempted, no random number consumed): an error raised later, deep
    # inside the device pipeline, then propagates instead of silently selecting the slow host path
    if hasattr(painter, "paint_stream") and getattr(painter, "can_paint_stream", lambda z=0.0: True)(z):
        if seed is None:
            import torch
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        ids = first_tile_id + np.arange(len(tiles), dtype=np.int64)
        painted = painter.paint_stream(np.stack(tiles), z, batch_size=min(batch_size, len(tiles)), tile_ids=ids,
                                       seed=seed, **noise)
    if painted is None:
        if pixel_noise:
            noise["seed"] = seed                 # (None: paint_batch draws a fresh key)
        painted = painter.paint_batch(np.stack(tiles), z, batch_size=batch_size, **noise)
    mask_std = regularise_std if regularise else None
    if np.ndim(painted) == 4:                    # (N, F, H, W): one plane per label field, each with its own mask
        plane = np.stack([_blend_host(painted[:, f], slices, n_plane, falloff, sigma, mask_std)
                          for f in range(painted.shape[1])])
    else:
        plane = _blend_host(painted, slices, n_plane, falloff, sigma, mask_std)
    if return_problematic_tiles:
        return plane, _report_host(tiles, painted, regularise_std, int(max_problematic_tiles), len(origins),
                                   first_tile_id, z)
    return plane


def _blend_host(painted, slices, n_plane, falloff, sigma, regularise_std):
    """The blend of ``paint_plane`` (process_SLICS.py:205-220): the painted tiles of ONE field, in tile order, weighted by
    ``make_weight_map`` (zeroed beyond ``regularise_std`` tile standard deviations), accumulated and divided."""
    plane = np.zeros((n_plane, n_plane))
    weight = np.zeros((n_plane, n_plane))
    it = iter(painted)
    for j in range(len(slices)):
        for k in range(len(slices)):
            p = next(it)
            w = make_weight_map(p.shape, falloff=falloff, sigma=sigma)
            if regularise_std is not None:
                w[np.abs(p - p.mean()) > p.std() * regularise_std] = 0
            plane[slices[j][k]] += w * p
            weight[slices[j][k]] += w
    with np.errstate(invalid="ignore"):          # 0 / 0 where no tile reaches, as in the reference
        return plane / weight


def _paint_plane_device(painter, delta, tile_relative_size, n_pixel_tile, z, min_tile_overlap, falloff, sigma,
                        regularise_std, batch_size, seed, first_tile_id, out, pixel_noise=False, regularise=True,
                        report_cap=None, keep=None, plane_number=None):
    """``paint_plane(on_device=True)``.  ``report_cap``: the plane's own report is built and (plane, report) returned.
    ``keep`` (``paint_light_cone``): the cone's ``painter.TileKeep``, in which this plane, number ``plane_number`` of
    the cone, leaves its counts and its problematic tiles on the device; nothing is downloaded here."""
    if not (hasattr(painter, "_paint_plane_device") and painter.can_paint_stream(z)):
        raise NotImplementedError("paint_plane(on_device=True) needs a painter with a device paint pipeline "
                                  "(CVAEPainter / CGANPainter .can_paint_stream)")
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
    kw = {"pixel_noise": True} if pixel_noise else {}
    if not regularise:
        kw["regularise"] = False
    own = keep is None and report_cap is not None
    if own:
        from .painter import TileKeep
        keep = TileKeep(painter, n_pixel_tile, report_cap, regularise_std)
    if keep is not None:
        # a lone plane's slots are numbered from 0, a cone's by its running tile id (first_tile_id there)
        kw["keep"] = keep.plane(0 if own else first_tile_id, n_tiles, geo["n_side"], first_tile_id, z, plane_number)
    plane = painter._paint_plane_device(delta, geo, z, w, batch_size=min(batch_size, n_tiles), tile_ids=ids, seed=seed,
                                        regularise_std=regularise_std, out=out, **kw)
    return (plane, _report_device(keep)[0]) if own else plane


def _report_device(keep):
    """Download what a ``painter.TileKeep`` holds, once, and build one ``TileReport`` per plane it has seen (in the order
    painted; each with the entries of that plane that fit the shared cap and ``n_problematic`` of that plane alone)."""
    reports = []
    for rec, mean, std, count, numbers, raws, painted in keep.download():
        entries = _entries(numbers, raws, painted, count, rec["n_side"], rec["first_tile_id"], rec["z"], rec["plane"])
        reports.append(TileReport(keep.regularise_std, mean, std, count,
                                  int(np.count_nonzero((count != 0).any(axis=1))), entries))
    return reports


def _cone_report(regularise_std, reports, numbers):
    """One report for a light cone from its tiled planes' reports, in plane order."""
    return TileReport(regularise_std, [r.mean for r in reports], [r.std for r in reports],
                      [r.n_outliers for r in reports], sum(r.n_problematic for r in reports),
                      [e for r in reports for e in r.tiles], planes=list(numbers))


# ---------------------------------------------------------------------------------------------------------------------
# Ensembles of planes: K latent draws of every tile, each draw blended into a plane of its own, the moments across the
# K planes.  (The moments of a feathered blend are not the blend of the tiles' moments: the blend runs in physical
# units behind a non-linear inverse.)

def ensemble_moments(planes):
    """(mean, var) across axis 0 of ``planes`` (K, ...) in float64, with the arithmetic of ``bp_plane_moments``
    (include/bp_hip.h), every operation rounded once, in ascending k: S = ((P_0 + P_1) + ...) + P_{K-1}, M = S / K,
    Q = ((P_0 - M)^2 + (P_1 - M)^2) + ..., mean = M, var = Q / K -- the population variance (``np.var``, ddof = 0) in two
    passes.  NaN (a pixel no tile reaches) and infinite elements give what IEEE arithmetic gives; K = 1 gives var = +0
    where the plane is finite."""
    p = np.asarray(planes, dtype=np.float64)
    if p.ndim < 1 or p.shape[0] < 1:
        raise ValueError("ensemble_moments needs at least one plane")
    K = np.float64(p.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        S = p[0].copy()
        for k in range(1, p.shape[0]):
            S = S + p[k]
        M = S / K
        Q = None
        for k in range(p.shape[0]):
            d = p[k] - M
            Q = d * d if Q is None else Q + d * d
        return M, Q / K


def _need_ensemble(painter, zs, draws, batch_size, pixel_noise, on_device, what, method="_paint_plane_device"):
    """The refusals the ensemble surfaces share, before any random number is drawn or any graph is captured: ``draws``
    = K outside 1 ... 64 or not dividing ``batch_size`` (ValueError), ``pixel_noise`` (NotImplementedError), a painter
    without ``paint_ensemble`` -- the CGAN has no latent -- or without an ensemble pipeline at one of the redshifts
    ``zs``, or, with ``on_device``, without the device ``method`` (NotImplementedError).  Returns K."""
    from .models import paint_graph as PG
    K = PG.check_draws(draws)
    if batch_size is not None and (int(batch_size) < K or int(batch_size) % K):
        raise ValueError(f"batch_size counts generator samples: {K} draws per tile must divide it, got {batch_size}")
    if pixel_noise:
        raise NotImplementedError(f"{what} has no pixel_noise: an ensemble block has no noise_org, so the overlapping "
                                  "tiles of a plane could not share their noise lattice")
    if not (hasattr(painter, "paint_ensemble") and hasattr(painter, "_device_paint_parameters")):
        raise NotImplementedError(f"{what} needs a painter with paint_ensemble (a CVAEPainter: a CGAN has no latent to "
                                  "draw from)")
    if on_device and not hasattr(painter, method):
        raise NotImplementedError(f"{what}(on_device=True) needs a painter with a device paint pipeline")
    for z in zs:                                  # (NotImplementedError where the painter has no ensemble pipeline)
        painter._device_paint_parameters(np.full(1, float(z)), ensemble=True)
    return K


def _fresh_seed(seed):
    if seed is None:
        import torch
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    return seed


def paint_plane_ensemble(painter, delta, tile_relative_size, n_pixel_tile, z, draws, min_tile_overlap=0.5, falloff=0.05,
                         sigma=0.5, regularise_std=None, batch_size=64, seed=None, first_tile_id=0, on_device=False,
                         out=None, return_planes=False):
    """The conditional mean and scatter of a painted PLANE at fixed dark matter: ``draws`` = K (1 ... 64) latent draws
    of every tile of ``paint_plane``'s tiling, draw k of all tiles blended into plane k exactly as ``paint_plane``
    blends (``falloff``, ``sigma``, ``regularise_std`` per draw and field), and the moments ACROSS the K planes:
    returns (mean, var), float64 (n_plane, n_plane) -- (F, n_plane, n_plane) for a painter with F > 1 label fields --
    with ``var`` the population variance (``ensemble_moments``).  ``return_planes=True`` adds the K planes,
    (K, [F,] n_plane, n_plane).  Pixels no tile reaches are NaN in all three.

    Draw l of tile (j, k) uses the Philox counter (g, l, ``first_tile_id`` + j * n_side + k) under the key ``seed``
    (None: a fresh key from torch's global generator): plane 0 is the plane ``paint_plane`` paints for the same seed and
    ids, and nothing depends on ``batch_size``, which counts generator samples -- K must divide it (ValueError), and a
    batch carries ``batch_size // K`` tiles.  The painter needs ``paint_ensemble`` (a CVAEPainter; NotImplementedError
    for a CGAN, which has no latent, and for transforms or models without an ensemble pipeline), checked before any
    random number is drawn or any graph is captured.  There is no ``pixel_noise`` here and no sharding over ranks.

    Host path: ``paint_plane``'s host cut and zoom, ``painter.paint_ensemble(..., return_draws=True)``, the host blend
    per draw and field, ``ensemble_moments``.

    ``on_device=True``: cut, zoom, the draws, the K blends (``bp_plane_blend_fields`` over K F planes) and the moments
    (``bp_plane_moments``) run on the device on one stream; the conditioning of a tile runs once, not K times, and only
    mean and variance (and the planes, if asked for) are downloaded.  ``out`` = (mean, var): two CUDA float64 tensors
    of the result's shape that receive it; nothing is downloaded, and with ``return_planes`` the planes are a CUDA
    tensor.  ``delta`` may be a CUDA tensor, used in place.  The K accumulator pairs take ``16 K F n_plane^2`` bytes of
    device memory (4.3 GB at 4096^2 and K = 16), kept until ``painter.release_paint_buffers()``.  Parity with the
    host path is ``paint_plane``'s: equal bits of cut and blend, 1 ulp (float32) in the resampled tiles, the tie band of
    ``regularise_std``."""
    K = _need_ensemble(painter, [z], draws, batch_size, False, on_device, "paint_plane_ensemble")
    if out is not None and not on_device:
        raise ValueError("out= needs on_device=True")
    geo = plane_geometry(delta.shape[0], tile_relative_size, n_pixel_tile, min_tile_overlap)
    n_plane, cut, n_tiles = geo["n_plane"], geo["cut"], len(geo["origins"])
    per = min(int(batch_size) // K, n_tiles)                     # tiles per batch
    ids = first_tile_id + np.arange(n_tiles, dtype=np.int64)
    if on_device:
        if cut != n_pixel_tile and int(round(cut * (n_pixel_tile / cut))) != n_pixel_tile:
            raise ValueError(f"a {cut}-pixel cut does not zoom to {n_pixel_tile} pixels")
        if (geo["dst"] + n_pixel_tile > n_plane).any():
            raise ValueError("the tiling does not fit the plane")
        w = make_weight_map((n_pixel_tile, n_pixel_tile), falloff=falloff, sigma=sigma)
        return painter._paint_plane_device(delta, geo, z, w, batch_size=per, tile_ids=ids, seed=_fresh_seed(seed),
                                           regularise_std=regularise_std, out=out, draws=K,
                                           return_planes=return_planes)
    origins, slices = generate_tiling(n_plane, n_pixel_tile, min_tile_overlap)
    tiles = []
    for xs in origins:
        for ys in origins:
            t = get_tile(delta, (xs, ys), tile_relative_size)
            if t.shape[0] != n_pixel_tile:
                import scipy.ndimage
                t = scipy.ndimage.zoom(t, zoom=n_pixel_tile / t.shape[0], mode="reflect")
            tiles.append(np.asarray(t, dtype=np.float32))
    painted = painter.paint_ensemble(np.stack(tiles), z, draws=K, batch_size=per * K, tile_ids=ids,
                                     seed=_fresh_seed(seed), return_draws=True)[2]
    if painted.ndim == 4:                        # (N, K, H, W) -> (N, K, 1, H, W)
        painted = painted[:, :, None]
    planes = np.stack([np.stack([_blend_host(painted[:, k, f], slices, n_plane, falloff, sigma, regularise_std)
                                 for f in range(painted.shape[2])]) for k in range(K)])
    if painted.shape[2] == 1:
        planes = planes[:, 0]
    mean, var = ensemble_moments(planes)
    return (mean, var, planes) if return_planes else (mean, var)


# ---------------------------------------------------------------------------------------------------------------------
# From painted planes to one Compton-y map (process_SLICS.py:12-66), and the light cone end to end.

_SLAB = 252.5                                     # comoving thickness of a SLICS slab in Mpc/h (process_SLICS.py:26, 29)
_projection_buffers = {}                          # per device: the float64 scratch of bp_plane_project_order
_DEVICE_ORDERS = (2, 3, 4, 5)                     # spline orders csrc/ymap.hip has (0 and 1 have no prefilter: host only)


def release_projection_buffers():
    """Free the device scratch ``project_planes(on_device=True)`` keeps between calls (two float64 images of the
    largest plane projected so far, per device)."""
    _projection_buffers.clear()


def _project_host(y_map, d, scale, order):
    """One turn of the reference loop (process_SLICS.py:56-64) with its per-plane factor given as ``scale``."""
    import scipy.ndimage
    zoom_factor = y_map.shape[0] / d.shape[0]
    d = d.copy()
    d[np.isnan(d)] = 0
    d *= scale
    y_map += scipy.ndimage.zoom(d, zoom=zoom_factor, order=order, mode="mirror")


def _project_device(plane, scale, y_map, order=3):
    """y_map += zoom(nan_to_zero(plane) * scale, order) on the device (csrc/ymap.hip), on the current stream of the
    plane's device, without a host synchronisation: ``plane`` a contiguous square CUDA float64 tensor (left as it is),
    ``y_map`` a contiguous CUDA float64 (res, res) tensor, ``order`` in 2 ... 5.  The scratch kept per device is
    measured against what THIS order asks for at every call, so a change of order can only grow it."""
    import ctypes as C
    import torch
    from . import _lib as L
    lib = L.load()
    n, res = plane.shape[0], y_map.shape[0]
    ws = int(lib.bp_plane_project_order_workspace(n, res, order))
    key = str(plane.device)
    scratch = _projection_buffers.get(key)
    if scratch is None or scratch.numel() * 8 < ws:
        _projection_buffers.pop(key, None)
        scratch = _projection_buffers[key] = torch.empty(max(ws // 8, 1), dtype=torch.float64, device=plane.device)
    with torch.cuda.device(plane.device):
        sm = C.c_void_p(torch.cuda.current_stream(plane.device).cuda_stream)
        L.check(lib.bp_plane_project_order(L.ptr(plane), plane.shape[0], plane.shape[1], float(scale), int(order),
                                           L.ptr(scratch), scratch.numel() * 8, L.ptr(y_map), res, sm),
                "plane project")


def _check_map(out, resolution, device=None):
    import torch
    if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float64 or
            tuple(out.shape) != (resolution, resolution) or not out.is_contiguous() or
            (device is not None and out.device != device)):
        raise ValueError(f"out must be a contiguous CUDA float64 ({resolution}, {resolution}) tensor"
                         + (f" on {device}" if device is not None else ""))


def project_planes(planes, scales, resolution, order=3, on_device=False, out=None):
    """Sum painted planes into one (resolution, resolution) map: NaNs (pixels no tile reached) are zeroed, plane i is
    multiplied by ``scales[i]`` and resampled to the map's resolution with ``scipy.ndimage.zoom(order, mode="mirror")``
    (the loop of ``create_y_map``, process_SLICS.py:55-64).  ``scales[i]`` is the whole per-plane factor: the reference's
    division by ``zoom_factor**2`` is part of it (``y_map_scales`` computes it).  The planes are not modified.

    ``on_device=True`` (orders 2 to 5; NotImplementedError otherwise, before anything is launched): planes may be NumPy
    arrays (uploaded as float64) or square CUDA float64 tensors (used in place), and each is projected by
    ``bp_plane_project_order`` (csrc/ymap.hip) in float64, within 1e-12 of the largest pixel of SciPy's result.  The map is
    downloaded once, or, with ``out`` (a CUDA float64 (resolution, resolution) tensor), ACCUMULATED into ``out``, which
    is returned.  The scratch is kept between calls (``release_projection_buffers``)."""
    if not on_device:
        if out is not None:
            raise ValueError("out= needs on_device=True")
        y_map = np.zeros((resolution, resolution))
        for d, s in zip(planes, scales):
            _project_host(y_map, d, s, order)
        return y_map
    if order not in _DEVICE_ORDERS:
        raise NotImplementedError("project_planes(on_device=True) resamples with splines of order 2 to 5 only")
    import torch
    if out is not None:
        _check_map(out, resolution)
    dev = out.device if out is not None else None
    y_map = out
    with torch.no_grad():
        for d, s in zip(planes, scales):
            if isinstance(d, torch.Tensor):
                if not d.is_cuda or d.dtype != torch.float64 or d.dim() != 2 or d.shape[0] != d.shape[1]:
                    raise TypeError("a device plane must be a square CUDA float64 tensor")
                if dev is not None and d.device != dev:
                    raise ValueError(f"a plane lives on {d.device}, the map on {dev}")
                p = d if d.is_contiguous() else d.contiguous()
            else:
                d = np.asarray(d)
                if d.ndim != 2 or d.shape[0] != d.shape[1]:
                    raise TypeError("a plane must be a square 2-d array")
                if dev is None:
                    dev = torch.device("cuda", torch.cuda.current_device())
                p = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float64)).to(dev)
            if y_map is None:
                dev = p.device
                y_map = torch.zeros((resolution, resolution), dtype=torch.float64, device=dev)
            _project_device(p, s, y_map, order)
        if out is not None:
            return out
        if y_map is None:                                        # no planes
            return np.zeros((resolution, resolution))
        return y_map.cpu().numpy()


def pixel_area_mean(chi_lo, chi_hi, theta_pix, scale_factor_of_chi):
    """Mean over the comoving slab [chi_lo, chi_hi] of the squared physical size ``(chi a(chi) theta_pix)**2`` of a map
    pixel of ``theta_pix`` radians (``A_pix_mean`` / ``L_pix`` of process_SLICS.py:13-20, with pyccl's scale factor
    replaced by the callable ``scale_factor_of_chi``)."""
    import scipy.integrate
    f = lambda chi: (chi * scale_factor_of_chi(chi) * theta_pix) ** 2          # noqa: E731
    return scipy.integrate.quad(f, chi_lo, chi_hi)[0] / (chi_hi - chi_lo)


def slab_edges(chi, h):
    """Comoving edges of the slabs whose mid-planes lie at ``chi``: half a slab in front of every plane (not in front
    of the observer), one slab behind the last (process_SLICS.py:25-29)."""
    d_A = np.array(chi, dtype=np.float64)
    d_A -= _SLAB / h / 2
    if d_A[0] < 0:
        d_A[0] = 0
    return np.append(d_A, d_A[-1] + _SLAB / h)


def y_map_scales(n_pixel_planes, resolution, map_size, chi, scale_factor_of_chi, h):
    """The factor that turns painted plane i (``n_pixel_planes[i]`` pixels a side) into its contribution to a Compton-y
    map of ``resolution`` pixels and ``map_size`` degrees a side, in float64 and in the reference's order of
    operations (process_SLICS.py:31-32, 41-50, 56, 60): ``V_c (Xe + Xi) / Xe y_fac / A_pix_eff[i] / zoom_factor**2``."""
    d_A = slab_edges(chi, h)
    theta_pix = map_size / resolution * np.pi / 180            # pixel size in radians
    A_pix_eff = np.array([pixel_area_mean(d_A[i], d_A[i + 1], theta_pix, scale_factor_of_chi)
                          for i in range(len(n_pixel_planes))])
    y_fac = 8.125561e-16                                       # sigma_T / m_e c^2 in SI
    mpc = 3.086e22                                             # m / Mpc
    eV = 1.60218e-19                                           # J
    cm = 0.01                                                  # m
    Xe = 1.17
    Xi = 1.08
    V_c = (400 / h / 2048 * mpc / cm) ** 3                     # volume of a simulation cell in cm^3
    y_fac = y_fac * eV * mpc ** -2                             # sigma_T / m_e c^2 in Mpc^2 / eV
    scales = []
    for i, n in enumerate(n_pixel_planes):
        zoom_factor = resolution / n
        scales.append(V_c * (Xe + Xi) / Xe * y_fac / A_pix_eff[i] / zoom_factor ** 2)
    return np.array(scales, dtype=np.float64)


def create_y_map(painted_planes, z, resolution, map_size, chi, scale_factor_of_chi, h, order=3, on_device=False,
                 out=None):
    """Compton-y map of ``map_size`` degrees and ``resolution`` pixels a side from the painted planes of a light cone
    (``create_y_map`` of process_SLICS.py:12-66).  The cosmology is the caller's: ``chi[i]`` is the comoving angular
    distance of plane i (what ``ccl.comoving_angular_distance`` gave at ``1 / (1 + z[i])``), ``scale_factor_of_chi`` a
    callable a(chi), ``h`` the dimensionless Hubble parameter.  The rest is ``y_map_scales`` and ``project_planes``."""
    painted_planes = list(painted_planes)
    if not len(painted_planes) == len(z) == len(chi):
        raise ValueError("painted_planes, z and chi need one entry per plane")
    scales = y_map_scales([d.shape[0] for d in painted_planes], resolution, map_size, chi, scale_factor_of_chi, h)
    return project_planes(painted_planes, scales, resolution, order=order, on_device=on_device, out=out)


def _streams(painter, z):
    return hasattr(painter, "paint_stream") and getattr(painter, "can_paint_stream", lambda z=0.0: True)(z)


def _field_index(painter, field):
    """Which label field of ``painter`` a light cone projects: None for a painter with one label field (``field`` may
    name it), the index of ``field`` for a painter with several -- ValueError without a name or for a name the painter
    does not paint.  Draws no random number."""
    fields = list(getattr(painter, "label_fields", None) or [])
    if field is not None and fields and field not in fields:
        raise ValueError(f"field {field!r} is not one of the painter's label fields {fields}")
    if len(fields) > 1:
        if field is None:
            raise ValueError(f"a painter with the label fields {fields} needs field=<one of them>")
        return fields.index(field)
    return None


def small_plane_geometry(n_mass, shift, delta_size, tile_size, mass_size, n_pixel_tile):
    """The integers of ``paint_small_plane`` for a mass plane of ``n_mass`` rows, with ``get_tile``'s exact expressions:
    the window cut from the mass plane -- origin (``x0``, ``y0``), not wrapped yet, and ``cut`` pixels a side -- and the
    footprint cropped from the painted tile of ``n_pixel_tile`` pixels -- origin (``r0``, ``c0``) and ``crop`` pixels a
    side.  ValueError for ``tile_size < delta_size``, as ``get_tile``'s."""
    rel, exp = delta_size / mass_size, tile_size / delta_size
    if exp < 1:
        raise ValueError("Expension factors < 1 not supported.")
    cut = int(n_mass * rel * exp)
    off = int(n_mass * rel * (exp - 1) / 2)
    centre = (1 - delta_size / tile_size) / 2
    return {"x0": int(n_mass * shift[0]) - off, "y0": int(n_mass * shift[1]) - off, "cut": cut,
            "r0": int(n_pixel_tile * centre), "c0": int(n_pixel_tile * centre),
            "crop": int(n_pixel_tile * (delta_size / tile_size) * 1)}


def paint_small_plane(painter, massplane, shift, delta_size, tile_size, mass_size, n_pixel_tile, z, seed=None,
                      tile_id=0, subtract_minimum=False, field=None, pixel_noise=False, on_device=False, out=None):
    """Paint a plane whose footprint ``delta_size`` is smaller than the network's tile ``tile_size`` (the low-redshift
    branch of ``process_SLICS``, process_SLICS.py:149-176): ONE tile, expanded to the network's size around the
    footprint, is cut with wrap-around at ``shift`` from the periodic mass plane of ``mass_size`` (all three sizes in
    the same unit), resampled to ``n_pixel_tile`` pixels with ``scipy.ndimage.zoom(mode="mirror")`` and painted, and
    the central footprint of the painted tile is returned.  ``subtract_minimum``: the reference's ``SLICS_density``
    switch (the tile's minimum is subtracted before resampling).

    By default cut and zoom stay on the host.  A painter with a device pipeline for this redshift
    (``can_paint_stream``) paints through ``paint_stream`` with the Philox key (``seed``, ``tile_id``); ``seed=None``
    draws a fresh key from torch's global generator.  Any other painter goes through ``paint``.  The plane is returned
    as float64, like ``paint_plane``'s.  ``field``: the label field to return, needed for a painter with several
    (ValueError without it, before any random number is drawn).  ``pixel_noise``: the tile is a draw from the likelihood
    (``paint_plane``) on the lattice ``tile_id`` at origin (0, 0), on either path (``paint`` under the same ``seed``).

    ``on_device=True`` (opt-in; needs ``painter.can_paint_stream(z)``, NotImplementedError otherwise, raised before any
    random number is drawn or any graph is captured): minimum, cut, zoom, paint and crop run on the device on one stream
    (csrc/window.hip around ``model.paint_graph(1)``), with the integers of ``small_plane_geometry`` and the seed word,
    tile id and noise lattice of the host path.  A NumPy or memory-mapped ``massplane`` (float32 or float64): only the
    wrapped window is gathered on the host and uploaded.  A CUDA ``massplane`` on the painter's device is used in
    place, the wrap in the kernel; both give the same bits.  Returns the (m, m) float64 plane as NumPy, or fills and
    returns ``out`` (a CUDA float64 (m, m) tensor; nothing is downloaded).  The resampled tile is SciPy's float64
    zoom rounded once to float32, within one float32 rounding of the host path's tile and not bit-equal to it
    everywhere, so the painted planes of the two paths differ by what the network makes of that."""
    j = _field_index(painter, field)
    noise = {}
    if pixel_noise:
        _need_pixel_noise(painter)
        noise = {"pixel_noise": True}
    if on_device:
        return _paint_small_plane_device(painter, massplane, shift, delta_size, tile_size, mass_size, n_pixel_tile, z,
                                         seed, tile_id, subtract_minimum, j, out, pixel_noise)
    if out is not None:
        raise ValueError("out= needs on_device=True")
    import scipy.ndimage
    tile = get_tile(massplane, shift, tile_relative_size=delta_size / mass_size,
                    expansion_factor=tile_size / delta_size)
    if subtract_minimum:
        tile = tile - tile.min()
    tile = scipy.ndimage.zoom(tile, zoom=n_pixel_tile / tile.shape[0], mode="mirror")
    if _streams(painter, z):
        if tile.shape != (n_pixel_tile, n_pixel_tile):
            raise ValueError(f"the expanded tile zooms to {tile.shape}, not to {n_pixel_tile} pixels")
        if seed is None:
            import torch
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        painted = painter.paint_stream(np.asarray(tile, dtype=np.float32)[None], z, batch_size=1,
                                       tile_ids=np.array([tile_id], dtype=np.int64), seed=seed, **noise)[0]
    else:
        if pixel_noise:
            noise.update(seed=seed, noise_id=tile_id)
        painted = painter.paint(input=tile, z=z, transform=True, inverse_transform=True, **noise)
    if j is not None:
        painted = painted[j]
    centre = (1 - delta_size / tile_size) / 2
    # (float64 like paint_plane's planes: the projection then scales a float32 tile in double on either path)
    return get_tile(np.asarray(painted, dtype=np.float64), shift=(centre, centre),
                    tile_relative_size=delta_size / tile_size)


def _paint_small_plane_device(painter, massplane, shift, delta_size, tile_size, mass_size, n_pixel_tile, z, seed,
                              tile_id, subtract_minimum, j, out, pixel_noise, draws=None, return_planes=False,
                              moments=True):
    """``draws`` = K: the ensemble form (``paint_small_plane_ensemble``, which has checked the painter already)."""
    if draws is None and not (hasattr(painter, "_paint_small_plane_device") and _streams(painter, z)):
        raise NotImplementedError("paint_small_plane(on_device=True) needs a painter with a device paint pipeline "
                                  "(CVAEPainter / CGANPainter .can_paint_stream)")
    import torch
    geo = small_plane_geometry(massplane.shape[0], shift, delta_size, tile_size, mass_size, n_pixel_tile)
    cut = geo["cut"]
    if cut < 2 or int(round(cut * (n_pixel_tile / cut))) != n_pixel_tile:
        raise ValueError(f"the expanded tile of {cut} pixels does not zoom to {n_pixel_tile} pixels")
    if tuple(painter._tile_shape()) != (n_pixel_tile, n_pixel_tile):
        raise ValueError(painter._shape_mismatch((1, n_pixel_tile, n_pixel_tile)))
    dev = torch.device(painter.model.device)
    if isinstance(massplane, torch.Tensor):
        if massplane.device != dev:
            raise ValueError(f"the mass plane lives on {massplane.device}, the painter on {dev}")
        plane = massplane if massplane.is_contiguous() else massplane.contiguous()
        origin = (geo["x0"], geo["y0"])
    else:
        # (get_tile's own gather: the window alone crosses the host link, not the plane)
        window = get_tile(massplane, shift, tile_relative_size=delta_size / mass_size,
                          expansion_factor=tile_size / delta_size)
        if window.dtype not in (np.float32, np.float64):
            raise TypeError("the mass plane must be float32 or float64")
        plane = torch.from_numpy(np.ascontiguousarray(window)).to(dev)
        origin = (0, 0)
    if plane.dim() != 2 or plane.dtype not in (torch.float32, torch.float64):
        raise TypeError("the mass plane must be a 2-d float32 or float64 plane")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    kw = {"pixel_noise": True} if pixel_noise else {}
    if draws is not None:
        kw = {"draws": draws, "return_planes": return_planes, "moments": moments}
    return painter._paint_small_plane_device(plane, origin, cut, (geo["r0"], geo["c0"], geo["crop"]), z, tile_id, seed,
                                             subtract_minimum=subtract_minimum, field_index=j, out=out, **kw)


def paint_light_cone(painter, planes, z, delta_size, tile_size, n_pixel_tile, resolution, scales, min_tile_overlap=0.5,
                     falloff=0.05, sigma=0.5, regularise_std=None, batch_size=64, order=3, subtract_minimum=False,
                     on_device=False, seed=None, out=None, return_planes=False, field=None, pixel_noise=False,
                     small_planes_on_device=False, regularise=True, return_problematic_tiles=False,
                     max_problematic_tiles=16):
    """Mass planes in, one y map out (``process_SLICS`` followed by ``create_y_map``'s loop, process_SLICS.py:147-220 and
    55-64): plane i of the light cone is painted at redshift ``z[i]`` and projected into the (resolution, resolution)
    map with the factor ``scales[i]`` (``y_map_scales``) at once; no list of painted planes is kept.

    ``planes`` is any iterable with one entry per redshift, consumed one at a time.  Where ``delta_size[i] >=
    tile_size`` the entry is the periodic delta plane and goes through ``paint_plane`` with ``tile_relative_size =
    tile_size / delta_size[i]`` (``min_tile_overlap``, ``falloff``, ``sigma``, ``regularise_std``, ``batch_size`` are
    passed on).  Otherwise the entry is ``(massplane, shift, mass_size)`` and goes through ``paint_small_plane``.

    One Philox key serves the whole light cone (``seed``; None draws a fresh one from torch's global generator) and
    every tile has its own counter: a tiled plane takes as many tile ids as it has tiles, a small plane one.

    ``painter``: a ``CVAEPainter`` or a ``CGANPainter`` (the reference's light-cone driver takes either,
    scripts/create_lightcone.py:43-54); the key and the counters below are the CVAE's latent noise and do not affect a
    CGAN's planes.

    ``on_device=True`` (orders 2 to 5 and a painter with a device pipeline at every redshift; NotImplementedError
    otherwise, before any random number is drawn): ``paint_plane(on_device=True, out=...)`` leaves each plane in a
    device buffer that ``bp_plane_project_order`` reads on the same stream and the next plane reuses; only the finished map is downloaded,
    or nothing with ``out`` (a CUDA float64 (resolution, resolution) tensor that is accumulated into and returned).
    Small planes are painted as on the host path and uploaded, for which the stream is synchronised.

    ``small_planes_on_device=True`` (with ``on_device=True`` only; ValueError without it): small planes take
    ``paint_small_plane(on_device=True, out=...)`` into a device buffer that the projection reads on the same stream --
    no synchronisation, no upload of a painted plane; a mass plane given as a CUDA tensor is cut in place, of a host
    one only the window is uploaded.  Off by default: the device's resampled tile is within one float32 rounding of
    SciPy's and not bit-equal to it, so a small plane painted this way is not the host path's bit for bit, which it is
    with the flag off.

    ``field``: a painter with several label fields paints all of them from one latent draw, and the map is made of
    ONE: ``field`` names it (ValueError without it or for a name the painter does not paint, before any random number is
    drawn).  That field's plane is the one projected and, with ``return_planes``, kept; on the device it is a slice of
    the (F, n_plane, n_plane) buffer ``paint_plane`` blends into.  A painter with one label field needs no ``field``.

    ``pixel_noise=True`` is passed to every plane (``paint_plane`` / ``paint_small_plane``: ValueError for a painter
    without a variance head, before any random number is drawn): a tiled plane's noise lattice is its first tile id.

    ``regularise`` and ``return_problematic_tiles`` are passed to every tiled plane (``paint_plane``; ValueError without
    a ``regularise_std``, before any random number is drawn).  The cone has ONE report (``TileReport``): its per-tile
    arrays are lists with one array per tiled plane, its entries carry the plane's number and the cone's running tile
    id, and ``max_problematic_tiles`` caps the cone, not each plane.  Small planes are one unmasked tile and contribute
    nothing, as in the reference.  With ``on_device=True`` one keep buffer and one device cursor serve the whole cone:
    nothing of the report is downloaded, and the stream is not synchronised for it, until the last plane is enqueued.

    Returns the map, or (map, painted planes as host arrays) with ``return_planes=True``; with
    ``return_problematic_tiles=True`` the report is appended: (map, report) or (map, planes, report)."""
    z, delta_size = list(z), list(delta_size)
    if not len(z) == len(delta_size) == len(scales):
        raise ValueError("z, delta_size and scales need one entry per plane")
    _check_report(regularise_std, return_problematic_tiles, max_problematic_tiles)
    j = _field_index(painter, field)
    noise = {}
    if pixel_noise:
        _need_pixel_noise(painter)
        noise = {"pixel_noise": True}
    n_f = len(painter.label_fields) if j is not None else 1
    if out is not None and not on_device:
        raise ValueError("out= needs on_device=True")
    if small_planes_on_device and not on_device:
        raise ValueError("small_planes_on_device=True needs on_device=True")
    # eligibility is decided UP FRONT, as in paint_plane: no random number is drawn for a light cone that cannot run
    if on_device:
        if order not in _DEVICE_ORDERS:
            raise NotImplementedError("paint_light_cone(on_device=True) resamples with splines of order 2 to 5 only")
        if not (hasattr(painter, "_paint_plane_device") and all(painter.can_paint_stream(zi) for zi in z)):
            raise NotImplementedError("paint_light_cone(on_device=True) needs a painter with a device paint pipeline "
                                      "(CVAEPainter / CGANPainter .can_paint_stream) at every redshift")
        import torch
        dev = torch.device(painter.model.device)
        if out is not None:
            _check_map(out, resolution, dev)
    if seed is None and any(_streams(painter, zi) for zi in z):
        import torch
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    if on_device:
        y_map = out if out is not None else torch.zeros((resolution, resolution), dtype=torch.float64, device=dev)
        buf = None                                               # the painted plane, reused from plane to plane
    else:
        y_map = np.zeros((resolution, resolution))
    kept = []
    tile_id = 0
    n_done = 0
    cap = int(max_problematic_tiles)
    reports, tiled, keep = [], [], None          # the tiled planes' reports (host path), their numbers, the device's keep
    for i, entry in enumerate(planes):
        if i >= len(z):
            raise ValueError("more planes than redshifts")
        n_done += 1
        if delta_size[i] >= tile_size:
            rel = tile_size / delta_size[i]
            geo = plane_geometry(entry.shape[0], rel, n_pixel_tile, min_tile_overlap)
            kw = dict(min_tile_overlap=min_tile_overlap, falloff=falloff, sigma=sigma, regularise_std=regularise_std,
                      batch_size=batch_size, seed=seed, first_tile_id=tile_id, **noise)
            if not regularise:
                kw["regularise"] = False
            tile_id += geo["n_side"] ** 2
            if on_device:
                n_plane = geo["n_plane"]
                if buf is None or buf.numel() < n_f * n_plane * n_plane:
                    buf = None                                   # (let go of the smaller one first)
                    buf = torch.empty(n_f * n_plane * n_plane, dtype=torch.float64, device=dev)
                shape = (n_plane, n_plane) if j is None else (n_f, n_plane, n_plane)
                if return_problematic_tiles:     # paint_plane's device path, the plane's report left in the cone's keep
                    if keep is None:
                        from .painter import TileKeep
                        keep = TileKeep(painter, n_pixel_tile, cap, regularise_std)
                    tiled.append(i)
                    plane = _paint_plane_device(painter, entry, rel, n_pixel_tile, z[i], min_tile_overlap, falloff,
                                                sigma, regularise_std, batch_size, seed, kw["first_tile_id"],
                                                buf[:n_f * n_plane * n_plane].view(shape), pixel_noise, regularise,
                                                keep=keep, plane_number=i)
                else:
                    plane = paint_plane(painter, entry, rel, n_pixel_tile, z[i], on_device=True,
                                        out=buf[:n_f * n_plane * n_plane].view(shape), **kw)
            elif return_problematic_tiles:
                left = max(cap - sum(len(r.tiles) for r in reports), 0)
                plane, r = paint_plane(painter, entry, rel, n_pixel_tile, z[i], return_problematic_tiles=True,
                                       max_problematic_tiles=left, **kw)
                for e in r.tiles:
                    e.plane = i
                reports.append(r)
                tiled.append(i)
            else:
                plane = paint_plane(painter, entry, rel, n_pixel_tile, z[i], **kw)
            if j is not None:
                plane = plane[j]                                 # (a contiguous slice of the fields' planes)
        else:
            massplane, shift, mass_size = entry
            kw = dict(seed=seed, tile_id=tile_id, subtract_minimum=subtract_minimum, field=field, **noise)
            tile_id += 1
            host = None
            if small_planes_on_device:                           # one stream from the cut to the projection
                m = small_plane_geometry(massplane.shape[0], shift, delta_size[i], tile_size, mass_size,
                                         n_pixel_tile)["crop"]
                plane = paint_small_plane(painter, massplane, shift, delta_size[i], tile_size, mass_size, n_pixel_tile,
                                          z[i], on_device=True,
                                          out=torch.empty((m, m), dtype=torch.float64, device=dev), **kw)
            else:
                if on_device:                                    # paint_stream copies on streams of its own
                    torch.cuda.current_stream(dev).synchronize()
                plane = paint_small_plane(painter, massplane, shift, delta_size[i], tile_size, mass_size, n_pixel_tile,
                                          z[i], **kw)
                if on_device:
                    host = plane
                    plane = torch.from_numpy(np.ascontiguousarray(plane)).to(dev)
        if on_device:
            _project_device(plane, scales[i], y_map, order)
            if return_planes:
                kept.append(host if delta_size[i] < tile_size and host is not None else plane.cpu().numpy())
        else:
            _project_host(y_map, plane, scales[i], order)
            if return_planes:
                kept.append(plane)
    if n_done != len(z):
        raise ValueError("fewer planes than redshifts")
    if on_device and out is None:
        y_map = y_map.cpu().numpy()
    if return_problematic_tiles:
        if keep is not None:                                     # behind the last plane: one download for the cone
            reports = _report_device(keep)
        report = _cone_report(regularise_std, reports, tiled)
        return (y_map, kept, report) if return_planes else (y_map, report)
    return (y_map, kept) if return_planes else y_map


def paint_small_plane_ensemble(painter, massplane, shift, delta_size, tile_size, mass_size, n_pixel_tile, z, draws,
                               seed=None, tile_id=0, subtract_minimum=False, field=None, pixel_noise=False,
                               on_device=False, out=None, return_planes=False):
    """``paint_small_plane`` for K = ``draws`` latent draws of its one tile: the central footprint of every draw, and
    the moments across the K footprints (``ensemble_moments``): (mean, var), float64 (m, m), and with
    ``return_planes=True`` the K planes (K, m, m).  Draw l uses the Philox counter (g, l, ``tile_id``) under ``seed``:
    plane 0 is ``paint_small_plane``'s for the same seed and id.  ``field`` as there.  Refusals as in
    ``paint_plane_ensemble``; ``pixel_noise=True`` is not offered (NotImplementedError).

    Host path: ``paint_small_plane``'s cut and zoom, ``painter.paint_ensemble(..., return_draws=True)``, the crop per
    draw.  ``on_device=True``: minimum, cut, zoom, ``model.paint_graph(1, draws=K)``, one ``bp_tile_crop`` per draw and
    ``bp_plane_moments`` on one stream; ``out`` = (mean, var), two CUDA float64 (m, m) tensors, receives the result
    (nothing is downloaded; the planes, if asked for, are then a CUDA tensor).  As for single paintings, the device's
    resampled tile is within one float32 rounding of the host's and not bit-equal to it."""
    j = _field_index(painter, field)
    K = _need_ensemble(painter, [z], draws, None, pixel_noise, on_device, "paint_small_plane_ensemble",
                       "_paint_small_plane_device")
    if on_device:
        return _paint_small_plane_device(painter, massplane, shift, delta_size, tile_size, mass_size, n_pixel_tile, z,
                                         seed, tile_id, subtract_minimum, j, out, False, draws=K,
                                         return_planes=return_planes)
    if out is not None:
        raise ValueError("out= needs on_device=True")
    import scipy.ndimage
    tile = get_tile(massplane, shift, tile_relative_size=delta_size / mass_size,
                    expansion_factor=tile_size / delta_size)
    if subtract_minimum:
        tile = tile - tile.min()
    tile = scipy.ndimage.zoom(tile, zoom=n_pixel_tile / tile.shape[0], mode="mirror")
    if tile.shape != (n_pixel_tile, n_pixel_tile):
        raise ValueError(f"the expanded tile zooms to {tile.shape}, not to {n_pixel_tile} pixels")
    painted = painter.paint_ensemble(np.asarray(tile, dtype=np.float32)[None], z, draws=K, batch_size=K,
                                     tile_ids=np.array([tile_id], dtype=np.int64), seed=_fresh_seed(seed),
                                     return_draws=True)[2][0]
    if j is not None:
        painted = painted[:, j]
    centre = (1 - delta_size / tile_size) / 2
    planes = np.stack([get_tile(np.asarray(p, dtype=np.float64), shift=(centre, centre),
                                tile_relative_size=delta_size / tile_size) for p in painted])
    mean, var = ensemble_moments(planes)
    return (mean, var, planes) if return_planes else (mean, var)


def _check_map_pair(out, resolution, device):
    if not (isinstance(out, (tuple, list)) and len(out) == 2):
        raise ValueError("out must be the pair (y_mean, y_var)")
    for t in out:
        _check_map(t, resolution, device)
    if out[0].data_ptr() == out[1].data_ptr():
        raise ValueError("out must be two different tensors")


def paint_light_cone_ensemble(painter, planes, z, delta_size, tile_size, n_pixel_tile, resolution, scales, draws,
                              min_tile_overlap=0.5, falloff=0.05, sigma=0.5, regularise_std=None, batch_size=64, order=3,
                              subtract_minimum=False, on_device=False, seed=None, out=None, field=None,
                              pixel_noise=False, small_planes_on_device=False, return_maps=False):
    """The conditional mean and scatter of the Compton-y map of a light cone at fixed dark matter: ``paint_light_cone``
    with K = ``draws`` latent draws of every tile.  Every plane is painted as an ensemble (``paint_plane_ensemble`` /
    ``paint_small_plane_ensemble``), draw k's finished plane is projected into y map k exactly as ``paint_light_cone``
    projects, and after the last plane the moments are taken across the K maps: returns (y_mean, y_var), float64
    (resolution, resolution), ``y_var`` the population variance (``ensemble_moments``); ``return_maps=True`` adds the K
    maps (K, resolution, resolution).  Painted planes are not returned.

    Tile ids are allocated as ``paint_light_cone`` allocates them, and draw l of a tile uses the counter (g, l, id)
    under the one key ``seed``: map 0 is ``paint_light_cone``'s map for the same seed.  ``batch_size`` counts generator
    samples: K must divide it.  Refusals as in ``paint_plane_ensemble`` (checked at every redshift, before any random
    number is drawn), and ``pixel_noise=True`` is not offered (NotImplementedError).

    ``on_device=True`` (orders 2 to 5): the K finished planes stay in the painter's accumulators (divided in place),
    ``bp_plane_project_order`` adds plane k into map k of a (K, resolution, resolution) device buffer on the same
    stream, and ``bp_plane_moments`` reduces the maps; only the moments (and the maps, if asked for) are downloaded.
    ``out`` = (y_mean, y_var): two CUDA float64 (resolution, resolution) tensors that are FILLED (the moments of an
    accumulated map would mean nothing) and returned; the maps are then a CUDA tensor.  ``small_planes_on_device`` as in
    ``paint_light_cone``: without it small planes take the host path of ``paint_small_plane_ensemble`` and their K
    planes are uploaded."""
    z, delta_size = list(z), list(delta_size)
    if not len(z) == len(delta_size) == len(scales):
        raise ValueError("z, delta_size and scales need one entry per plane")
    j = _field_index(painter, field)
    K = _need_ensemble(painter, z, draws, batch_size, pixel_noise, on_device, "paint_light_cone_ensemble")
    if out is not None and not on_device:
        raise ValueError("out= needs on_device=True")
    if small_planes_on_device and not on_device:
        raise ValueError("small_planes_on_device=True needs on_device=True")
    if on_device:
        if order not in _DEVICE_ORDERS:
            raise NotImplementedError("paint_light_cone_ensemble(on_device=True) resamples with splines of order 2 to 5 "
                                      "only")
        import torch
        dev = torch.device(painter.model.device)
        if out is not None:
            _check_map_pair(out, resolution, dev)
        y_maps = torch.zeros((K, resolution, resolution), dtype=torch.float64, device=dev)
    else:
        y_maps = np.zeros((K, resolution, resolution))
    seed = _fresh_seed(seed)
    tile_id = 0
    n_done = 0
    for i, entry in enumerate(planes):
        if i >= len(z):
            raise ValueError("more planes than redshifts")
        n_done += 1
        if delta_size[i] >= tile_size:
            rel = tile_size / delta_size[i]
            geo = plane_geometry(entry.shape[0], rel, n_pixel_tile, min_tile_overlap)
            kw = dict(min_tile_overlap=min_tile_overlap, falloff=falloff, sigma=sigma, regularise_std=regularise_std,
                      batch_size=batch_size, seed=seed, first_tile_id=tile_id)
            tile_id += geo["n_side"] ** 2
            if on_device:
                drawn = _paint_plane_ensemble_planes(painter, entry, geo, n_pixel_tile, z[i], K, **kw)
            else:
                drawn = paint_plane_ensemble(painter, entry, rel, n_pixel_tile, z[i], K, return_planes=True, **kw)[2]
            if j is not None:
                drawn = drawn[:, j]                              # (K contiguous slices of the fields' planes)
        else:
            massplane, shift, mass_size = entry
            args = (painter, massplane, shift, delta_size[i], tile_size, mass_size, n_pixel_tile, z[i])
            kw = dict(seed=seed, tile_id=tile_id, subtract_minimum=subtract_minimum)
            tile_id += 1
            if small_planes_on_device:                           # one stream from the cut to the projection
                drawn = _paint_small_plane_device(*args, j=j, out=None, pixel_noise=False, draws=K, moments=False, **kw)
            else:
                if on_device:                                    # paint_ensemble copies on streams of its own
                    torch.cuda.current_stream(dev).synchronize()
                drawn = paint_small_plane_ensemble(*args, K, field=field, return_planes=True, **kw)[2]
                if on_device:
                    drawn = torch.from_numpy(np.ascontiguousarray(drawn)).to(dev)
        for k in range(K):
            if on_device:
                _project_device(drawn[k], scales[i], y_maps[k], order)
            else:
                _project_host(y_maps[k], drawn[k], scales[i], order)
    if n_done != len(z):
        raise ValueError("fewer planes than redshifts")
    if not on_device:
        mean, var = ensemble_moments(y_maps)
        return (mean, var, y_maps) if return_maps else (mean, var)
    import ctypes as C
    from . import _lib as L
    from .painter import _plane_moments
    with torch.no_grad(), torch.cuda.device(dev):
        sm = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        return _plane_moments(L.load(), y_maps, None, K, (resolution, resolution), out, y_maps if return_maps else None,
                              sm)


def _paint_plane_ensemble_planes(painter, delta, geo, n_pixel_tile, z, K, min_tile_overlap, falloff, sigma,
                                 regularise_std, batch_size, seed, first_tile_id):
    """The K finished planes of one tiled plane of a light-cone ensemble, on the device: a (K, [F,] n_plane, n_plane)
    CUDA tensor in the painter's accumulator, valid until the painter paints its next plane."""
    n_plane, cut, n_tiles = geo["n_plane"], geo["cut"], len(geo["origins"])
    if cut != n_pixel_tile and int(round(cut * (n_pixel_tile / cut))) != n_pixel_tile:
        raise ValueError(f"a {cut}-pixel cut does not zoom to {n_pixel_tile} pixels")
    if (geo["dst"] + n_pixel_tile > n_plane).any():
        raise ValueError("the tiling does not fit the plane")
    ids = first_tile_id + np.arange(n_tiles, dtype=np.int64)
    w = make_weight_map((n_pixel_tile, n_pixel_tile), falloff=falloff, sigma=sigma)
    return painter._paint_plane_device(delta, geo, z, w, batch_size=min(int(batch_size) // K, n_tiles), tile_ids=ids,
                                       seed=seed, regularise_std=regularise_std, draws=K, moments=False)
