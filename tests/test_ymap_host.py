"""CPU: the y-map half of the light cone (lightcone.project_planes, pixel_area_mean, create_y_map, paint_small_plane,
paint_light_cone on the host path) against the reference loops written out here, and tests/ymap_ref.py -- the float64
restatement the GPU tests fall back to -- against SciPy."""
import numpy as np
import pytest

import ymap_ref as R
from baryon_painter_amd import lightcone as LC

nd = pytest.importorskip("scipy.ndimage")


def _lognormal(n, seed, sigma=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.exp(sigma * rng.standard_normal((n, n)))


@pytest.mark.parametrize("n,n_out", [(37, 20), (37, 37), (37, 50), (300, 257), (20, 64)])
@pytest.mark.parametrize("chunked", [False, True])
def test_restatement_equals_scipy_mirror_zoom(n, n_out, chunked):
    a = _lognormal(n, 100 + n + n_out)
    ref = nd.zoom(a, n_out / n, order=3, mode="mirror")
    assert ref.shape == (n_out, n_out)
    got = R.zoom(a, n_out, chunked=chunked)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(a).max()


def test_chunked_prefilter_equals_the_full_line():
    """A 3000-sample line in pieces of 256 and of the kernel's 224 samples with 32-sample warm-ups, against
    scipy.ndimage.spline_filter1d: double precision; a 16-sample warm-up is not."""
    rng = np.random.Generator(np.random.PCG64(5))
    x = np.exp(rng.standard_normal((3000, 3)))
    ref = nd.spline_filter1d(x, order=3, axis=0, mode="mirror")
    top = np.abs(ref).max()
    assert np.abs(R.prefilter_lines(x) - ref).max() <= 1e-15 * top
    for chunk in (256, R.CHUNK):
        assert np.abs(R.prefilter_lines_chunked(x, chunk, 32) - ref).max() <= 1e-15 * top
    assert np.abs(R.prefilter_lines_chunked(x, 256, 16) - ref).max() > 1e-13 * top
    assert R.Z ** 32 < 1e-18


def test_mirror_is_not_reflect():
    a = _lognormal(37, 6)
    assert np.abs(R.zoom(a, 50) - nd.zoom(a, 50 / 37, order=3, mode="reflect")).max() > 1e-6


def _planes_with_nans():
    planes = [_lognormal(n, 20 + n) for n in (40, 64, 75)]
    planes[0][:3] = np.nan                                       # a rim no tile reached
    planes[0][:, -2:] = np.nan
    planes[1][20:30, 5:9] = np.nan                               # an interior block
    planes[2][-1] = np.nan
    return planes


@pytest.mark.parametrize("order", [1, 3])
def test_project_planes_is_the_reference_loop(order):
    planes = _planes_with_nans()
    before = [p.copy() for p in planes]
    scales = [0.5, 3.0e-7, 12.0]
    resolution = 50
    y_map = np.zeros((resolution, resolution))                   # process_SLICS.py:55-64, zoom_factor**2 in the scale
    for i, d in enumerate(planes):
        zoom_factor = resolution / d.shape[0]
        d = d.copy()
        d[np.isnan(d)] = 0
        d *= scales[i]
        y_map += nd.zoom(d, zoom=zoom_factor, order=order, mode="mirror")
    got = LC.project_planes(planes, scales, resolution, order=order)
    assert got.dtype == np.float64 and np.array_equal(got, y_map)
    for p, b in zip(planes, before):                             # the planes are left alone, NaNs included
        assert np.array_equal(p, b, equal_nan=True)
    if order == 3:
        assert np.abs(R.project(planes, scales, resolution) - y_map).max() <= 1e-13 * np.abs(y_map).max()
    with pytest.raises(ValueError):
        LC.project_planes(planes, scales, resolution, out=np.zeros((resolution, resolution)))


def test_pixel_area_mean_known_answer():
    theta, lo, hi = 2.5e-4, 310.0, 680.0
    got = LC.pixel_area_mean(lo, hi, theta, lambda chi: 1.0)
    ref = theta ** 2 * (hi ** 3 - lo ** 3) / (3 * (hi - lo))
    assert abs(got - ref) <= 1.5e-8 * ref                        # (quad's default relative tolerance)
    a = lambda chi: 1 / (1 + chi / 3000.0)                       # noqa: E731
    k = np.linspace(lo, hi, 200001)
    f = (k * a(k) * theta) ** 2
    num = ((f[1:] + f[:-1]) / 2 * np.diff(k)).sum() / (hi - lo)          # trapezoids
    assert abs(LC.pixel_area_mean(lo, hi, theta, a) - num) <= 1e-8 * num


def test_slab_edges_clamp_the_first_plane():
    h = 0.7
    slab = 252.5 / h
    chi = np.array([100.0, 100.0 + slab, 100.0 + 2 * slab])      # the first plane is closer than half a slab
    before = chi.copy()
    e = LC.slab_edges(chi, h)
    assert np.array_equal(chi, before)
    assert e.shape == (4,) and e[0] == 0.0
    assert np.array_equal(e[1:3], chi[1:] - 252.5 / h / 2)
    assert e[3] == e[2] + 252.5 / h
    far = LC.slab_edges(chi + 500.0, h)
    assert far[0] == chi[0] + 500.0 - 252.5 / h / 2


def test_create_y_map_scales_and_projects():
    h, resolution, map_size = 0.6898, 48, 10.0
    z = [0.1, 0.4, 0.9]
    chi = np.array([120.0, 1100.0, 2200.0])
    a = lambda c: 1 / (1 + c / 3300.0)                           # noqa: E731
    planes = _planes_with_nans()
    # process_SLICS.py:25-32, 41-50, 60, evaluated here
    d_A = chi.copy()
    d_A -= 252.5 / h / 2
    assert d_A[0] < 0
    d_A[0] = 0
    d_A = np.append(d_A, d_A[-1] + 252.5 / h)
    theta_pix = map_size / resolution * np.pi / 180
    A = [LC.pixel_area_mean(d_A[i], d_A[i + 1], theta_pix, a) for i in range(3)]
    y_fac = 8.125561e-16
    mpc = 3.086e22
    eV = 1.60218e-19
    cm = 0.01
    Xe = 1.17
    Xi = 1.08
    V_c = (400 / h / 2048 * mpc / cm) ** 3
    y_fac = y_fac * eV * mpc ** -2
    scales = [V_c * (Xe + Xi) / Xe * y_fac / A[i] / (resolution / planes[i].shape[0]) ** 2 for i in range(3)]
    got = LC.y_map_scales([p.shape[0] for p in planes], resolution, map_size, chi, a, h)
    assert np.array_equal(got, np.array(scales))
    y = LC.create_y_map(planes, z, resolution, map_size, chi, a, h)
    assert np.array_equal(y, LC.project_planes(planes, scales, resolution))
    assert np.isfinite(y).all() and y.max() > 0
    with pytest.raises(ValueError):
        LC.create_y_map(planes, z[:2], resolution, map_size, chi, a, h)


class _Identity:
    """A painter that returns its input (``paint`` for single tiles, ``paint_batch`` for paint_plane)."""
    def __init__(self):
        self.calls = []

    def paint(self, input, z=0.0, transform=True, inverse_transform=True):
        self.calls.append(("paint", input.shape, z))
        return input

    def paint_batch(self, tiles, z, batch_size=64):
        self.calls.append(("paint_batch", tiles.shape, z))
        return tiles


def test_paint_small_plane_is_cut_of_zoom_of_cut():
    mass = _lognormal(120, 7)
    shift = (0.9, 0.85)                                          # wraps along both axes
    delta_size, tile_size, mass_size, n_tile = 30.0, 50.0, 100.0, 64
    # process_SLICS.py:162-175 with the reference's get_tile written out
    size = int(120 * (delta_size / mass_size) * (tile_size / delta_size))
    off = int(120 * (delta_size / mass_size) * (tile_size / delta_size - 1) / 2)
    x0, y0 = int(120 * shift[0]) - off, int(120 * shift[1]) - off
    assert x0 + size > 120 and y0 + size > 120
    tile = mass.take(range(x0, x0 + size), axis=0, mode="wrap").take(range(y0, y0 + size), axis=1, mode="wrap")
    tile = nd.zoom(tile, zoom=n_tile / tile.shape[0], mode="mirror")
    assert tile.shape == (n_tile, n_tile)
    c = int(n_tile * ((1 - delta_size / tile_size) / 2))
    m = int(n_tile * (delta_size / tile_size))
    ref = tile[c:c + m, c:c + m]
    p = _Identity()
    got = LC.paint_small_plane(p, mass, shift, delta_size, tile_size, mass_size, n_tile, 0.05)
    assert got.dtype == np.float64 and np.array_equal(got, ref)
    assert p.calls == [("paint", (n_tile, n_tile), 0.05)]
    tile = mass.take(range(x0, x0 + size), axis=0, mode="wrap").take(range(y0, y0 + size), axis=1, mode="wrap")
    tile = nd.zoom(tile - tile.min(), zoom=n_tile / tile.shape[0], mode="mirror")
    got = LC.paint_small_plane(p, mass, shift, delta_size, tile_size, mass_size, n_tile, 0.05, subtract_minimum=True)
    assert np.array_equal(got, tile[c:c + m, c:c + m])


def test_paint_light_cone_host_is_paint_plane_then_project_planes():
    import torch
    p = _Identity()
    n_tile, tile_size, resolution = 32, 50.0, 70
    z = [0.05, 0.3, 0.6]
    delta_size = [30.0, 100.0, 133.0]
    mass = _lognormal(120, 8)
    deltas = [_lognormal(64, 9), _lognormal(100, 10)]
    planes = [(mass, (0.9, 0.1), 100.0), deltas[0], deltas[1]]
    scales = [2.0, 0.25, 1e-3]
    painted = [LC.paint_small_plane(p, mass, (0.9, 0.1), 30.0, tile_size, 100.0, n_tile, z[0]),
               LC.paint_plane(p, deltas[0], tile_size / 100.0, n_tile, z[1], falloff=0.1),
               LC.paint_plane(p, deltas[1], tile_size / 133.0, n_tile, z[2], falloff=0.1)]
    assert painted[1].shape == (64, 64) and painted[2].shape == (85, 85)
    ref = LC.project_planes(painted, scales, resolution)
    state = torch.get_rng_state()
    y, kept = LC.paint_light_cone(p, iter(planes), z, delta_size, tile_size, n_tile, resolution, scales, falloff=0.1,
                                  return_planes=True)
    assert torch.equal(torch.get_rng_state(), state)             # no paint_stream: no key is drawn
    assert np.array_equal(y, ref)
    assert len(kept) == 3 and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(kept, painted))
    assert np.array_equal(LC.paint_light_cone(p, planes, z, delta_size, tile_size, n_tile, resolution, scales,
                                              falloff=0.1), ref)
    ref1 = LC.project_planes(painted, scales, resolution, order=1)
    assert np.array_equal(LC.paint_light_cone(p, planes, z, delta_size, tile_size, n_tile, resolution, scales,
                                              falloff=0.1, order=1), ref1)
    with pytest.raises(ValueError):
        LC.paint_light_cone(p, planes[:2], z, delta_size, tile_size, n_tile, resolution, scales)
    with pytest.raises(NotImplementedError):                     # no device pipeline: refused before anything is drawn
        LC.paint_light_cone(p, planes, z, delta_size, tile_size, n_tile, resolution, scales, on_device=True)
    assert torch.equal(torch.get_rng_state(), state)
    with pytest.raises(NotImplementedError):
        LC.project_planes(painted, scales, resolution, order=1, on_device=True)


def test_tile_ids_advance_from_plane_to_plane():
    """A painter with a paint_stream sees one key for the light cone and disjoint tile ids."""
    seen = []

    class Stream(_Identity):
        def can_paint_stream(self, z=0.0):
            return True

        def paint_stream(self, inputs, z, batch_size=64, tile_ids=None, seed=0):
            seen.append((int(seed), [int(t) for t in tile_ids]))
            return inputs

    import torch
    p = Stream()
    mass = _lognormal(120, 11)
    planes = [_lognormal(64, 12).astype(np.float32), (mass, (0.2, 0.3), 100.0), _lognormal(64, 13).astype(np.float32)]
    z, delta_size = [0.3, 0.05, 0.4], [100.0, 30.0, 100.0]
    LC.paint_light_cone(p, planes, z, delta_size, 50.0, 32, 40, [1.0, 1.0, 1.0], seed=17)
    assert [s for s, _ in seen] == [17, 17, 17]
    ids = [t for _, ts in seen for t in ts]
    assert ids == list(range(len(ids))) and len(seen[0][1]) == 9 and len(seen[1][1]) == 1
    del seen[:]
    torch.manual_seed(1)
    LC.paint_light_cone(p, planes, z, delta_size, 50.0, 32, 40, [1.0, 1.0, 1.0])
    LC.paint_light_cone(p, planes, z, delta_size, 50.0, 32, 40, [1.0, 1.0, 1.0])
    keys = [s for s, _ in seen]
    assert len(set(keys[:3])) == 1 and len(set(keys[3:])) == 1 and keys[0] != keys[3]
