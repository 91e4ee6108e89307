"""CPU: tests/small_plane_ref.py -- the restatement the GPU tests of the device small plane compare with -- against
``lightcone.get_tile`` (bit for bit: the integer steps) and ``scipy.ndimage.zoom(mode="mirror")`` (1e-13 of the window's
maximum, before the rounding to float32), ``lightcone.small_plane_geometry`` against the reference's expressions, and
the keyword checks of ``paint_light_cone`` that need no GPU."""
import numpy as np
import pytest

import small_plane_ref as S
from baryon_painter_amd import lightcone as LC


def _smooth(n, m, seed, dtype):
    """A smooth positive periodic rows x cols plane (as ``_smooth`` of tests/test_gpu_ymap.py)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ky, kx = np.fft.fftfreq(n) * n, np.fft.fftfreq(m) * m
    keep = np.hypot(ky[:, None] / n, kx[None, :] / m) < 0.1
    f = np.fft.ifft2(np.fft.fft2(rng.standard_normal((n, m))) * keep).real
    return (np.exp(f / f.std() * 0.5) * 0.05).astype(dtype)


# (shift, delta_size, tile_size, mass_size) on a 120-pixel mass plane of size 100: the window's origin is negative,
# past the edge, and straddles the corner; the last has no expansion at all
CASES = [((0.05, 0.02), 30.0, 50.0, 100.0), ((1.2, 1.15), 30.0, 50.0, 100.0), ((0.9, 0.85), 30.0, 50.0, 100.0),
         ((0.3, 0.95), 20.0, 64.0, 100.0), ((0.5, 0.5), 50.0, 50.0, 100.0)]


@pytest.mark.parametrize("shift,delta_size,tile_size,mass_size", CASES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_integer_steps_are_get_tile(shift, delta_size, tile_size, mass_size, dtype):
    mass = _smooth(120, 120, 3, dtype)
    n_tile = 64
    (x0, y0, cut), (r0, c0, m) = S.geometry(120, shift, delta_size, tile_size, mass_size, n_tile)
    ref = LC.get_tile(mass, shift, tile_relative_size=delta_size / mass_size, expansion_factor=tile_size / delta_size)
    got = S.wrapped_window(mass, x0, y0, cut)
    assert got.dtype == dtype and got.shape == (cut, cut) and np.array_equal(got, ref)
    geo = LC.small_plane_geometry(120, shift, delta_size, tile_size, mass_size, n_tile)
    assert (geo["x0"], geo["y0"], geo["cut"], geo["r0"], geo["c0"], geo["crop"]) == (x0, y0, cut, r0, c0, m)
    rng = np.random.Generator(np.random.PCG64(4))
    painted = rng.standard_normal((n_tile, n_tile)).astype(np.float32)
    centre = (1 - delta_size / tile_size) / 2
    ref = LC.get_tile(np.asarray(painted, dtype=np.float64), shift=(centre, centre),
                      tile_relative_size=delta_size / tile_size)
    got = S.crop(painted, r0, c0, m)
    assert got.dtype == np.float64 and np.array_equal(got, ref)


def test_the_cases_wrap_as_they_say():
    org = [S.geometry(120, *c, 64)[0] for c in CASES]
    assert org[0][0] < 0 and org[0][1] < 0                                          # negative
    assert org[1][0] >= 120 and org[1][1] >= 120                                    # past the edge
    assert org[2][0] < 120 < org[2][0] + org[2][2] and org[2][1] < 120 < org[2][1] + org[2][2]    # the corner


def test_non_square_plane_wraps_each_axis_by_its_own_length():
    mass = _smooth(100, 155, 5, np.float32)
    for x0, y0, size in [(0, 0, 64), (-37, 250, 64), (95, -5, 40)]:
        ref = mass.take(range(x0, x0 + size), axis=0, mode="wrap").take(range(y0, y0 + size), axis=1, mode="wrap")
        assert np.array_equal(S.wrapped_window(mass, x0, y0, size), ref)
    img = mass[:64, :64]
    ref = img.take(range(50, 80), axis=0, mode="wrap").take(range(60, 90), axis=1, mode="wrap")
    assert np.array_equal(S.crop(img, 50, 60, 30), ref.astype(np.float64))


@pytest.mark.parametrize("shift,delta_size,tile_size,mass_size", CASES[:4])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("subtract_minimum", [False, True])
def test_zoom_is_scipy_before_the_rounding(shift, delta_size, tile_size, mass_size, dtype, subtract_minimum):
    nd = pytest.importorskip("scipy.ndimage")
    mass = _smooth(120, 120, 6, dtype)
    n_tile = 64
    tile = LC.get_tile(mass, shift, tile_relative_size=delta_size / mass_size, expansion_factor=tile_size / delta_size)
    (x0, y0, cut), _ = S.geometry(120, shift, delta_size, tile_size, mass_size, n_tile)
    if subtract_minimum:
        tile = tile - tile.min()                                 # (in the plane's dtype, as paint_small_plane does)
    assert tile.dtype == dtype
    ref = nd.zoom(tile.astype(np.float64), zoom=n_tile / tile.shape[0], mode="mirror")
    assert ref.shape == (n_tile, n_tile)
    for chunked in (False, True):
        got = S.zoom64(S.wrapped_window(mass, x0, y0, cut), n_tile, subtract_minimum, chunked)
        assert got.dtype == np.float64
        assert np.abs(got - ref).max() <= 1e-13 * np.abs(tile).max()
    # what the host path hands the network: SciPy's zoom in the tile's dtype, as float32
    host = np.asarray(nd.zoom(tile, zoom=n_tile / tile.shape[0], mode="mirror"), dtype=np.float32)
    got = S.tile32(S.wrapped_window(mass, x0, y0, cut), n_tile, subtract_minimum)
    assert got.dtype == np.float32
    assert (np.abs(got.astype(np.float64) - ref) <= S.ulp32(ref) / 2 + 1e-13 * np.abs(tile).max()).all()
    print(f"bit-equal to the host path's tile: {(got == host).mean():.4f} of the pixels")


def test_ulp32():
    x = np.array([1.0, 1.5, 1.9999999, 2.0, 0.75, 3e-40, 0.0])
    ref = [2.0 ** -23, 2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24, 2.0 ** -149, 2.0 ** -149]
    assert np.array_equal(S.ulp32(x), np.array(ref))
    assert np.array_equal(S.ulp32(-x), np.array(ref))


def test_slics_geometry():
    """The reference driver's numbers: 12288-pixel mass planes of 505 Mpc/h, 100 Mpc/h tiles of 512 pixels, and the
    two planes of a 10 degree field that are smaller than a tile."""
    for delta_size, crop in ((22.0, int(512 * 22 / 100)), (66.0, int(512 * 66 / 100))):
        geo = LC.small_plane_geometry(12288, (0.3, 0.7), delta_size, 100.0, 505.0, 512)
        (x0, y0, cut), (r0, c0, m) = S.geometry(12288, (0.3, 0.7), delta_size, 100.0, 505.0, 512)
        assert cut == 2433 and geo["cut"] == 2433
        assert m == crop and geo["crop"] == crop
        assert (geo["x0"], geo["y0"], geo["r0"], geo["c0"]) == (x0, y0, r0, c0)
        assert int(round(cut * (512 / cut))) == 512              # SciPy's zoom comes out at the tile's size
        assert r0 == int(512 * (1 - delta_size / 100.0) / 2) and r0 + m <= 512
    with pytest.raises(ValueError):
        LC.small_plane_geometry(12288, (0.3, 0.7), 150.0, 100.0, 505.0, 512)        # not a small plane


def test_small_planes_on_device_needs_on_device():
    import torch

    class Host:
        def paint(self, input, z=0.0, transform=True, inverse_transform=True):
            raise AssertionError("nothing is painted")

    mass = _smooth(120, 120, 7, np.float32)
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="small_planes_on_device"):
        LC.paint_light_cone(Host(), [(mass, (0.9, 0.1), 100.0)], [0.05], [30.0], 50.0, 32, 40, [1.0],
                            small_planes_on_device=True)
    with pytest.raises(ValueError, match="out="):
        LC.paint_small_plane(Host(), mass, (0.9, 0.1), 30.0, 50.0, 100.0, 32, 0.05, out=np.zeros((19, 19)))
    with pytest.raises(NotImplementedError):                     # no device pipeline: refused before anything is drawn
        LC.paint_small_plane(Host(), mass, (0.9, 0.1), 30.0, 50.0, 100.0, 32, 0.05, on_device=True)
    assert torch.equal(torch.get_rng_state(), state)
