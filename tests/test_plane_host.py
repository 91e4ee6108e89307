"""Host side of the device light-cone planes (lightcone.paint_plane(on_device=True), csrc/plane.hip): the entry points
are built, the float64 restatement the resampling kernel follows reproduces scipy.ndimage.zoom at the sizes pinned here
(63 ... 300), and the geometry helper gives the integers of get_tile / generate_tiling.  The restatement is the exact
cubic spline under half-sample symmetric boundaries; SciPy's zoom is that for lines of 12 samples and more, and departs
from it below (7e-6 of the largest value at 4 samples, 6e-4 at 2): tests/test_plane_kernels_host.py pins and records
both."""
import numpy as np
import pytest

import plane_ref as R
from baryon_painter_amd import lightcone as LC


def test_plane_symbols_resolve():
    from baryon_painter_amd import _lib as L
    lib = L.load()
    for name in ("bp_plane_cut_workspace", "bp_plane_cut", "bp_plane_blend", "bp_plane_finish"):
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert lib.bp_plane_cut_workspace(3, 80, 64) == 2 * 3 * 80 * 80 * 8
    assert lib.bp_plane_cut_workspace(3, 64, 64) == 0


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("n_in,exact", [(63, True), (80, True), (100, True), (300, False)])
def test_spline_restatement_matches_scipy_zoom(n_in, exact):
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.Generator(np.random.PCG64(n_in))
    n_out = 64 if n_in < 300 else 256
    a = np.exp(rng.standard_normal((n_in, n_in)) * 0.5) * 0.05 - 0.01           # signs of both kinds
    ref = nd.zoom(a, n_out / n_in, order=3, mode="reflect")
    got = R.zoom(a, n_out)
    assert ref.shape == got.shape == (n_out, n_out)
    u = _ulps(got, ref)
    if exact:
        assert u.max() == 0
    else:
        assert u.max() <= 1
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_spline_restatement_on_float32_input():
    nd = pytest.importorskip("scipy.ndimage")
    a = (np.random.Generator(np.random.PCG64(9)).standard_normal((85, 85))).astype(np.float32)
    ref = nd.zoom(a, 64 / 85, order=3, mode="reflect")                           # float32 out, float64 inside
    assert ref.dtype == np.float32
    assert _ulps(R.zoom(a, 64), ref).max() == 0


@pytest.mark.parametrize("n_delta,n_tile,n_plane", [(150, 64, 150), (200, 64, 150), (100, 64, 100), (137, 64, 121),
                                                    (625, 512, 4096), (1500, 512, 4096), (60, 64, 64 / 0.4)])
def test_geometry_matches_get_tile_and_generate_tiling(n_delta, n_tile, n_plane):
    rel = n_tile / n_plane
    geo = LC.plane_geometry(n_delta, rel, n_tile, 0.5)
    origins, slices = LC.generate_tiling(int(n_tile / rel), n_tile, 0.5)
    assert geo["n_plane"] == int(n_tile / rel) and geo["n_side"] == len(origins)
    assert geo["origins"].dtype == np.int32 and geo["dst"].dtype == np.int32
    assert len(geo["origins"]) == len(geo["dst"]) == len(origins) ** 2
    # get_tile's cut, by probing it with a plane whose value encodes its coordinates
    delta = np.arange(n_delta * n_delta, dtype=np.int64).reshape(n_delta, n_delta)
    t = 0
    for j, xs in enumerate(origins):
        for k, ys in enumerate(origins):
            cut = LC.get_tile(delta, (xs, ys), rel)
            assert cut.shape == (geo["cut"], geo["cut"])
            x0, y0 = geo["origins"][t]
            assert cut[0, 0] == delta[x0 % n_delta, y0 % n_delta]
            rows = (x0 + np.arange(geo["cut"])) % n_delta
            cols = (y0 + np.arange(geo["cut"])) % n_delta
            assert np.array_equal(cut, delta[np.ix_(rows, cols)])
            sx, sy = slices[j][k]
            assert (sx.start, sy.start) == tuple(geo["dst"][t])
            assert sx.stop - sx.start == n_tile
            t += 1


def test_blend_restatement_equals_the_host_loop():
    """plane_ref.blend without regularisation is the host loop of paint_plane (what the GPU blend is held to)."""
    rng = np.random.Generator(np.random.PCG64(4))
    n_tile, n_plane = 64, 150
    geo = LC.plane_geometry(n_plane, n_tile / n_plane, n_tile)
    tiles = rng.standard_normal((len(geo["dst"]), n_tile, n_tile)).astype(np.float32)
    w = LC.make_weight_map((n_tile, n_tile), falloff=0.05, sigma=0.5)
    origins, slices = LC.generate_tiling(n_plane, n_tile)
    acc, wsum = np.zeros((n_plane, n_plane)), np.zeros((n_plane, n_plane))
    it = iter(tiles)
    for j in range(len(origins)):
        for k in range(len(origins)):
            p = next(it)
            acc[slices[j][k]] += w * p
            wsum[slices[j][k]] += w
    with np.errstate(invalid="ignore"):
        ref = acc / wsum
    got = R.blend(tiles, geo["dst"], n_plane, w)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got[~np.isnan(ref)], ref[~np.isnan(ref)])
