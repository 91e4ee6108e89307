"""The problematic-tile report of ``lightcone.paint_plane`` / ``paint_light_cone`` on the host path, with a stub
painter whose paintings are hand-made: flat-ish tiles, some with spikes of known number (process_SLICS.py:212-216)."""
import numpy as np
import pytest

from baryon_painter_amd import lightcone as LC

TILE, N, REL, Z = 64, 150, 64 / 150, 0.42
SPIKES = {2: (1,), 5: (2,), 11: (3,)}             # tile number -> spikes (per field)
SPIKES2 = {2: (1, 0), 5: (0, 2), 11: (3, 1)}


class Stub:
    """Paints its input, times (f + 1) in field f, with ``spikes[t][f]`` pixels of tile t set to 100."""

    def __init__(self, spikes):
        self.spikes = spikes
        self.fields = len(next(iter(spikes.values())))

    def paint_batch(self, tiles, z, batch_size=64):
        out = np.stack([tiles * np.float32(f + 1) for f in range(self.fields)], axis=1)
        for t, per_field in self.spikes.items():
            for f, k in enumerate(per_field):
                out[t, f].reshape(-1)[[0, TILE * TILE - 1, 77][:k]] = 100.0
        return out[:, 0] if self.fields == 1 else out


def _delta(seed=1):
    """Uniform in [1, 2): no pixel of a tile is 3 stds from its mean unless it is a spike."""
    return np.random.Generator(np.random.PCG64(seed)).uniform(1, 2, (N, N)).astype(np.float32)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("spikes", [SPIKES, SPIKES2])
def test_host_report_names_the_spiked_tiles(spikes):
    p, delta = Stub(spikes), _delta()
    F = p.fields
    plane, rep = LC.paint_plane(p, delta, REL, TILE, Z, regularise_std=3, first_tile_id=40,
                                return_problematic_tiles=True)
    assert _same(plane, LC.paint_plane(p, delta, REL, TILE, Z, regularise_std=3, first_tile_id=40))
    n_side = LC.plane_geometry(N, REL, TILE)["n_side"]
    want = np.zeros((n_side ** 2, F), dtype=np.int32)
    for t, k in spikes.items():
        want[t] = k
    assert rep.n_outliers.dtype == np.int32 and np.array_equal(rep.n_outliers, want)
    assert rep.mean.shape == rep.std.shape == (n_side ** 2, F) and rep.mean.dtype == rep.std.dtype == np.float64
    assert rep.n_problematic == 3 and [e.tile for e in rep.tiles] == [2, 5, 11] and rep.regularise_std == 3
    origins, _ = LC.generate_tiling(N, TILE)
    painted = p.paint_batch(np.stack([np.asarray(LC.get_tile(delta, (x, y), REL), np.float32)
                                      for x in origins for y in origins]), Z)
    for e in rep.tiles:
        j, k = e.position
        assert (j, k) == divmod(e.tile, n_side) and e.tile_id == 40 + e.tile and e.z == Z and e.plane is None
        raw = np.asarray(LC.get_tile(delta, (origins[j], origins[k]), REL), np.float32)
        assert e.input.dtype == np.float32 and np.array_equal(e.input, raw)
        assert e.painted.shape == ((TILE, TILE) if F == 1 else (F, TILE, TILE)) and np.array_equal(e.painted, painted[e.tile])
        assert np.array_equal(e.n_outliers, want[e.tile])
        assert e.as_tuple()[0] == Z and e.as_tuple()[1] is e.input and e.as_tuple()[2] is e.painted
        f0 = painted[e.tile] if F == 1 else painted[e.tile, 0]
        assert rep.mean[e.tile, 0] == f0.mean() and rep.std[e.tile, 0] == f0.std()
    # the cap: the first ones, and the full number
    for cap in (0, 1, 3, 7):
        r = LC.paint_plane(p, delta, REL, TILE, Z, regularise_std=3, return_problematic_tiles=True,
                           max_problematic_tiles=cap)[1]
        assert r.n_problematic == 3 and [e.tile for e in r.tiles] == [2, 5, 11][:cap]


def test_detect_only_mode_blends_the_unmasked_plane():
    p, delta = Stub(SPIKES2), _delta(2)
    plain = LC.paint_plane(p, delta, REL, TILE, Z)
    masked, rep = LC.paint_plane(p, delta, REL, TILE, Z, regularise_std=3, return_problematic_tiles=True)
    detect, rep0 = LC.paint_plane(p, delta, REL, TILE, Z, regularise_std=3, regularise=False,
                                  return_problematic_tiles=True)
    assert _same(detect, plain) and _same(LC.paint_plane(p, delta, REL, TILE, Z, regularise_std=3, regularise=False), plain)
    assert not _same(masked, plain) and np.nanmax(masked) < 10 < np.nanmax(plain)
    assert np.array_equal(rep.n_outliers, rep0.n_outliers) and np.array_equal(rep.mean, rep0.mean)
    assert np.array_equal(rep.std, rep0.std) and rep.n_problematic == rep0.n_problematic == 3
    for a, b in zip(rep.tiles, rep0.tiles):
        assert a.tile == b.tile and np.array_equal(a.input, b.input) and np.array_equal(a.painted, b.painted)


def test_host_light_cone_report_concatenates_its_planes():
    pytest.importorskip("scipy.ndimage")
    p = Stub(SPIKES)
    planes, z, size = [_delta(3), _delta(4)], [0.3, 0.5], [150.0, 150.0]
    kw = dict(tile_size=64.0, n_pixel_tile=TILE, resolution=40, scales=[1.0, 2.0], regularise_std=3)
    y, rep = LC.paint_light_cone(p, planes, z, size, return_problematic_tiles=True, max_problematic_tiles=4, **kw)
    assert np.array_equal(y, LC.paint_light_cone(p, planes, z, size, **kw))
    assert rep.planes == [0, 1] and len(rep.n_outliers) == 2 and rep.n_problematic == 6
    assert [(e.plane, e.tile, e.tile_id) for e in rep.tiles] == [(0, 2, 2), (0, 5, 5), (0, 11, 11), (1, 2, 18)]
    assert [e.z for e in rep.tiles] == [0.3, 0.3, 0.3, 0.5]
    y0 = LC.paint_light_cone(p, planes, z, size, regularise=False, **kw)
    assert np.array_equal(y0, LC.paint_light_cone(p, planes, z, size, **dict(kw, regularise_std=None)))
    assert not np.array_equal(y0, y)


def test_report_without_a_threshold_is_refused_before_a_random_number_is_drawn():
    torch = pytest.importorskip("torch")
    p, delta = Stub(SPIKES), _delta()
    state = torch.get_rng_state()
    with pytest.raises(ValueError):
        LC.paint_plane(p, delta, REL, TILE, Z, return_problematic_tiles=True)
    with pytest.raises(ValueError):
        LC.paint_plane(p, delta, REL, TILE, Z, regularise_std=-1.0, return_problematic_tiles=True)
    with pytest.raises(ValueError):
        LC.paint_plane(p, delta, REL, TILE, Z, regularise_std=3, return_problematic_tiles=True, max_problematic_tiles=-1)
    with pytest.raises(ValueError):
        LC.paint_light_cone(p, [delta], [Z], [150.0], 64.0, TILE, 40, [1.0], return_problematic_tiles=True)
    assert torch.equal(torch.get_rng_state(), state)
