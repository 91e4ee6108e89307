"""GPU: the problematic-tile report of ``lightcone.paint_plane`` / ``paint_light_cone`` (``on_device=True``,
``return_problematic_tiles=True``) with 64^2 synthetic painters, planes of 4 x 4 tiles and batches of 5.

The device report is held to a RECOMPUTATION from the device's own tiles: ``bp_plane_cut``'s tiles through the C ABI,
painted by ``paint_stream`` under the plane's seed and tile ids (the bits the plane pipeline blends), counted by the
float64 restatement of tests/outlier_ref.py.  Counts, the problematic set and every kept input and painting must be
EQUAL; that no pixel sits in the restatement's tie band is asserted first.  The thresholds ``STD`` were chosen at
development time, from the sorted per-tile maxima of |p - mean| / std, inside a gap of those maxima so that some tiles
are flagged and some are not (both asserted)."""
import numpy as np
import pytest
import torch

import gpu_util as G
import host_cases as HC
import multi_field_cases as MF
import outlier_ref as R
from baryon_painter_amd import _lib as L
from baryon_painter_amd import lightcone as LC
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils import datasets as D
from baryon_painter_amd.utils import synthetic as syn
from baryon_painter_amd.utils.datasets import BAHAMASDataset

pytestmark = pytest.mark.gpu

TILE, REL, SEED, BATCH = 64, 64 / 150, 6, 5
# (painter, plane) -> regularise_std, inside a gap of the plane's sorted per-tile maxima of |p - mean| / std: the maxima
# on either side of it, and how many of the 16 tiles it flags.  No other pixel of any tile is within 1e-3 of it
STD = {("cvae", "plain"): 3.628,          # 3.626931 | 3.629295: 6 tiles
       ("cvae", "zoomed"): 3.597,         # 3.595799 | 3.598379: 5 tiles (and all 16 of the plain plane)
       ("two fields", "plain"): 4.537,    # 4.535271 | 4.538632 in field 1, field 0 stays below 3.22: 9 tiles
       ("cgan", "plain"): 5.0}            # 4.983864 | 5.017496: 11 tiles


def _delta(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (np.exp(rng.standard_normal((n, n)) * 0.5) * 0.05).astype(np.float32)


def _smooth(n, seed):
    """A smooth positive periodic plane: white noise resampled by a cubic goes negative, which shift-log cannot take."""
    rng = np.random.Generator(np.random.PCG64(seed))
    k = np.fft.fftfreq(n)
    f = np.fft.ifft2(np.fft.fft2(rng.standard_normal((n, n))) * (np.hypot(k[:, None], k[None, :]) < 0.1)).real
    return (np.exp(f / f.std() * 0.5) * 0.05).astype(np.float32)


# the planes: (delta, z, first tile id) -- the ids the light cone below gives them behind its one small plane
PLAIN = (lambda: _delta(150, 41), 0.42, 17)       # 150 pixels: 64-pixel cuts, no resampling
ZOOMED = (lambda: _smooth(200, 42), 0.3, 1)       # 200 pixels: 85-pixel cuts resampled to 64


def _checkpointed(tmp, arch, ds):
    """A 64x64 CVAE painter with non-trivial running statistics, loaded from checkpoint files."""
    from baryon_painter_amd.painter import CVAEPainter
    torch.manual_seed(3)
    p = CVAEPainter(training_data_set=ds, test_data_set=ds, architecture=arch, compute_device="cuda:0")
    x, y, aux = syn.synthetic_batch(4, TILE, TILE, seed=77)
    sx = (1.0 - 0.15 * np.arange(arch["dim_x"][0], dtype=np.float32))[None, :, None, None]
    sy = (1.0 - 0.2 * np.arange(arch["dim_y"][0], dtype=np.float32))[None, :, None, None]
    with torch.no_grad():
        p.model(torch.from_numpy(x * sx), torch.from_numpy(y * sy), torch.from_numpy(aux))
    files = (str(tmp / "state"), str(tmp / "meta"))
    p.save_state_to_file(files)
    return CVAEPainter(filename=files, compute_device="cuda:0")


def build(kind, tmp):
    if kind == "cvae":
        fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
        tr = T.chain_transformations([fwd, T.atleast_3d, T.as_float32])
        itr = T.chain_transformations([T.squeeze, inv])
        ds = BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"],
                            n_tile=1, n_stack=3, transform=tr, inverse_transform=itr, scale_to_SLICS=True)
        return _checkpointed(tmp, A.fiducial_architecture(TILE), ds)
    if kind == "two fields":
        tr, itr = MF.chains(T)
        ds = BAHAMASDataset(data=MF.data_dict3(), redshifts=list(HC.REDSHIFTS), label_fields=list(MF.LABELS), n_tile=1,
                            n_stack=3, transform=tr, inverse_transform=itr, scale_to_SLICS=True)
        return _checkpointed(tmp, A.fiducial_architecture(TILE, n_fields=len(MF.LABELS)), ds)
    assert kind == "cgan"
    from baryon_painter_amd.painter import CGANPainter
    torch.manual_seed(4)
    p = CGANPainter(training_data_set=D.SyntheticTileDataset(n_sample=16, tile_size=TILE, seed=3), tile_size=TILE,
                    compute_device="cuda:0", n_res=1)
    p.train(n_iter=2, batch_size=2)
    return p


@pytest.fixture(scope="module")
def painters(tmp_path_factory):
    """kind -> painter, built once per kind."""
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = build(kind, tmp_path_factory.mktemp("ckpt"))
        return cache[kind]
    return get


_tiles = {}


def device_tiles(p, kind, which):
    """(raw, painted) of a plane as its device pipeline sees them, computed once per (painter, plane) and shared:
    ``bp_plane_cut``'s (n, 64, 64) float32 tiles and ``paint_stream``'s paintings of them, (n, 64, 64) or (n, F, 64, 64)."""
    make, z, first = which
    key = (kind, first)
    if key not in _tiles:
        lib = L.load()
        delta = make()
        geo = LC.plane_geometry(delta.shape[0], REL, TILE)
        n, cut = len(geo["origins"]), geo["cut"]
        d, org = G.dev(delta), G.dev(geo["origins"], torch.int32)
        raw = torch.full((n, TILE, TILE), float("nan"), device="cuda")
        ws = int(lib.bp_plane_cut_workspace(n, cut, TILE))
        scratch = torch.empty(max(ws // 8, 1), dtype=torch.float64, device="cuda")
        L.check(lib.bp_plane_cut(L.ptr(d), L.F32, delta.shape[0], delta.shape[1], L.ptr(org), n, cut, TILE,
                                 L.ptr(scratch), ws, L.ptr(raw), G.stream()), "plane cut")
        raw = raw.cpu().numpy()
        painted = p.paint_stream(raw, z, batch_size=BATCH, tile_ids=first + np.arange(n, dtype=np.int64), seed=SEED)
        for a in (raw, painted):
            a.setflags(write=False)
        _tiles[key] = (raw, painted)
    return _tiles[key]


def expected(painted, r, tie=R.TIE):
    """(mean, std, counts) as (n, F) arrays and the problematic tile numbers, from the restatement; asserts that its
    tie band is empty."""
    n = len(painted)
    F = painted.shape[1] if painted.ndim == 4 else 1
    mean, std, counts, ties = R.outliers(painted.reshape(n * F, TILE, TILE), r, tie)
    assert not ties.any()
    return mean.reshape(n, F), std.reshape(n, F), counts.reshape(n, F), R.problematic(counts, F)


def check_report(rep, raw, painted, r, z, first, cap=16, plane=None):
    mean, std, counts, bad = expected(painted, r)
    assert 0 < len(bad) < len(painted), bad                      # some tiles are flagged and some are not
    assert rep.n_outliers.dtype == np.int32 and np.array_equal(rep.n_outliers, counts)
    assert rep.mean.dtype == rep.std.dtype == np.float64
    assert np.abs(rep.mean - mean).max() <= 1e-12 * np.abs(mean).max() and np.abs(rep.std - std).max() <= 1e-12 * std.max()
    assert rep.n_problematic == len(bad) and [e.tile for e in rep.tiles] == list(bad[:cap])
    n_side = int(round(len(painted) ** 0.5))
    for e in rep.tiles:
        assert e.position == divmod(e.tile, n_side) and e.tile_id == first + e.tile and e.z == z and e.plane == plane
        assert e.input.dtype == e.painted.dtype == np.float32
        assert np.array_equal(e.input, raw[e.tile]) and np.array_equal(e.painted, painted[e.tile])
        assert np.array_equal(e.n_outliers, counts[e.tile])
    return bad


def same_report(a, b):
    assert np.array_equal(a.n_outliers, b.n_outliers) and a.n_problematic == b.n_problematic
    assert np.array_equal(a.mean, b.mean, equal_nan=True) and np.array_equal(a.std, b.std, equal_nan=True)
    assert [(e.tile, e.tile_id, e.plane) for e in a.tiles] == [(e.tile, e.tile_id, e.plane) for e in b.tiles]
    for e, f in zip(a.tiles, b.tiles):
        assert np.array_equal(e.input, f.input) and np.array_equal(e.painted, f.painted)
        assert np.array_equal(e.n_outliers, f.n_outliers)


def same_plane(a, b):
    assert np.array_equal(a, b, equal_nan=True) and np.isfinite(a).mean() > 0.9


def paint(p, which, r, **kw):
    make, z, first = which
    return LC.paint_plane(p, make(), REL, TILE, z, seed=SEED, first_tile_id=first, batch_size=BATCH, on_device=True,
                          regularise_std=r, **kw)


def blend(painted, n_plane, r):
    """``bp_plane_blend`` / ``bp_plane_finish`` of all tiles of one field in one batch, through the C ABI."""
    lib = L.load()
    geo = LC.plane_geometry(n_plane, REL, TILE)
    n, dst = len(painted), geo["dst"]
    td, dd = G.dev(np.array(painted)), G.dev(dst, torch.int32)   # (a copy: the shared tiles are read-only)
    wd = G.dev(LC.make_weight_map((TILE, TILE), falloff=0.05, sigma=0.5), torch.float64)
    acc = torch.zeros((n_plane, n_plane), dtype=torch.float64, device="cuda")
    wsum, out = torch.zeros_like(acc), torch.zeros_like(acc)
    stats = torch.empty(2 * n, dtype=torch.float64, device="cuda")
    L.check(lib.bp_plane_blend(L.ptr(td), n, TILE, L.ptr(dd), int(dst[:, 0].min()), int(dst[:, 1].min()),
                               int(dst[:, 0].max()) + TILE, int(dst[:, 1].max()) + TILE, L.ptr(wd), 0 if r is None else 1,
                               0.0 if r is None else float(r), L.ptr(stats), L.ptr(acc), L.ptr(wsum), n_plane, n_plane,
                               G.stream()), "plane blend")
    L.check(lib.bp_plane_finish(L.ptr(acc), L.ptr(wsum), n_plane * n_plane, L.ptr(out), G.stream()), "plane finish")
    return out.cpu().numpy()


def test_device_report_equals_the_recomputation(painters):
    p, r = painters("cvae"), STD["cvae", "plain"]
    raw, painted = device_tiles(p, "cvae", PLAIN)
    plane, rep = paint(p, PLAIN, r, return_problematic_tiles=True)
    check_report(rep, raw, painted, r, PLAIN[1], PLAIN[2])
    # the default path is what it was: the blend of those tiles, with the report and without it
    ref = blend(painted, 150, r)
    same_plane(plane, ref)
    same_plane(paint(p, PLAIN, r), ref)
    same_plane(paint(p, PLAIN, None), blend(painted, 150, None))
    assert not np.array_equal(ref, blend(painted, 150, None), equal_nan=True)
    # out= keeps its meaning
    out = torch.full((150, 150), 3.0, dtype=torch.float64, device="cuda")
    got, rep2 = paint(p, PLAIN, r, return_problematic_tiles=True, out=out)
    assert got is out
    same_plane(out.cpu().numpy(), ref)
    same_report(rep2, rep)


def test_detect_only_mode(painters):
    p, r = painters("cvae"), STD["cvae", "plain"]
    plain = paint(p, PLAIN, None)
    detect, rep0 = paint(p, PLAIN, r, regularise=False, return_problematic_tiles=True)
    same_plane(detect, plain)
    same_plane(paint(p, PLAIN, r, regularise=False), plain)
    masked, rep = paint(p, PLAIN, r, return_problematic_tiles=True)
    assert not np.array_equal(masked, plain, equal_nan=True)
    same_report(rep0, rep)


def test_cap_keeps_the_first_tiles_and_counts_all(painters):
    p, r = painters("cvae"), STD["cvae", "plain"]
    raw, painted = device_tiles(p, "cvae", PLAIN)
    bad = expected(painted, r)[3]
    assert len(bad) >= 2
    for cap in (0, 1, len(bad) - 1):
        rep = paint(p, PLAIN, r, return_problematic_tiles=True, max_problematic_tiles=cap)[1]
        assert len(rep.tiles) == cap
        check_report(rep, raw, painted, r, PLAIN[1], PLAIN[2], cap=cap)


def test_zoomed_plane_reports_the_zoomed_input(painters):
    p, r = painters("cvae"), STD["cvae", "zoomed"]
    assert LC.plane_geometry(200, REL, TILE)["cut"] == 85
    raw, painted = device_tiles(p, "cvae", ZOOMED)
    plane, rep = paint(p, ZOOMED, r, return_problematic_tiles=True)
    check_report(rep, raw, painted, r, ZOOMED[1], ZOOMED[2])
    same_plane(plane, blend(painted, 150, r))


def test_two_field_painter(painters):
    p, r = painters("two fields"), STD["two fields", "plain"]
    raw, painted = device_tiles(p, "two fields", PLAIN)
    assert painted.shape[1:] == (2, TILE, TILE)
    plane, rep = paint(p, PLAIN, r, return_problematic_tiles=True)
    check_report(rep, raw, painted, r, PLAIN[1], PLAIN[2])
    assert rep.n_outliers.shape == (16, 2) and rep.tiles[0].painted.shape == (2, TILE, TILE)
    assert ((rep.n_outliers != 0).sum(axis=1) == 1).any()        # a tile flagged in one of its fields alone
    for f in range(2):
        same_plane(plane[f], blend(np.ascontiguousarray(painted[:, f]), 150, r))


def test_cgan_painter(painters):
    p, r = painters("cgan"), STD["cgan", "plain"]
    raw, painted = device_tiles(p, "cgan", PLAIN)
    plane, rep = paint(p, PLAIN, r, return_problematic_tiles=True)
    check_report(rep, raw, painted, r, PLAIN[1], PLAIN[2])
    same_plane(plane, blend(painted, 150, r))


def test_host_report_equals_device_report_outside_the_tie_band(painters):
    """The host path counts with NumPy's float32 sums, the device with float64 ones: ``paint_plane`` documents a tie
    band of 1e-6 around the threshold.  For this plane the band is empty (asserted), so the reports are equal."""
    p, r = painters("cvae"), STD["cvae", "plain"]
    raw, painted = device_tiles(p, "cvae", PLAIN)
    expected(painted, r, tie=1e-6)
    make, z, first = PLAIN
    host_plane, host = LC.paint_plane(p, make(), REL, TILE, z, seed=SEED, first_tile_id=first, batch_size=BATCH,
                                      regularise_std=r, return_problematic_tiles=True)
    dev_plane, dev = paint(p, PLAIN, r, return_problematic_tiles=True)
    assert np.array_equal(host.n_outliers, dev.n_outliers) and host.n_problematic == dev.n_problematic
    assert [(e.tile, e.tile_id, e.position) for e in host.tiles] == [(e.tile, e.tile_id, e.position) for e in dev.tiles]
    for e, f in zip(host.tiles, dev.tiles):                      # cut == tile: the same tiles bit for bit
        assert np.array_equal(e.input, f.input) and np.array_equal(e.painted, f.painted)
    assert np.abs(host.mean - dev.mean).max() <= 1e-5 * np.abs(dev.mean).max()
    assert np.abs(host.std - dev.std).max() <= 1e-5 * dev.std.max()
    same_plane(host_plane, dev_plane)


def test_light_cone_report_concatenates_its_planes(painters):
    pytest.importorskip("scipy.ndimage")              # (the small plane is cut and zoomed with SciPy on the host)
    p, r = painters("cvae"), STD["cvae", "zoomed"]
    planes = [(_smooth(256, 43), (0.9, 0.85), 128.0), ZOOMED[0](), PLAIN[0]()]
    z, size = [0.05, ZOOMED[1], PLAIN[1]], [32.0, 150.0, 150.0]
    kw = dict(tile_size=64.0, n_pixel_tile=TILE, resolution=96, batch_size=BATCH, scales=[1.5, 0.5, 2.0], seed=SEED,
              on_device=True, regularise_std=r)
    y, rep = LC.paint_light_cone(p, iter(planes), z, size, return_problematic_tiles=True, max_problematic_tiles=64, **kw)
    assert np.array_equal(y, LC.paint_light_cone(p, planes, z, size, **kw)) and np.isfinite(y).all()
    one = [paint(p, w, r, return_problematic_tiles=True, max_problematic_tiles=64)[1] for w in (ZOOMED, PLAIN)]
    assert rep.planes == [1, 2] and len(rep.n_outliers) == len(rep.mean) == len(rep.std) == 2
    assert rep.n_problematic == one[0].n_problematic + one[1].n_problematic == len(rep.tiles)
    assert len(one[0].tiles) > 0 and len(one[1].tiles) > 0
    for i, o in enumerate(one):
        assert np.array_equal(rep.n_outliers[i], o.n_outliers) and np.array_equal(rep.mean[i], o.mean)
        assert np.array_equal(rep.std[i], o.std)
    both = [(i + 1, e) for i, o in enumerate(one) for e in o.tiles]
    assert [(e.plane, e.tile, e.tile_id, e.z) for e in rep.tiles] == [(i, e.tile, e.tile_id, e.z) for i, e in both]
    for e, (_, f) in zip(rep.tiles, both):
        assert np.array_equal(e.input, f.input) and np.array_equal(e.painted, f.painted)
        assert np.array_equal(e.n_outliers, f.n_outliers)
    # the cap is the cone's: the first plane's tiles and one of the second's
    cap = len(one[0].tiles) + 1
    y2, planes2, capped = LC.paint_light_cone(p, planes, z, size, return_problematic_tiles=True, return_planes=True,
                                              max_problematic_tiles=cap, **kw)
    assert np.array_equal(y2, y) and len(planes2) == 3
    assert capped.n_problematic == rep.n_problematic
    assert [(e.plane, e.tile) for e in capped.tiles] == [(e.plane, e.tile) for e in rep.tiles[:cap]]
    # detect-only: the cone without a threshold
    y0 = LC.paint_light_cone(p, planes, z, size, regularise=False, **kw)
    assert np.array_equal(y0, LC.paint_light_cone(p, planes, z, size, **dict(kw, regularise_std=None)))
    assert not np.array_equal(y0, y)


def test_report_without_a_threshold_is_refused_before_any_side_effect(painters):
    p = painters("cvae")
    delta = PLAIN[0]()
    n_graphs = len(p.model._graphs)
    state = torch.get_rng_state()
    for on_device in (True, False):
        with pytest.raises(ValueError):
            LC.paint_plane(p, delta, REL, TILE, 0.42, on_device=on_device, return_problematic_tiles=True)
        with pytest.raises(ValueError):
            LC.paint_light_cone(p, [delta], [0.42], [150.0], 64.0, TILE, 96, [1.0], on_device=on_device,
                                return_problematic_tiles=True)
    assert torch.equal(torch.get_rng_state(), state) and len(p.model._graphs) == n_graphs
