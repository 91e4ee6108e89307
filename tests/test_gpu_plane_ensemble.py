"""GPU: ensembles of planes and light cones (lightcone.paint_plane_ensemble, paint_small_plane_ensemble,
paint_light_cone_ensemble): every draw blended, or projected, on its own and the moments across the K results.

The painter is the 64^2 painter of tests/test_gpu_paint_plane_device.py with the running statistics settled as in
tests/test_gpu_ensemble_paint.py (thirty training-mode forwards), so that the draws of a tile differ by far more than
the comparisons resolve.  Plane 0 against ``paint_plane(on_device=True)`` and map 0 against ``paint_light_cone``: equal
bits.  The device planes against the host path's: the limits of tests/test_gpu_paint_plane_device.py (1e-6 of the
plane's maximum without resampling, 1e-5 with it or with ``regularise_std``).  The moments against the float64 loop of
tests/plane_ensemble_ref.py over the returned planes or maps: equal bits."""
import numpy as np
import pytest
import torch

import host_cases as HC
import multi_field_cases as MF
import plane_ensemble_ref as R
import test_gpu_multi_field_painter as MFP
import test_gpu_paint_plane_device as PD
import test_gpu_small_plane as SP
from baryon_painter_amd import lightcone as LC
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils import synthetic as syn
from baryon_painter_amd.utils.datasets import BAHAMASDataset

pytestmark = pytest.mark.gpu

TILE, N_PLANE, K = 64, 150, 3
REL = TILE / N_PLANE
Z = 0.42
N_TILES = 16                                      # 4 x 4 tiles of 64 pixels cover 150 with at least half a tile of overlap
ONE, FOUR = K, 4 * K                              # batch sizes (generator samples) that carry 1 tile and 4 tiles
LOOSEST = 1e-5                                    # the loosest limit a plane is compared within, of its maximum


def _settle(q):
    """Thirty training-mode forwards without gradients: p_z_in's batch-norm statistics settle and the latent matters
    (tests/test_gpu_ensemble_paint.py)."""
    x, y, aux = syn.synthetic_batch(4, TILE, TILE, seed=77)
    sx = np.ones((1, q.model.dim_x[0], 1, 1), np.float32) if q.model.dim_x[0] == 1 else \
        (1.0 - 0.15 * np.arange(q.model.dim_x[0], dtype=np.float32))[None, :, None, None]
    q.model.train(True)
    with torch.no_grad():
        for _ in range(30):
            q.model(torch.from_numpy(x * sx), torch.from_numpy(y), torch.from_numpy(aux))
    q.model.train(False)
    return q


@pytest.fixture(scope="module")
def painter(tmp_path_factory):
    from baryon_painter_amd.painter import CVAEPainter
    arch = A.fiducial_architecture(TILE)
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    tr = T.chain_transformations([fwd, T.atleast_3d, T.as_float32])
    itr = T.chain_transformations([T.squeeze, inv])
    ds = BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=1,
                        n_stack=3, transform=tr, inverse_transform=itr, scale_to_SLICS=True)
    torch.manual_seed(3)
    p = CVAEPainter(training_data_set=ds, test_data_set=ds, architecture=arch, compute_device="cuda:0")
    x, y, aux = syn.synthetic_batch(4, TILE, TILE, seed=77)
    with torch.no_grad():
        p.model(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
    d = tmp_path_factory.mktemp("ckpt")
    files = (str(d / "state"), str(d / "meta"))
    p.save_state_to_file(files)
    return _settle(CVAEPainter(filename=files, compute_device="cuda:0"))


def _moments_of(mean, var, planes):
    m, v = R.moments(np.asarray(planes))
    assert mean.dtype == var.dtype == np.float64 and mean.shape == var.shape == planes.shape[1:]
    assert R.same_bits(mean, m) and R.same_bits(var, v)


def _same(a, b):
    assert R.same_bits(np.asarray(a), np.asarray(b))


@pytest.fixture(scope="module")
def plain(painter):
    """The ensemble every test of the plain geometry shares: K = 3 over ``_delta(150, 41)``, one tile per batch."""
    delta = PD._delta(N_PLANE, 41)
    kw = dict(seed=5, first_tile_id=7)
    return delta, kw, LC.paint_plane_ensemble(painter, delta, REL, TILE, Z, K, batch_size=ONE, on_device=True,
                                              return_planes=True, **kw)


def test_plane_ensemble_without_zoom(painter, plain):
    q = painter
    delta, kw, (mean, var, planes) = plain
    assert LC.plane_geometry(N_PLANE, REL, TILE)["n_side"] ** 2 == N_TILES
    assert planes.shape == (K, N_PLANE, N_PLANE) and planes.dtype == np.float64
    ok = np.isfinite(planes[0])
    assert ok.mean() > 0.9 and all(np.array_equal(np.isfinite(p), ok) for p in planes)
    # the draws differ by far more than any comparison below resolves: the variance is not rounding
    top = np.abs(planes[0][ok]).max()
    apart = np.abs(planes[1][ok] - planes[0][ok]).max() / top
    print("draws 0 and 1 differ by", apart, "of the plane's maximum")
    assert apart > LOOSEST
    # plane 0 is paint_plane's plane for the same seed and ids, bit for bit
    PD._same_plane(planes[0], LC.paint_plane(q, delta, REL, TILE, Z, batch_size=4, on_device=True, **kw))
    # the moments are those of the returned planes
    _moments_of(mean, var, planes)
    assert (var[ok] > 0).any() and (var[ok] >= 0).all() and np.isnan(var[~ok]).all() and np.isnan(mean[~ok]).all()
    # four tiles per batch: equal bits
    wide = LC.paint_plane_ensemble(q, delta, REL, TILE, Z, K, batch_size=FOUR, on_device=True, return_planes=True, **kw)
    for a, b in zip(wide, (mean, var, planes)):
        _same(a, b)
    # without the planes: the same moments
    pair = LC.paint_plane_ensemble(q, delta, REL, TILE, Z, K, batch_size=FOUR, on_device=True, **kw)
    assert len(pair) == 2
    _same(pair[0], mean), _same(pair[1], var)
    # every plane against the host path's plane
    h_mean, h_var, h_planes = LC.paint_plane_ensemble(q, delta, REL, TILE, Z, K, batch_size=FOUR, return_planes=True, **kw)
    assert h_planes.shape == planes.shape and h_planes.dtype == np.float64
    for k in range(K):
        PD._close(planes[k], h_planes[k], 1e-6)
    _moments_of(h_mean, h_var, h_planes)
    m_ref, v_ref = LC.ensemble_moments(h_planes)
    _same(h_mean, m_ref), _same(h_var, v_ref)


def test_one_draw_is_the_plane_and_has_no_variance(painter, plain):
    delta, kw, (_, _, planes) = plain
    mean, var, one = LC.paint_plane_ensemble(painter, delta, REL, TILE, Z, 1, batch_size=4, on_device=True,
                                             return_planes=True, **kw)
    assert one.shape == (1, N_PLANE, N_PLANE)
    _same(one[0], planes[0]), _same(mean, one[0])
    ok = np.isfinite(mean)
    assert (var[ok] == 0).all() and not np.signbit(var[ok]).any() and np.isnan(var[~ok]).all()


def test_plane_ensemble_with_zoom_and_with_regularise_std(painter):
    pytest.importorskip("scipy.ndimage")              # (the host path zooms with SciPy)
    q = painter
    delta = PD._smooth_delta(200, 42)
    assert LC.plane_geometry(200, REL, TILE)["cut"] == 85
    dev = LC.paint_plane_ensemble(q, delta, REL, TILE, Z, K, batch_size=FOUR, seed=7, on_device=True, return_planes=True)
    host = LC.paint_plane_ensemble(q, delta, REL, TILE, Z, K, batch_size=FOUR, seed=7, return_planes=True)
    for k in range(K):
        PD._close(dev[2][k], host[2][k], 1e-5)
    _moments_of(*dev)
    _moments_of(*host)
    delta = PD._delta(N_PLANE, 41)
    dev = LC.paint_plane_ensemble(q, delta, REL, TILE, Z, K, batch_size=ONE, seed=6, regularise_std=3, on_device=True,
                                  return_planes=True)
    host = LC.paint_plane_ensemble(q, delta, REL, TILE, Z, K, batch_size=FOUR, seed=6, regularise_std=3,
                                   return_planes=True)
    for k in range(K):
        PD._close(dev[2][k], host[2][k], 1e-5)
    _moments_of(*dev)
    PD._same_plane(dev[2][0], LC.paint_plane(q, delta, REL, TILE, Z, batch_size=4, seed=6, regularise_std=3,
                                             on_device=True))
    free = LC.paint_plane_ensemble(q, delta, REL, TILE, Z, K, batch_size=ONE, seed=6, on_device=True, return_planes=True)
    ok = np.isfinite(free[2])
    assert not np.array_equal(free[2][ok], dev[2][ok])               # the mask drops something


def test_out_receives_the_moments_and_a_device_delta_is_used_in_place(painter, plain):
    delta, kw, (mean, var, planes) = plain
    mean_t = torch.full((N_PLANE, N_PLANE), 3.0, dtype=torch.float64, device="cuda")
    var_t = torch.full_like(mean_t, 3.0)
    dt = torch.from_numpy(delta).cuda()
    r = LC.paint_plane_ensemble(painter, dt, REL, TILE, Z, K, batch_size=FOUR, on_device=True, out=(mean_t, var_t), **kw)
    assert len(r) == 2 and r[0] is mean_t and r[1] is var_t
    _same(mean_t.cpu().numpy(), mean), _same(var_t.cpu().numpy(), var)
    r = LC.paint_plane_ensemble(painter, dt, REL, TILE, Z, K, batch_size=FOUR, on_device=True, out=(mean_t, var_t),
                                return_planes=True, **kw)
    assert r[0] is mean_t and r[2].is_cuda and tuple(r[2].shape) == (K, N_PLANE, N_PLANE)
    _same(r[2].cpu().numpy(), planes)
    assert torch.equal(dt.cpu(), torch.from_numpy(delta))
    for bad in (mean_t, (mean_t, mean_t), (mean_t, var_t[:10]), (mean_t, var_t.float()), (mean_t.cpu(), var_t.cpu())):
        with pytest.raises(ValueError, match="out"):
            LC.paint_plane_ensemble(painter, dt, REL, TILE, Z, K, batch_size=FOUR, on_device=True, out=bad, **kw)
    with pytest.raises(ValueError, match="on_device"):
        LC.paint_plane_ensemble(painter, delta, REL, TILE, Z, K, batch_size=FOUR, out=(mean_t, var_t), **kw)
    painter.release_paint_buffers()
    assert "_plane_device_buffers" not in painter.__dict__


def test_two_field_painter(tmp_path):
    q = _settle(MFP._build("single scale", tmp_path)[0])
    F = len(MF.LABELS)
    delta = PD._delta(N_PLANE, 41)
    kw = dict(seed=5, first_tile_id=3)
    mean, var, planes = LC.paint_plane_ensemble(q, delta, REL, TILE, Z, K, batch_size=ONE, on_device=True,
                                                return_planes=True, **kw)
    assert mean.shape == var.shape == (F, N_PLANE, N_PLANE) and planes.shape == (K, F, N_PLANE, N_PLANE)
    _moments_of(mean, var, planes)
    single = LC.paint_plane(q, delta, REL, TILE, Z, batch_size=4, on_device=True, **kw)
    host = LC.paint_plane_ensemble(q, delta, REL, TILE, Z, K, batch_size=FOUR, return_planes=True, **kw)
    assert host[2].shape == planes.shape and host[0].shape == mean.shape
    for j in range(F):
        PD._same_plane(planes[0, j], single[j])
        for k in range(K):
            PD._close(planes[k, j], host[2][k, j], 1e-6)
    assert not np.array_equal(planes[0, 0], planes[0, 1], equal_nan=True)
    wide = LC.paint_plane_ensemble(q, delta, REL, TILE, Z, K, batch_size=FOUR, on_device=True, return_planes=True, **kw)
    for a, b in zip(wide, (mean, var, planes)):
        _same(a, b)
    # the light cone projects the named field's K planes
    y = LC.paint_light_cone_ensemble(q, [delta], [Z], [float(N_PLANE)], float(TILE), TILE, 48, [2.0], K, batch_size=FOUR,
                                     seed=5, on_device=True, field=MF.LABELS[1], return_maps=True)
    one = LC.paint_light_cone(q, [delta], [Z], [float(N_PLANE)], float(TILE), TILE, 48, [2.0], batch_size=4, seed=5,
                              on_device=True, field=MF.LABELS[1])
    _same(y[2][0], one)
    _moments_of(*y)
    with pytest.raises(ValueError, match="field"):
        LC.paint_light_cone_ensemble(q, [delta], [Z], [float(N_PLANE)], float(TILE), TILE, 48, [2.0], K, batch_size=FOUR)


def test_small_plane_ensemble(painter):
    q = painter
    host_mass = SP._smooth(256, 256, 43)
    dev_mass = torch.from_numpy(host_mass).cuda()
    geo = LC.small_plane_geometry(256, SP.SHIFT, SP.DELTA, SP.TILE_SIZE, SP.MASS_SIZE, SP.TILE)
    m = geo["crop"]
    assert (geo["cut"], m) == (128, 32) and SP.TILE == TILE
    kw = dict(seed=5, tile_id=9)
    mean, var, planes = LC.paint_small_plane_ensemble(q, dev_mass, *SP.SMALL, K, on_device=True, return_planes=True, **kw)
    assert planes.shape == (K, m, m) and planes.dtype == np.float64 and np.isfinite(planes).all()
    _same(planes[0], LC.paint_small_plane(q, dev_mass, *SP.SMALL, on_device=True, **kw))
    _moments_of(mean, var, planes)
    assert (var > 0).any() and np.abs(planes[1] - planes[0]).max() > LOOSEST * np.abs(planes[0]).max()
    # a host mass plane (the window is uploaded), the minimum subtracted, out=
    again = LC.paint_small_plane_ensemble(q, host_mass, *SP.SMALL, K, on_device=True, return_planes=True, **kw)
    for a, b in zip(again, (mean, var, planes)):
        _same(a, b)
    sub = LC.paint_small_plane_ensemble(q, dev_mass, *SP.SMALL, K, on_device=True, return_planes=True,
                                        subtract_minimum=True, **kw)
    _same(sub[2][0], LC.paint_small_plane(q, dev_mass, *SP.SMALL, on_device=True, subtract_minimum=True, **kw))
    _moments_of(*sub)
    out = tuple(torch.full((m, m), 3.0, dtype=torch.float64, device="cuda") for _ in range(2))
    r = LC.paint_small_plane_ensemble(q, dev_mass, *SP.SMALL, K, on_device=True, out=out, **kw)
    assert r[0] is out[0] and r[1] is out[1]
    _same(out[0].cpu().numpy(), mean), _same(out[1].cpu().numpy(), var)
    # the host path: SciPy's tile is within one float32 rounding of the device's and what the network makes of that is
    # not pinned (tests/test_gpu_small_plane.py prints it too); its moments are those of its planes
    pytest.importorskip("scipy.ndimage")
    h = LC.paint_small_plane_ensemble(q, host_mass, *SP.SMALL, K, return_planes=True, **kw)
    assert h[2].shape == planes.shape and h[2].dtype == np.float64
    _moments_of(*h)
    print("small plane, device against host: max |difference| of a draw",
          np.abs(h[2] - planes).max() / np.abs(h[2]).max(), "of the planes' maximum")
    with pytest.raises(ValueError, match="on_device"):
        LC.paint_small_plane_ensemble(q, host_mass, *SP.SMALL, K, out=out, **kw)


RES = 48


def _cone():
    """One small plane and one tiled plane without resampling (tests/test_gpu_ymap.py's "small" and "plain")."""
    planes = [(SP._smooth(256, 256, 43), SP.SHIFT, SP.MASS_SIZE), PD._delta(N_PLANE, 41)]
    z, size = [SP.Z, Z], [SP.DELTA, float(N_PLANE)]
    scales = LC.y_map_scales([32, N_PLANE], RES, 10.0, np.array([200.0, 1500.0]), lambda c: 1 / (1 + c / 3300.0), 0.69)
    return planes, z, size, scales


@pytest.mark.parametrize("order", [3, 5])
def test_light_cone_ensemble(painter, order):
    pytest.importorskip("scipy.ndimage")                          # (the host path zooms with SciPy)
    q = painter
    planes, z, size, scales = _cone()
    kw = dict(tile_size=SP.TILE_SIZE, n_pixel_tile=TILE, resolution=RES, scales=scales, order=order, seed=5)
    # everything on the device: map 0 is paint_light_cone's map, the moments are those of the maps
    mean, var, maps = LC.paint_light_cone_ensemble(q, iter(planes), z, size, draws=K, batch_size=FOUR, on_device=True,
                                                   small_planes_on_device=True, return_maps=True, **kw)
    assert maps.shape == (K, RES, RES) and maps.dtype == np.float64 and np.isfinite(maps).all()
    one = LC.paint_light_cone(q, planes, z, size, batch_size=4, on_device=True, small_planes_on_device=True, **kw)
    _same(maps[0], one)
    _moments_of(mean, var, maps)
    assert (var > 0).any() and np.abs(maps[1] - maps[0]).max() > LOOSEST * np.abs(maps[0]).max()
    pair = LC.paint_light_cone_ensemble(q, planes, z, size, draws=K, batch_size=ONE, on_device=True,
                                        small_planes_on_device=True, **kw)
    assert len(pair) == 2
    _same(pair[0], mean), _same(pair[1], var)
    out = tuple(torch.full((RES, RES), 3.0, dtype=torch.float64, device="cuda") for _ in range(2))
    r = LC.paint_light_cone_ensemble(q, planes, z, size, draws=K, batch_size=FOUR, on_device=True,
                                     small_planes_on_device=True, out=out, return_maps=True, **kw)
    assert r[0] is out[0] and r[1] is out[1] and r[2].is_cuda
    _same(out[0].cpu().numpy(), mean), _same(out[1].cpu().numpy(), var), _same(r[2].cpu().numpy(), maps)
    # small planes painted as on the host path: no resampled tile differs between the paths, the planes are the
    # host path's bit for bit and each map is within the projection's 1e-12 of its largest pixel (tests/test_gpu_ymap.py)
    host = LC.paint_light_cone_ensemble(q, planes, z, size, draws=K, batch_size=FOUR, return_maps=True, **kw)
    dev = LC.paint_light_cone_ensemble(q, planes, z, size, draws=K, batch_size=FOUR, on_device=True, return_maps=True,
                                       **kw)
    _moments_of(*host)
    _moments_of(*dev)
    for k in range(K):
        err, top = np.abs(dev[2][k] - host[2][k]).max(), np.abs(host[2][k]).max()
        print(f"order {order}, map {k}: max |dev - host| = {err:.3e} of {top:.3e}")
        assert top > 0 and err <= 1e-12 * top
    _same(dev[2][0], LC.paint_light_cone(q, planes, z, size, batch_size=4, on_device=True, **kw))


def test_a_second_seed_changes_the_planes_and_captures_nothing(painter, plain):
    q = painter
    delta, kw, (mean, var, planes) = plain
    args = (q, delta, REL, TILE, Z, K)
    first = LC.paint_plane_ensemble(*args, batch_size=ONE, on_device=True, return_planes=True, **kw)
    n_graphs, n_plans = len(q.model._graphs), len(q.model._paint_plans)
    second = LC.paint_plane_ensemble(*args, batch_size=ONE, on_device=True, return_planes=True, seed=2 ** 63 + 5,
                                     first_tile_id=7)
    again = LC.paint_plane_ensemble(*args, batch_size=ONE, on_device=True, return_planes=True, **kw)
    other = LC.paint_plane_ensemble(*args, batch_size=ONE, on_device=True, return_planes=True, seed=5, first_tile_id=70)
    assert (len(q.model._graphs), len(q.model._paint_plans)) == (n_graphs, n_plans)
    ok = np.isfinite(planes[0])
    assert not np.array_equal(second[2][:, ok], first[2][:, ok]) and not np.array_equal(other[2][:, ok], first[2][:, ok])
    for a, b, c in zip(again, first, (mean, var, planes)):
        _same(a, b), _same(a, c)
    _moments_of(*second)
    # seed=None draws a fresh key from torch's global generator
    torch.manual_seed(123)
    a = LC.paint_plane_ensemble(*args, batch_size=ONE, on_device=True)
    b = LC.paint_plane_ensemble(*args, batch_size=ONE, on_device=True)
    torch.manual_seed(123)
    c = LC.paint_plane_ensemble(*args, batch_size=ONE, on_device=True)
    assert not np.array_equal(a[0][ok], b[0][ok])
    _same(a[0], c[0]), _same(a[1], c[1])
    assert len(q.model._graphs) == n_graphs


def test_refusals_raise_before_any_side_effect(painter):
    q = painter
    delta = PD._delta(N_PLANE, 44)
    planes, z, size, scales = _cone()
    cone = dict(tile_size=SP.TILE_SIZE, n_pixel_tile=TILE, resolution=RES, scales=scales)

    def surfaces(p, **kw):
        small = {k: v for k, v in kw.items() if k != "batch_size"}
        return [lambda: LC.paint_plane_ensemble(p, delta, REL, TILE, Z, **kw),
                lambda: LC.paint_small_plane_ensemble(p, planes[0][0], *SP.SMALL, **small),
                lambda: LC.paint_light_cone_ensemble(p, planes, z, size, **cone, **kw)]

    def doubled(x, field, z, stats):
        return 2.0 * x

    class HostOnly:
        def paint_batch(self, tiles, z, batch_size=64):
            return tiles
    n_graphs = len(q.model._graphs)
    state = torch.get_rng_state()
    good = q.transform
    try:
        q.transform = type(good)(T.chain_transformations([doubled] + list(good.func.steps)), good.stats)
        for on_device in (False, True):
            for call in surfaces(q, draws=K, batch_size=FOUR, on_device=on_device):
                with pytest.raises(NotImplementedError):
                    call()
    finally:
        q.transform = good
    for on_device in (False, True):
        for call in surfaces(HostOnly(), draws=K, batch_size=FOUR, on_device=on_device):
            with pytest.raises(NotImplementedError):
                call()
        for call in surfaces(q, draws=65, batch_size=FOUR, on_device=on_device) + \
                surfaces(q, draws=0, batch_size=FOUR, on_device=on_device) + \
                surfaces(q, draws=K, batch_size=64, on_device=on_device)[::2]:
            with pytest.raises(ValueError):
                call()
        for call in surfaces(q, draws=K, batch_size=FOUR, on_device=on_device, pixel_noise=True)[1:]:
            with pytest.raises(NotImplementedError, match="noise_org"):
                call()
    for order in (0, 1, 6):
        with pytest.raises(NotImplementedError, match="order"):
            LC.paint_light_cone_ensemble(q, planes, z, size, draws=K, batch_size=FOUR, on_device=True, order=order, **cone)
    t = torch.zeros((RES, RES), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="on_device"):
        LC.paint_light_cone_ensemble(q, planes, z, size, draws=K, batch_size=FOUR, out=(t, t.clone()), **cone)
    with pytest.raises(ValueError, match="on_device"):
        LC.paint_light_cone_ensemble(q, planes, z, size, draws=K, batch_size=FOUR, small_planes_on_device=True, **cone)
    with pytest.raises(ValueError, match="out"):
        LC.paint_light_cone_ensemble(q, planes, z, size, draws=K, batch_size=FOUR, on_device=True, out=t, **cone)
    assert torch.equal(torch.get_rng_state(), state)
    assert len(q.model._graphs) == n_graphs
