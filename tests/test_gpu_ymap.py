"""GPU: the Compton-y map on the device (csrc/ymap.hip, lightcone.project_planes / paint_light_cone(on_device=True)):
bp_plane_project against scipy.ndimage.zoom(order=3, mode="mirror") in float64, its guards, and the whole light cone
against the host path of the same painter and seed.

The limit of every projection comparison is |got - ref| <= 1e-12 max|ref| on every pixel: double rounding through two
prefilter passes and sixteen taps is about 1e-15, the 32-sample warm-up of the chunked prefilter adds <= 3e-16
(tests/test_ymap_host.py), and a float32 shortcut anywhere would be about 6e-8.  One more term belongs to the budget:
the sampling coordinate k (n - 1) / (res - 1) carries a rounding of up to an ulp of its size, about 1e-13 of a pixel at
n = 1000, which moves the spline by that much times its slope (with white-noise planes the slope is of the order of the
plane's maximum per pixel).  The kernel forms the coordinate as SciPy does (k times the rounded ratio), so that the two
sample at the same point; an implementation that divides last would show about 4e-14 at 1000 -> 333, still inside."""
import ctypes as C

import numpy as np
import pytest
import torch

import host_cases as HC
import ymap_ref as R
from baryon_painter_amd import _lib as L
from baryon_painter_amd import lightcone as LC
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils import synthetic as syn
from baryon_painter_amd.utils.datasets import BAHAMASDataset

import gpu_util as G

pytestmark = pytest.mark.gpu

LIMIT = 1e-12
MARGIN = 1024                                     # doubles of canary on either side of y and of the scratch
CANARY = -7.25


def _zoom(a, n_out):
    try:
        import scipy.ndimage as nd
    except ImportError:                           # the float64 restatement that tests/test_ymap_host.py pins to SciPy
        return R.zoom(a, n_out)
    return nd.zoom(a, n_out / a.shape[0], order=3, mode="mirror")


def _host_loop(planes, scales, res, y0=None):
    y = np.zeros((res, res)) if y0 is None else y0.copy()
    for d, s in zip(planes, scales):
        d = d.copy()
        d[np.isnan(d)] = 0
        d *= s
        y += _zoom(d, res)
    return y


class _Map:
    """A (res, res) map and a scratch inside larger allocations: NaN margins around y, canary margins around the
    scratch, the scratch itself NaN (whatever leaks from it into y shows)."""

    def __init__(self, res, ws_bytes, y0=None):
        self.res = res
        self.ybuf = torch.full((res * res + 2 * MARGIN,), float("nan"), dtype=torch.float64, device="cuda")
        self.y = self.ybuf[MARGIN:MARGIN + res * res].view(res, res)
        self.y.copy_(torch.zeros(res, res, dtype=torch.float64) if y0 is None else torch.from_numpy(y0))
        self.nws = max(ws_bytes // 8, 1)
        self.sbuf = torch.full((self.nws + 2 * MARGIN,), CANARY, dtype=torch.float64, device="cuda")
        self.scratch = self.sbuf[MARGIN:MARGIN + self.nws]
        self.scratch.fill_(float("nan"))

    def project(self, plane_d, scale, scratch_bytes=None, rows=None, cols=None, res=None):
        n = plane_d.shape[0]
        return L.load().bp_plane_project(
            L.ptr(plane_d), n if rows is None else rows, plane_d.shape[1] if cols is None else cols, float(scale),
            C.c_void_p(self.scratch.data_ptr()), self.nws * 8 if scratch_bytes is None else scratch_bytes,
            C.c_void_p(self.y.data_ptr()), self.res if res is None else res, G.stream())

    def result(self):
        torch.cuda.synchronize()
        yb, sb = self.ybuf.cpu().numpy(), self.sbuf.cpu().numpy()
        assert np.isnan(yb[:MARGIN]).all() and np.isnan(yb[-MARGIN:]).all(), "written outside y"
        assert (sb[:MARGIN] == CANARY).all() and (sb[-MARGIN:] == CANARY).all(), "written outside the scratch"
        return yb[MARGIN:-MARGIN].reshape(self.res, self.res).copy()


def _device_project(planes, scales, res, y0=None):
    lib = L.load()
    ws = max(int(lib.bp_plane_project_workspace(p.shape[0], res)) for p in planes)
    m = _Map(res, ws, y0)
    for p, s in zip(planes, scales):
        d = torch.from_numpy(np.ascontiguousarray(p)).cuda()
        L.check(m.project(d, s), "plane project")
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), p, equal_nan=True), "the plane was modified"
    return m.result()


def _plane(n, seed, sigma=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.exp(sigma * rng.standard_normal((n, n)))


def _within(got, ref):
    assert np.isfinite(got).all()
    err, top = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"max |got - ref| = {err:.3e} = {err / top:.3e} of max |ref|")
    assert err <= LIMIT * top, (err, top)


# down-sampling, up-sampling, unit zoom, lines shorter than the warm-up (20) and just above it (33), and planes of
# the chunk length (224) - 1, + 0, + 1
@pytest.mark.parametrize("n,res", [(300, 257), (1000, 333), (257, 300), (100, 1000), (256, 256), (20, 64), (33, 64),
                                   (223, 150), (224, 150), (225, 300)])
def test_project_is_scipy_mirror_zoom(n, res):
    p = _plane(n, 1000 + n)
    s = 0.37
    _within(_device_project([p], [s], res), _host_loop([p], [s], res))


@pytest.mark.parametrize("n,res", [(300, 257), (257, 300)])
def test_project_wide_dynamic_range(n, res):
    p = _plane(n, 7, sigma=3.0)                                   # exp(3 N(0, 1)): seven decades
    assert p.max() / p.min() > 1e7
    _within(_device_project([p], [1.0], res), _host_loop([p], [1.0], res))


def test_project_zeroes_nans_and_leaves_the_plane():
    p = _plane(300, 8)
    p[:7] = np.nan                                                # the rim no tile reaches ...
    p[:, -5:] = np.nan
    p[-1] = np.nan
    p[120:160, 40:90] = np.nan                                    # ... and a block inside
    got = _device_project([p], [2.5], 257)                        # (asserts that P is unchanged, NaNs included)
    _within(got, _host_loop([p], [2.5], 257))


def test_accumulation_in_order_and_bitwise_repeatable():
    rng = np.random.Generator(np.random.PCG64(9))
    res = 200
    y0 = rng.standard_normal((res, res))
    planes = [_plane(100, 10), _plane(300, 11), _plane(257, 12)]
    planes[1][:4] = np.nan
    scales = [0.5, 3.0, 1.0e-2]
    ref = _host_loop(planes, scales, res, y0)
    got = _device_project(planes, scales, res, y0)
    _within(got, ref)
    assert np.array_equal(got, _device_project(planes, scales, res, y0))


def test_guards_write_nothing():
    lib = L.load()
    rng = np.random.Generator(np.random.PCG64(13))
    res = 64
    y0 = rng.standard_normal((res, res))
    p = torch.from_numpy(_plane(100, 14)).cuda()
    ws = int(lib.bp_plane_project_workspace(100, res))
    assert ws > 0 and lib.bp_plane_project_workspace(1, res) == 0 and lib.bp_plane_project_workspace(100, 1) == 0
    m = _Map(res, ws, y0)
    assert m.project(p, 1.0, scratch_bytes=ws - 8) == L.BP_EWORKSPACE
    assert m.project(p, 1.0, scratch_bytes=0) == L.BP_EWORKSPACE
    assert m.project(p, 1.0, rows=100, cols=99) == L.BP_EINVAL   # not square
    assert m.project(p, 1.0, rows=50, cols=200) == L.BP_EINVAL
    assert m.project(p, 1.0, rows=1, cols=1) == L.BP_EINVAL      # n < 2
    assert m.project(p, 1.0, res=1) == L.BP_EINVAL               # res < 2
    assert np.array_equal(m.result(), y0)
    assert np.isnan(m.scratch.cpu().numpy()).all()               # (not even the scratch)


def test_project_planes_on_device():
    LC.release_projection_buffers()
    planes = [_plane(100, 15), _plane(257, 16), _plane(20, 17)]
    planes[0][:3, :] = np.nan
    scales = [1.5, 0.25, 4.0]
    res = 128
    ref = _host_loop(planes, scales, res)
    got = LC.project_planes(planes, scales, res, on_device=True)                  # NumPy in, NumPy out
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    _within(got, ref)
    tens = [torch.from_numpy(p).cuda() for p in planes]                           # CUDA in
    got_t = LC.project_planes(tens, scales, res, on_device=True)
    assert np.array_equal(got_t, got)
    assert all(np.array_equal(t.cpu().numpy(), p, equal_nan=True) for t, p in zip(tens, planes))
    rng = np.random.Generator(np.random.PCG64(18))
    y0 = rng.standard_normal((res, res))
    out = torch.from_numpy(y0).cuda()                                             # out= is accumulated into
    r = LC.project_planes([tens[0], planes[1], tens[2]], scales, res, on_device=True, out=out)
    assert r is out
    _within(out.cpu().numpy(), _host_loop(planes, scales, res, y0))
    before = out.clone()
    with pytest.raises(NotImplementedError):
        LC.project_planes(tens, scales, res, order=1, on_device=True, out=out)
    assert torch.equal(out, before)
    with pytest.raises(ValueError):
        LC.project_planes(tens, scales, res, on_device=True, out=torch.zeros(res, res, device="cuda"))   # float32
    assert LC._projection_buffers
    LC.release_projection_buffers()
    assert not LC._projection_buffers


@pytest.fixture(scope="module")
def painter(tmp_path_factory):
    """A 64x64 painter loaded from checkpoint files (as in test_gpu_paint_plane_device.py)."""
    from baryon_painter_amd.painter import CVAEPainter
    size = 64
    arch = A.fiducial_architecture(size)
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    tr = T.chain_transformations([fwd, T.atleast_3d, T.as_float32])
    itr = T.chain_transformations([T.squeeze, inv])
    ds = BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=1,
                        n_stack=3, transform=tr, inverse_transform=itr, scale_to_SLICS=True)
    torch.manual_seed(3)
    p = CVAEPainter(training_data_set=ds, test_data_set=ds, architecture=arch, compute_device="cuda:0")
    x, y, aux = syn.synthetic_batch(4, size, size, seed=77)
    with torch.no_grad():
        p.model(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
    d = tmp_path_factory.mktemp("ckpt")
    files = (str(d / "state"), str(d / "meta"))
    p.save_state_to_file(files)
    return CVAEPainter(filename=files, compute_device="cuda:0")


def _delta(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (np.exp(rng.standard_normal((n, n)) * 0.5) * 0.05).astype(np.float32)


def _smooth(n, seed):
    """A smooth positive periodic plane (the spline resampling of white noise overshoots below zero, where the
    shift-log transform is NaN on both paths)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    k = np.fft.fftfreq(n) * n
    f = np.fft.ifft2(np.fft.fft2(rng.standard_normal((n, n))) * (np.hypot(k[:, None], k[None, :]) < n / 10)).real
    return (np.exp(f / f.std() * 0.5) * 0.05).astype(np.float32)


# tiles of 64 pixels and of size 64; a 150-pixel plane of size 150 without resampling, a 200-pixel plane of the same
# size (85 -> 64 cuts), and a plane of size 32 < 64 from a 256-pixel mass plane of size 128 (128 -> 64, centre 32)
TILE, RES = 64, 120
KW = dict(tile_size=64.0, n_pixel_tile=TILE, resolution=RES, batch_size=8)


def _cone(which):
    entries = {"plain": (_delta(150, 41), 0.42, 150.0), "zoomed": (_smooth(200, 42), 0.3, 150.0),
               "small": ((_smooth(256, 43), (0.9, 0.85), 128.0), 0.05, 32.0)}
    planes, z, size = zip(*(entries[w] for w in which))
    n_pix = [150 if w != "small" else 32 for w in which]
    chi = np.array([1500.0 if w == "plain" else 1100.0 if w == "zoomed" else 200.0 for w in which])
    order = np.argsort(chi)
    scales = np.empty(len(which))
    scales[order] = LC.y_map_scales([n_pix[i] for i in order], RES, 10.0, chi[order], lambda c: 1 / (1 + c / 3300.0),
                                    0.69)
    return list(planes), list(z), list(size), scales


def _finite_equal(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_light_cone_without_resampled_planes(painter):
    pytest.importorskip("scipy.ndimage")                          # (the host path zooms with SciPy)
    planes, z, size, scales = _cone(["small", "plain"])
    host, hp = LC.paint_light_cone(painter, planes, z, size, scales=scales, seed=5, return_planes=True, **KW)
    dev, dp = LC.paint_light_cone(painter, iter(planes), z, size, scales=scales, seed=5, on_device=True,
                                  return_planes=True, **KW)
    assert [p.shape for p in dp] == [(32, 32), (150, 150)] and dev.shape == (RES, RES) and dev.dtype == np.float64
    for a, b in zip(dp, hp):                                      # the same bits
        assert _finite_equal(a, b)
    assert np.isfinite(dp[1]).mean() > 0.9 and np.abs(host).max() > 0
    _within(dev, host)


def test_light_cone_out_is_accumulated(painter):
    """Device path only (tiled planes: no SciPy anywhere): out= receives the map, the same seed the same bits."""
    planes, z, size, scales = [_delta(150, 46), _delta(150, 47)], [0.42, 0.3], [150.0, 150.0], [0.5, 2.0]
    dev = LC.paint_light_cone(painter, planes, z, size, scales=scales, seed=5, on_device=True, **KW)
    assert dev.shape == (RES, RES) and dev.dtype == np.float64 and np.isfinite(dev).all() and np.abs(dev).max() > 0
    out = torch.zeros((RES, RES), dtype=torch.float64, device="cuda")
    r = LC.paint_light_cone(painter, iter(planes), z, size, scales=scales, seed=5, on_device=True, out=out, **KW)
    assert r is out and np.array_equal(out.cpu().numpy(), dev)
    LC.paint_light_cone(painter, planes, z, size, scales=scales, seed=5, on_device=True, out=out, **KW)
    _within(out.cpu().numpy(), dev + dev)                         # ((a + b) + a) + b: rounding only
    with pytest.raises(ValueError):
        LC.paint_light_cone(painter, planes, z, size, scales=scales, seed=5, out=out, **KW)     # out= without on_device


def test_light_cone_with_a_resampled_plane(painter):
    """Three planes: small, tiled with 85 -> 64 cuts, tiled without resampling.  The resampled tiles of the two paths
    are within 1 ulp (float32) of each other going INTO the network, so the painted planes differ;
    the projection is linear, so the maps differ by at most the projection of that difference, which is bounded by
    scale * max |plane_dev - plane_host| * (sum of absolute weights of prefilter and sampling, both axes), plus the
    projection's own 1e-12."""
    pytest.importorskip("scipy.ndimage")
    planes, z, size, scales = _cone(["small", "zoomed", "plain"])
    host, hp = LC.paint_light_cone(painter, planes, z, size, scales=scales, seed=6, return_planes=True, **KW)
    dev, dp = LC.paint_light_cone(painter, planes, z, size, scales=scales, seed=6, on_device=True,
                                  return_planes=True, **KW)
    bound = LIMIT * np.abs(host).max()
    for i, (a, b) in enumerate(zip(dp, hp)):
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
        ok = ~np.isnan(b)
        diff = np.abs(a[ok] - b[ok]).max()
        n = a.shape[0]
        ti, w = R.axis_weights(n, RES)                            # one axis as a matrix: sampling times prefilter
        S = np.zeros((RES, n))
        for q in range(4):
            np.add.at(S, (np.arange(RES), ti[:, q]), w[:, q])
        gain = np.abs(S @ R.prefilter_lines(np.eye(n))).sum(axis=1).max()
        assert 1.0 - 1e-9 <= gain <= 3.0 ** 0.5 + 1e-9                   # (the prefilter alone: (1 + |z|) / (1 - |z|))
        print(f"plane {i}: max |dev - host| = {diff:.3e} of {np.abs(b[ok]).max():.3e}, weights {gain ** 2:.4f}")
        bound += scales[i] * diff * gain ** 2
    assert _finite_equal(dp[0], hp[0]) and _finite_equal(dp[2], hp[2])
    err = np.abs(dev - host).max()
    print(f"max |y_dev - y_host| = {err:.3e}, bound {bound:.3e}, max |y| {np.abs(host).max():.3e}")
    assert err <= bound


def test_light_cone_seeds(painter):
    d = _delta(150, 44)
    planes, z, size, scales = [d, d], [0.42, 0.42], [150.0, 150.0], [1.0, 1.0]
    kw = dict(scales=scales, on_device=True, return_planes=True, **KW)
    y1, p1 = LC.paint_light_cone(painter, planes, z, size, seed=11, **kw)
    y2, p2 = LC.paint_light_cone(painter, planes, z, size, seed=11, **kw)
    assert np.array_equal(y1, y2) and all(_finite_equal(a, b) for a, b in zip(p1, p2))
    # the same delta at the same redshift under the same key: only the tile ids tell the two planes apart
    ok = ~np.isnan(p1[0])
    assert not np.array_equal(p1[0][ok], p1[1][ok])
    n_tiles = LC.plane_geometry(150, 64 / 150, TILE)["n_side"] ** 2
    alone = LC.paint_plane(painter, d, 64 / 150, TILE, 0.42, batch_size=8, seed=11, first_tile_id=n_tiles,
                           on_device=True)
    assert _finite_equal(alone, p1[1])
    torch.manual_seed(123)
    ya = LC.paint_light_cone(painter, planes, z, size, scales=scales, on_device=True, **KW)
    yb = LC.paint_light_cone(painter, planes, z, size, scales=scales, on_device=True, **KW)
    assert not np.array_equal(ya, yb)
    torch.manual_seed(123)
    assert np.array_equal(LC.paint_light_cone(painter, planes, z, size, scales=scales, on_device=True, **KW), ya)


def test_ineligible_painter_raises_before_a_seed_is_drawn(painter):
    q = painter
    planes, z, size, scales = [_delta(150, 45)], [0.42], [150.0], [1.0]

    def doubled(x, field, z, stats):
        return 2.0 * x
    good = q.transform
    try:
        q.transform = type(good)(T.chain_transformations([doubled] + list(good.func.steps)), good.stats)
        n_graphs = len(q.model._graphs)
        state = torch.get_rng_state()
        with pytest.raises(NotImplementedError):
            LC.paint_light_cone(q, planes, z, size, scales=scales, on_device=True, **KW)
        assert torch.equal(torch.get_rng_state(), state)
        assert len(q.model._graphs) == n_graphs
    finally:
        q.transform = good

    class HostOnly:
        def paint_batch(self, tiles, z, batch_size=64):
            return tiles
    state = torch.get_rng_state()
    with pytest.raises(NotImplementedError):
        LC.paint_light_cone(HostOnly(), planes, z, size, scales=scales, on_device=True, **KW)
    with pytest.raises(NotImplementedError):
        LC.paint_light_cone(q, planes, z, size, scales=scales, on_device=True, order=1, **KW)
    assert torch.equal(torch.get_rng_state(), state)
