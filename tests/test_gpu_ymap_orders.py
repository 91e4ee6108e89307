"""GPU: the device y-map projection at spline orders 2, 4 and 5 (csrc/ymap.hip, bp_plane_project_order;
lightcone.project_planes / create_y_map / paint_light_cone(order=..., on_device=True)) against
scipy.ndimage.zoom(order, mode="mirror") in float64, order 3 through the new entry point against bp_plane_project
bit for bit, the guards, and a quintic light cone against the host path of the same painter and seed.

The limit is test_gpu_ymap.py's, |got - ref| <= 1e-12 max|ref| on every pixel, with the same budget: rounding through
the prefilter (four recursions per axis at orders 4 and 5) and up to 36 taps is about 1e-14 -- SciPy's own arithmetic is
1.3e-14 (order 4) and 7.4e-15 (order 5) from a plain sequential recursion (tests/test_ymap_orders_host.py) -- the
warm-ups of the chunked prefilter leave <= 1e-18 of their start, and the rounding of the sampling coordinate, formed as
SciPy forms it, is about 4e-14 at 1000 -> 333 if it were not.  Canary and NaN margins as in test_gpu_ymap.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_ymap as Y3
import ymap_ref_orders as R
from baryon_painter_amd import _lib as L
from baryon_painter_amd import lightcone as LC

import gpu_util as G

pytestmark = pytest.mark.gpu

LIMIT = Y3.LIMIT
NEW = (2, 4, 5)
painter = Y3.painter                              # the 64x64 checkpoint painter (module-scoped fixture)


def _zoom(a, n_out, order):
    try:
        import scipy.ndimage as nd
    except ImportError:                           # the restatement that tests/test_ymap_orders_host.py pins to SciPy
        return R.zoom(a, n_out, order)
    return nd.zoom(a, n_out / a.shape[0], order=order, mode="mirror")


def _host_loop(planes, scales, res, order, y0=None):
    y = np.zeros((res, res)) if y0 is None else y0.copy()
    for d, s in zip(planes, scales):
        d = d.copy()
        d[np.isnan(d)] = 0
        d *= s
        y += _zoom(d, res, order)
    return y


class _Map(Y3._Map):
    def project(self, plane_d, scale, order, scratch_bytes=None):
        n = plane_d.shape[0]
        return L.load().bp_plane_project_order(
            L.ptr(plane_d), n, plane_d.shape[1], float(scale), order, C.c_void_p(self.scratch.data_ptr()),
            self.nws * 8 if scratch_bytes is None else scratch_bytes, C.c_void_p(self.y.data_ptr()), self.res,
            G.stream())


def _device_project(planes, scales, res, order, y0=None):
    lib = L.load()
    ws = max(int(lib.bp_plane_project_order_workspace(p.shape[0], res, order)) for p in planes)
    assert ws == max(2 * 8 * p.shape[0] ** 2 for p in planes)
    m = _Map(res, ws, y0)
    for p, s in zip(planes, scales):
        d = torch.from_numpy(np.ascontiguousarray(p)).cuda()
        L.check(m.project(d, s, order), "plane project")
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), p, equal_nan=True), "the plane was modified"
    return m.result()


def _within(got, ref, what=""):
    assert np.isfinite(got).all()
    err, top = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"{what}max |got - ref| = {err:.3e} = {err / top:.3e} of max |ref|")
    assert err <= LIMIT * top, (err, top)


# down-sampling, up-sampling, unit zoom; one below, at and one above every length constant of the kernels: the
# short-line threshold (32), halo + 1 (33 with one pole, 97 with two) and the chunk (224), where several sub-chunks of
# the halo wrap round a line shorter than it; a line shorter than the threshold
SHAPES = [(300, 257), (1000, 333), (257, 300), (100, 1000), (256, 256), (31, 64), (32, 64), (33, 50), (34, 64),
          (96, 64), (97, 128), (98, 64), (223, 150), (224, 150), (225, 300), (20, 64)]


@pytest.mark.parametrize("order", NEW)
@pytest.mark.parametrize("n,res", SHAPES)
def test_project_is_scipy_mirror_zoom(n, res, order):
    p = Y3._plane(n, 1000 + n)
    s = 0.37
    _within(_device_project([p], [s], res, order), _host_loop([p], [s], res, order), f"order {order} {n} -> {res}: ")


@pytest.mark.parametrize("n,res", [(2, 7), (3, 9), (2, 2)])
def test_more_taps_than_samples(n, res):
    p = Y3._plane(n, 50 + n)
    _within(_device_project([p], [1.5], res, 5), _host_loop([p], [1.5], res, 5), f"order 5 {n} -> {res}: ")


@pytest.mark.parametrize("order", NEW)
@pytest.mark.parametrize("n,res", [(300, 257), (257, 300)])
def test_project_wide_dynamic_range(n, res, order):
    p = Y3._plane(n, 7, sigma=3.0)                                # exp(3 N(0, 1)): seven decades
    assert p.max() / p.min() > 1e7
    _within(_device_project([p], [1.0], res, order), _host_loop([p], [1.0], res, order), f"order {order} {n} -> {res}: ")


@pytest.mark.parametrize("order", NEW)
def test_project_zeroes_nans_and_leaves_the_plane(order):
    p = Y3._plane(300, 8)
    p[:7] = np.nan                                                # the rim no tile reaches ...
    p[:, -5:] = np.nan
    p[-1] = np.nan
    p[120:160, 40:90] = np.nan                                    # ... and a block inside
    got = _device_project([p], [2.5], 257, order)                 # (asserts that P is unchanged, NaNs included)
    _within(got, _host_loop([p], [2.5], 257, order), f"order {order}: ")


@pytest.mark.parametrize("n,res", [(300, 257), (20, 64)])
def test_order_3_is_bitwise_bp_plane_project(n, res):
    p = Y3._plane(n, 21)
    p[:2] = np.nan
    new = _device_project([p], [0.37], res, 3)
    old = Y3._device_project([p], [0.37], res)
    assert np.array_equal(new, old)
    lib = L.load()
    assert lib.bp_plane_project_order_workspace(n, res, 3) == lib.bp_plane_project_workspace(n, res)


def test_accumulation_in_order_and_bitwise_repeatable():
    rng = np.random.Generator(np.random.PCG64(9))
    res = 200
    y0 = rng.standard_normal((res, res))
    planes = [Y3._plane(100, 10), Y3._plane(300, 11), Y3._plane(257, 12)]
    planes[1][:4] = np.nan
    scales = [0.5, 3.0, 1.0e-2]
    got = _device_project(planes, scales, res, 5, y0)
    _within(got, _host_loop(planes, scales, res, 5, y0), "order 5, three planes: ")
    assert np.array_equal(got, _device_project(planes, scales, res, 5, y0))
    for order in (2, 4):
        one = _device_project(planes[:1], scales[:1], res, order, y0)
        assert np.array_equal(one, _device_project(planes[:1], scales[:1], res, order, y0))


def test_guards_write_nothing():
    lib = L.load()
    rng = np.random.Generator(np.random.PCG64(13))
    res = 64
    y0 = rng.standard_normal((res, res))
    p = torch.from_numpy(Y3._plane(100, 14)).cuda()
    ws = int(lib.bp_plane_project_order_workspace(100, res, 5))
    assert ws == 2 * 8 * 100 * 100
    for order in (0, 1, 6, -1):
        assert lib.bp_plane_project_order_workspace(100, res, order) == 0
    assert lib.bp_plane_project_order_workspace(1, res, 5) == 0 and lib.bp_plane_project_order_workspace(100, 1, 5) == 0
    m = _Map(res, ws, y0)
    for order in (0, 1, 6, -1):
        assert m.project(p, 1.0, order) == L.BP_EUNSUPPORTED
    for order in (2, 3, 4, 5):
        assert m.project(p, 1.0, order, scratch_bytes=ws - 8) == L.BP_EWORKSPACE
        assert m.project(p, 1.0, order, scratch_bytes=0) == L.BP_EWORKSPACE
    assert np.array_equal(m.result(), y0)
    assert np.isnan(m.scratch.cpu().numpy()).all()               # (not even the scratch)


def test_project_planes_on_device_reuses_the_scratch():
    LC.release_projection_buffers()
    planes = [Y3._plane(100, 15), Y3._plane(257, 16), Y3._plane(20, 17)]
    planes[0][:3, :] = np.nan
    scales = [1.5, 0.25, 4.0]
    res = 128
    small = LC.project_planes(planes[:1], scales[:1], res, order=3, on_device=True)      # order 3 first: a small scratch
    _within(small, _host_loop(planes[:1], scales[:1], res, 3), "order 3 first: ")
    ref = _host_loop(planes, scales, res, 5)
    got = LC.project_planes(planes, scales, res, order=5, on_device=True)                 # NumPy in, NumPy out
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    _within(got, ref, "order 5, NumPy planes: ")
    tens = [torch.from_numpy(p).cuda() for p in planes]                                   # CUDA in
    assert np.array_equal(LC.project_planes(tens, scales, res, order=5, on_device=True), got)
    assert all(np.array_equal(t.cpu().numpy(), p, equal_nan=True) for t, p in zip(tens, planes))
    rng = np.random.Generator(np.random.PCG64(18))
    y0 = rng.standard_normal((res, res))
    out = torch.from_numpy(y0).cuda()                                                     # out= is accumulated into
    r = LC.project_planes([tens[0], planes[1], tens[2]], scales, res, order=5, on_device=True, out=out)
    assert r is out
    _within(out.cpu().numpy(), _host_loop(planes, scales, res, 5, y0), "order 5, out=: ")
    for order in (2, 4):
        _within(LC.project_planes(tens, scales, res, order=order, on_device=True), _host_loop(planes, scales, res, order),
                f"order {order}: ")
    before = out.clone()
    for order in (0, 1, 6):
        with pytest.raises(NotImplementedError):
            LC.project_planes(tens, scales, res, order=order, on_device=True, out=out)
    assert torch.equal(out, before)
    LC.release_projection_buffers()


def test_create_y_map_on_device_at_order_5():
    planes = [Y3._plane(64, 31), Y3._plane(150, 32)]
    chi = np.array([300.0, 1200.0])
    args = ([0.1, 0.4], 96, 10.0, chi, lambda c: 1 / (1 + c / 3300.0), 0.69)
    host = LC.create_y_map(planes, *args, order=5)
    _within(LC.create_y_map(planes, *args, order=5, on_device=True), host, "create_y_map order 5: ")
    LC.release_projection_buffers()


def test_light_cone_at_order_5(painter):
    """scripts/create_lightcone.py's configuration: quintic projection.  Three planes -- small, tiled with 85 -> 64 cuts,
    tiled without resampling -- on the device against the host path of the same painter and seed.  The painted planes
    agree as at order 3 (test_gpu_ymap.py: the unresampled ones bit for bit; the resampled tiles are within 1 ulp
    (float32) of the host's going into the network, and whatever difference that leaves in the plane reaches the map
    through the linear projection, bounded by scale * max |plane_dev - plane_host| * (sum of absolute weights of
    prefilter and sampling, both axes)); the maps agree within 1e-12 of the largest pixel beyond that."""
    pytest.importorskip("scipy.ndimage")
    planes, z, size, scales = Y3._cone(["small", "zoomed", "plain"])
    host, hp = LC.paint_light_cone(painter, planes, z, size, scales=scales, seed=6, order=5, return_planes=True, **Y3.KW)
    dev, dp = LC.paint_light_cone(painter, planes, z, size, scales=scales, seed=6, order=5, on_device=True,
                                  return_planes=True, **Y3.KW)
    assert dev.shape == (Y3.RES, Y3.RES) and dev.dtype == np.float64 and np.abs(host).max() > 0
    bound = LIMIT * np.abs(host).max()
    for i, (a, b) in enumerate(zip(dp, hp)):
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
        ok = ~np.isnan(b)
        diff = np.abs(a[ok] - b[ok]).max()
        n = a.shape[0]
        ti, w = R.axis_weights(n, Y3.RES, 5)                      # one axis as a matrix: sampling times prefilter
        S = np.zeros((Y3.RES, n))
        for q in range(6):
            np.add.at(S, (np.arange(Y3.RES), ti[:, q]), w[:, q])
        gain = np.abs(S @ R.prefilter_lines(np.eye(n), 5)).sum(axis=1).max()
        print(f"plane {i}: max |dev - host| = {diff:.3e} of {np.abs(b[ok]).max():.3e}, weights {gain ** 2:.4f}")
        bound += scales[i] * diff * gain ** 2
    assert Y3._finite_equal(dp[0], hp[0]) and Y3._finite_equal(dp[2], hp[2])
    err = np.abs(dev - host).max()
    print(f"max |y_dev - y_host| = {err:.3e}, bound {bound:.3e}, max |y| {np.abs(host).max():.3e}")
    assert err <= bound
