"""GPU: the low-redshift plane of a light cone on the device (csrc/window.hip, lightcone.paint_small_plane(on_device=True),
lightcone.paint_light_cone(small_planes_on_device=True)).

The kernels through the C ABI, every output and the scratch inside canary margins:
  * bp_window_zoom against SciPy's float64 ``zoom(order=3, mode="mirror")`` r of the same wrapped window (tests/ymap_ref.py
    where SciPy is missing): |out - r| <= ulp32(r) / 2 + 1e-12 max |r| on every pixel -- ONE rounding to float32 plus the
    projection's own limit of tests/test_gpu_ymap.py (double rounding through two prefilter passes and sixteen taps,
    the 32-sample warm-up, the coordinate's rounding).  The share of pixels bit-equal to float32(r) is printed;
  * bp_window_min and bp_tile_crop bit for bit against NumPy;
  * every refusal, with nothing written.
The painters end to end by a CHAIN OF BITS: paint_small_plane(on_device=True) equals bp_window_zoom's tile from the C
ABI, painted by ``paint_stream`` at batch 1 under the same seed and tile id, cropped on the host.  (A tolerance against
the all-host path would rest on how a network amplifies one float32 rounding of its input, which nothing here can
derive; that difference is printed.)  The light cone equals ``project_planes(on_device=True)`` of planes painted one by
one."""
import ctypes as C

import numpy as np
import pytest
import torch

import gpu_util as G
import host_cases as HC
import multi_field_cases as MF
import small_plane_ref as S
import ymap_ref as R
from baryon_painter_amd import _lib as L
from baryon_painter_amd import lightcone as LC
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils import datasets as D
from baryon_painter_amd.utils import synthetic as syn
from baryon_painter_amd.utils.datasets import BAHAMASDataset

pytestmark = pytest.mark.gpu

LIMIT = 1e-12                                     # of max |r|: the projection's limit (tests/test_gpu_ymap.py)
MARGIN = 1024                                     # elements of canary on either side of every output and scratch
CANARY = -7.25
TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
CODE = {np.dtype(np.float32): L.F32, np.dtype(np.float64): L.F64}


def _zoom(a, n_out):
    try:
        import scipy.ndimage as nd
    except ImportError:                           # the float64 restatement that tests/test_ymap_host.py pins to SciPy
        return R.zoom(a, n_out)
    return nd.zoom(a, n_out / a.shape[0], order=3, mode="mirror")


def _smooth(rows, cols, seed, dtype=np.float32):
    """A smooth positive periodic plane (``_smooth`` of tests/test_gpu_ymap.py, rows x cols): white noise resampled by a
    cubic goes negative, which the shift-log transform cannot take."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ky, kx = np.fft.fftfreq(rows), np.fft.fftfreq(cols)
    f = np.fft.ifft2(np.fft.fft2(rng.standard_normal((rows, cols))) * (np.hypot(ky[:, None], kx[None, :]) < 0.1)).real
    return (np.exp(f / f.std() * 0.5) * 0.05).astype(dtype)


class _Buf:
    """``count`` elements of ``dtype`` filled with ``fill`` inside a larger allocation with canary margins."""

    def __init__(self, count, dtype, fill=float("nan")):
        self.count = count
        self.buf = torch.full((count + 2 * MARGIN,), CANARY, dtype=dtype, device="cuda")
        self.t = self.buf[MARGIN:MARGIN + count]
        self.t.fill_(fill)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    @property
    def nbytes(self):
        return self.count * self.t.element_size()

    def get(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert (b[:MARGIN] == CANARY).all() and (b[-MARGIN:] == CANARY).all(), "written outside the buffer"
        return b[MARGIN:-MARGIN].copy()


def _window_min(plane_d, x0, y0, size, **kw):
    """bp_window_min -> (return code, the _Buf of the minimum); ``kw`` overrides arguments."""
    lib = L.load()
    dt = plane_d.dtype
    scratch = _Buf(int(lib.bp_window_min_workspace()) // 8, torch.float64)
    out = _Buf(1, dt)
    a = dict(plane=L.ptr(plane_d), dtype=L.F32 if dt == torch.float32 else L.F64, rows=plane_d.shape[0],
             cols=plane_d.shape[1], x0=x0, y0=y0, size=size, scratch=scratch.ptr, scratch_bytes=scratch.nbytes,
             out=out.ptr)
    a.update(kw)
    rc = lib.bp_window_min(a["plane"], a["dtype"], a["rows"], a["cols"], a["x0"], a["y0"], a["size"], a["scratch"],
                           a["scratch_bytes"], a["out"], G.stream())
    out.scratch = scratch
    return rc, out


def _window_zoom(plane_d, x0, y0, size, tile, minimum=None, **kw):
    """bp_window_zoom -> (return code, the _Buf of the tile, the _Buf of the scratch); ``kw`` overrides arguments."""
    lib = L.load()
    ws = int(lib.bp_window_zoom_workspace(size, tile))          # (0 for arguments that are refused)
    scratch = _Buf(max(ws // 8, 1), torch.float64)
    out = _Buf(tile * tile if ws else 64 * 64, torch.float32)
    a = dict(plane=L.ptr(plane_d), dtype=L.F32 if plane_d.dtype == torch.float32 else L.F64, rows=plane_d.shape[0],
             cols=plane_d.shape[1], x0=x0, y0=y0, size=size, minimum=minimum, tile=tile, scratch=scratch.ptr,
             scratch_bytes=scratch.nbytes, out=out.ptr)
    a.update(kw)
    rc = lib.bp_window_zoom(a["plane"], a["dtype"], a["rows"], a["cols"], a["x0"], a["y0"], a["size"], a["minimum"],
                            a["tile"], a["scratch"], a["scratch_bytes"], a["out"], G.stream())
    return rc, out, scratch


def _device_tile(plane_d, x0, y0, size, tile, subtract_minimum):
    """The raw tile of the device small plane through the C ABI: (tile, tile) float32 NumPy."""
    minimum = None
    if subtract_minimum:
        rc, mn = _window_min(plane_d, x0, y0, size)
        L.check(rc, "window min")
        minimum = mn.ptr
    rc, out, scratch = _window_zoom(plane_d, x0, y0, size, tile, minimum)
    L.check(rc, "window zoom")
    scratch.get()
    return out.get().reshape(tile, tile)


PLANES = {}
ORIGINS = [(0, 0), (-37, 250), (190, -5)]         # none; both axes wrap; past the rows' end and before the first column


def _planes(dtype):
    """The two mass planes of the zoom tests, (256, 256) and (200, 310), host and device (built once per dtype)."""
    key = np.dtype(dtype)
    if key not in PLANES:
        hosts = [_smooth(256, 256, 51, dtype), _smooth(200, 310, 52, dtype)]
        PLANES[key] = [(h, torch.from_numpy(h).cuda()) for h in hosts]
    return PLANES[key]


# ----------------------------------------------------------------------------------------------------- the kernels
# lines shorter than the warm-up (20) and just above it (33), up-sampling (40), unit zoom (64), the chunk length (224)
# - 1, + 0, + 1, more than one chunk (300); 128 -> 48: an output that is no power of two
@pytest.mark.parametrize("size,tile,dtype", [(20, 64, np.float32), (33, 64, np.float32), (40, 64, np.float32),
                                             (64, 64, np.float32), (128, 64, np.float32), (223, 64, np.float32),
                                             (224, 64, np.float32), (225, 64, np.float32), (300, 64, np.float32),
                                             (128, 48, np.float32), (33, 64, np.float64), (225, 64, np.float64)])
def test_window_zoom_is_scipy_mirror_zoom_rounded_once(size, tile, dtype):
    worst, equal, count = 0.0, 0, 0
    for host, dev in _planes(dtype):
        before = host.copy()
        for x0, y0 in ORIGINS:
            w = S.wrapped_window(host, x0, y0, size)
            assert w.dtype == dtype and w.shape == (size, size)
            for subtract_minimum in (False, True):
                if subtract_minimum:
                    w = w - w.min()                              # (in the plane's dtype)
                r = _zoom(w.astype(np.float64), tile)
                assert r.shape == (tile, tile)
                got = _device_tile(dev, x0, y0, size, tile, subtract_minimum)
                assert got.dtype == np.float32 and np.isfinite(got).all()
                err = np.abs(got.astype(np.float64) - r)
                bound = S.ulp32(r) / 2 + LIMIT * np.abs(r).max()
                worst = max(worst, (err / bound).max())
                equal += int((got == r.astype(np.float32)).sum())
                count += got.size
                assert (err <= bound).all(), (x0, y0, subtract_minimum, (err / bound).max())
                again = _device_tile(dev, x0, y0, size, tile, subtract_minimum)
                assert np.array_equal(got, again)                # two launches, the same bits
        assert np.array_equal(dev.cpu().numpy(), before)         # the plane is not modified
    print(f"{size} -> {tile} {np.dtype(dtype).name}: worst |out - r| = {worst:.4f} of its bound, "
          f"{equal / count:.5f} of the pixels bit-equal to float32(r)")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_window_zoom_of_a_window_with_non_finite_values_does_not_fault(dtype):
    host = _smooth(256, 256, 53, dtype)
    host[10, 20], host[200, 100], host[250, 250] = np.nan, np.inf, -np.inf
    dev = torch.from_numpy(host).cuda()
    for size in (20, 300):                                        # the thread-per-line and the chunked prefilter
        got = _device_tile(dev, -37, 250, size, 64, True)         # (the canaries are checked; the values are not)
        assert got.shape == (64, 64)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("size", [1, 63, 64, 65, 300])
def test_window_min_is_numpy_min(size, dtype):
    for host, dev in _planes(dtype):
        for x0, y0 in ORIGINS:
            rc, out = _window_min(dev, x0, y0, size)
            L.check(rc, "window min")
            got = out.get()
            out.scratch.get()
            ref = S.wrapped_window(host, x0, y0, size).min()
            assert got.dtype == dtype and got.tobytes() == np.asarray(ref, dtype).tobytes(), (x0, y0, got, ref)
    # a NaN anywhere in the window is the minimum, as np.min's; outside the window it is not seen
    host = _planes(dtype)[1][0].copy()
    host[(190 + size - 1) % 200, (-5 + size // 2) % 310] = np.nan
    dev = torch.from_numpy(host).cuda()
    rc, out = _window_min(dev, 190, -5, size)
    L.check(rc, "window min")
    assert np.isnan(out.get()[0]) and np.isnan(S.wrapped_window(host, 190, -5, size).min())
    if size < 150:
        rc, out = _window_min(dev, 190 + size, -5, size)
        L.check(rc, "window min")
        ref = S.wrapped_window(host, 190 + size, -5, size).min()
        assert np.isfinite(ref) and out.get()[0] == ref


@pytest.mark.parametrize("r0,c0,m", [(16, 16, 32), (0, 0, 64), (50, 60, 30)])       # the last one wraps
def test_tile_crop_is_get_tile(r0, c0, m):
    rng = np.random.Generator(np.random.PCG64(54))
    img = rng.standard_normal((64, 64)).astype(np.float32)
    dev = torch.from_numpy(img).cuda()
    out = _Buf(m * m, torch.float64)
    L.check(L.load().bp_tile_crop(L.ptr(dev), 64, r0, c0, m, out.ptr, G.stream()), "tile crop")
    got = out.get().reshape(m, m)
    ref = LC.get_tile(np.asarray(img, dtype=np.float64), shift=(r0 / 64, c0 / 64), tile_relative_size=m / 64)
    assert ref.shape == (m, m) and np.array_equal(got, ref) and np.array_equal(got, S.crop(img, r0, c0, m))
    assert np.array_equal(dev.cpu().numpy(), img)


def test_guards_write_nothing():
    lib = L.load()
    host, dev = _planes(np.float32)[0]
    big = 1 << 30

    # bp_window_zoom
    def refused(code, **kw):
        rc, out, scratch = _window_zoom(dev, kw.pop("x0", 3), kw.pop("y0", 5), kw.pop("size", 40), kw.pop("tile", 64),
                                        **kw)
        assert rc == code, (rc, code, kw)
        assert np.isnan(out.get()).all() and np.isnan(scratch.get()).all()
    ws = int(lib.bp_window_zoom_workspace(40, 64))
    assert ws == 2 * 40 * 40 * 8
    assert lib.bp_window_zoom_workspace(1, 64) == 0 and lib.bp_window_zoom_workspace(40, 1) == 0
    assert lib.bp_window_zoom_workspace(46341, 64) == 0 and lib.bp_window_zoom_workspace(40, 46341) == 0
    for kw in (dict(plane=None), dict(scratch=None), dict(out=None), dict(rows=0), dict(cols=0), dict(size=1),
               dict(tile=1), dict(dtype=L.BF16), dict(dtype=7)):
        refused(L.BP_EINVAL, **kw)
    for kw in (dict(size=46341), dict(tile=46341), dict(x0=big), dict(x0=-big), dict(y0=big), dict(y0=-big)):
        refused(L.BP_EUNSUPPORTED, **kw)
    refused(L.BP_EWORKSPACE, scratch_bytes=ws - 8)
    refused(L.BP_EWORKSPACE, scratch_bytes=0)
    refused(L.BP_EINVAL, size=1, x0=big, scratch_bytes=0)        # the order: EINVAL, EUNSUPPORTED, EWORKSPACE
    refused(L.BP_EUNSUPPORTED, x0=big, scratch_bytes=0)

    # bp_window_min
    def refused_min(code, **kw):
        rc, out = _window_min(dev, kw.pop("x0", 3), kw.pop("y0", 5), kw.pop("size", 40), **kw)
        assert rc == code, (rc, code, kw)
        assert np.isnan(out.get()).all() and np.isnan(out.scratch.get()).all()
    for kw in (dict(plane=None), dict(scratch=None), dict(out=None), dict(rows=0), dict(cols=0), dict(size=0),
               dict(dtype=L.BF16)):
        refused_min(L.BP_EINVAL, **kw)
    for kw in (dict(size=46341), dict(x0=big), dict(x0=-big), dict(y0=big), dict(y0=-big)):
        refused_min(L.BP_EUNSUPPORTED, **kw)
    refused_min(L.BP_EWORKSPACE, scratch_bytes=int(lib.bp_window_min_workspace()) - 8)

    # bp_tile_crop
    img = torch.zeros((64, 64), dtype=torch.float32, device="cuda")
    out = _Buf(32 * 32, torch.float64)
    for args, code in (((None, 64, 16, 16, 32, out.ptr), L.BP_EINVAL), ((L.ptr(img), 64, 16, 16, 32, None), L.BP_EINVAL),
                       ((L.ptr(img), 0, 16, 16, 32, out.ptr), L.BP_EINVAL),
                       ((L.ptr(img), 64, 16, 16, 0, out.ptr), L.BP_EINVAL),
                       ((L.ptr(img), 46341, 16, 16, 32, out.ptr), L.BP_EUNSUPPORTED),
                       ((L.ptr(img), 64, big, 16, 32, out.ptr), L.BP_EUNSUPPORTED),
                       ((L.ptr(img), 64, 16, -big, 32, out.ptr), L.BP_EUNSUPPORTED)):
        assert lib.bp_tile_crop(*args, G.stream()) == code, args
    assert np.isnan(out.get()).all()
    assert np.array_equal(dev.cpu().numpy(), host)


# ---------------------------------------------------------------------------------------------------- the painters
# a plane of size 32 < 64 from a 256-pixel mass plane of size 128: a window of 128 -> 64 and a crop of 32 at 16
TILE, RES = 64, 120
SHIFT, DELTA, TILE_SIZE, MASS_SIZE, Z = (0.9, 0.85), 32.0, 64.0, 128.0, 0.05
SMALL = (SHIFT, DELTA, TILE_SIZE, MASS_SIZE, TILE, Z)


def _single_field_dataset():
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    tr = T.chain_transformations([fwd, T.atleast_3d, T.as_float32])
    itr = T.chain_transformations([T.squeeze, inv])
    return BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=1,
                          n_stack=3, transform=tr, inverse_transform=itr, scale_to_SLICS=True)


def _checkpointed(tmp, arch, ds, prepare=None):
    """A 64x64 CVAE painter with non-trivial running statistics, loaded from checkpoint files (the fixture of
    tests/test_gpu_ymap.py)."""
    from baryon_painter_amd.painter import CVAEPainter
    torch.manual_seed(3)
    p = CVAEPainter(training_data_set=ds, test_data_set=ds, architecture=arch, compute_device="cuda:0")
    x, y, aux = syn.synthetic_batch(4, TILE, TILE, seed=77)
    sx = (1.0 - 0.15 * np.arange(arch["dim_x"][0], dtype=np.float32))[None, :, None, None]
    sy = (1.0 - 0.2 * np.arange(arch["dim_y"][0], dtype=np.float32))[None, :, None, None]
    with torch.no_grad():
        p.model(torch.from_numpy(x * sx), torch.from_numpy(y * sy), torch.from_numpy(aux))
        if prepare is not None:
            prepare(p.model)
    files = (str(tmp / "state"), str(tmp / "meta"))
    p.save_state_to_file(files)
    return CVAEPainter(filename=files, compute_device="cuda:0")


def _build(kind, tmp):
    if kind == "cvae":
        return _checkpointed(tmp, A.fiducial_architecture(TILE), _single_field_dataset())
    if kind == "noise":                            # a variance head whose last convolution has a bias, set to -4
        arch = A.fiducial_architecture(TILE, predict_var=True)
        mu, var = arch["p_y_z_out"]
        name, cfg = var[-1]
        arch["p_y_z_out"] = (mu, list(var[:-1]) + [(name, dict(cfg, bias=True))])

        def bias(model):
            [m for m in model.p_var_out.modules() if getattr(m, "bias", None) is not None][-1].bias.fill_(-4.0)
        return _checkpointed(tmp, arch, _single_field_dataset(), bias)
    if kind in ("two fields", "two fields, split scale"):
        scales = None if kind == "two fields" else (2, 4, False)
        levels = 1 if scales is None else scales[0] + int(scales[2])
        tr, itr = MF.chains(T, scales=scales)
        ds = BAHAMASDataset(data=MF.data_dict3(), redshifts=list(HC.REDSHIFTS), label_fields=list(MF.LABELS), n_tile=1,
                            n_stack=3, transform=tr, inverse_transform=itr, n_feature_per_field=levels,
                            scale_to_SLICS=True)
        return _checkpointed(tmp, A.fiducial_architecture(TILE, n_fields=len(MF.LABELS), n_scale=levels), ds)
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
            cache[kind] = _build(kind, tmp_path_factory.mktemp("ckpt"))
        return cache[kind]
    return get


@pytest.fixture(scope="module")
def mass():
    host = _smooth(256, 256, 43)
    return host, torch.from_numpy(host).cuda()


def _chain(p, mass_d, seed, tile_id, subtract_minimum=False, pixel_noise=False, field=None):
    """bp_window_zoom's tile from the C ABI, painted by ``paint_stream`` at batch 1, cropped on the host."""
    geo = LC.small_plane_geometry(mass_d.shape[0], SHIFT, DELTA, TILE_SIZE, MASS_SIZE, TILE)
    assert (geo["cut"], geo["crop"], geo["r0"], geo["c0"]) == (128, 32, 16, 16)
    assert geo["x0"] + geo["cut"] > 256 and geo["y0"] + geo["cut"] > 256            # the window wraps on both axes
    tile = _device_tile(mass_d, geo["x0"], geo["y0"], geo["cut"], TILE, subtract_minimum)
    noise = {"pixel_noise": True} if pixel_noise else {}
    painted = p.paint_stream(tile[None], Z, batch_size=1, tile_ids=np.array([tile_id], dtype=np.int64), seed=seed,
                             **noise)[0]
    if field is not None:
        painted = painted[list(p.label_fields).index(field)]
    assert painted.shape == (TILE, TILE) and painted.dtype == np.float32
    return S.crop(painted, geo["r0"], geo["c0"], geo["crop"])


def _report_host(p, host_mass, dev_plane, **kw):
    """Print (never assert) the device plane against the all-host path's."""
    try:
        import scipy.ndimage  # noqa: F401
    except ImportError:
        return
    ref = LC.paint_small_plane(p, host_mass, *SMALL, **kw)
    top = np.abs(ref).max()
    print(f"max |device - host| = {np.abs(dev_plane - ref).max() / top:.3e} of the plane's maximum {top:.3e} "
          f"({kw})")


@pytest.mark.parametrize("case", ["plain", "subtract_minimum", "pixel_noise"])
def test_small_plane_is_the_chain_of_bits(painters, mass, case):
    p = painters("noise" if case == "pixel_noise" else "cvae")
    host, dev = mass
    kw = {} if case == "plain" else {case: True}
    ref = _chain(p, dev, 5, 9, **kw)
    got = LC.paint_small_plane(p, host, *SMALL, seed=5, tile_id=9, on_device=True, **kw)      # the window is uploaded
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (32, 32)
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    assert np.array_equal(got, ref)
    before = dev.clone()
    got_d = LC.paint_small_plane(p, dev, *SMALL, seed=5, tile_id=9, on_device=True, **kw)      # the plane in place
    assert np.array_equal(got_d, got) and torch.equal(dev, before)
    out = torch.full((32, 32), 3.0, dtype=torch.float64, device="cuda")
    r = LC.paint_small_plane(p, dev, *SMALL, seed=5, tile_id=9, on_device=True, out=out, **kw)
    assert r is out and np.array_equal(out.cpu().numpy(), got)
    # a float64 mass plane takes the kernels' other instantiation: its own chain
    got64 = LC.paint_small_plane(p, host.astype(np.float64), *SMALL, seed=5, tile_id=9, on_device=True, **kw)
    geo = LC.small_plane_geometry(256, SHIFT, DELTA, TILE_SIZE, MASS_SIZE, TILE)
    tile64 = _device_tile(dev.double(), geo["x0"], geo["y0"], geo["cut"], TILE, case == "subtract_minimum")
    noise = {"pixel_noise": True} if case == "pixel_noise" else {}
    painted = p.paint_stream(tile64[None], Z, batch_size=1, tile_ids=np.array([9], dtype=np.int64), seed=5, **noise)[0]
    assert np.array_equal(got64, S.crop(painted, 16, 16, 32))
    if case == "pixel_noise":                                    # the draw is not the mean, and another lattice another draw
        mean = LC.paint_small_plane(p, dev, *SMALL, seed=5, tile_id=9, on_device=True)
        assert not np.array_equal(mean, got)
    _report_host(p, host, got, seed=5, tile_id=9, **kw)
    with pytest.raises(ValueError):                              # out= of another shape
        LC.paint_small_plane(p, dev, *SMALL, seed=5, on_device=True,
                             out=torch.zeros((31, 31), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):                              # a window that does not zoom to the tile
        LC.paint_small_plane(p, dev, SHIFT, DELTA, TILE_SIZE, 12800.0, TILE, Z, seed=5, on_device=True)


def test_small_plane_seeds(painters, mass):
    p = painters("cvae")
    host, dev = mass
    a = LC.paint_small_plane(p, dev, *SMALL, seed=11, tile_id=3, on_device=True)
    assert np.array_equal(a, LC.paint_small_plane(p, dev, *SMALL, seed=11, tile_id=3, on_device=True))
    assert not np.array_equal(a, LC.paint_small_plane(p, dev, *SMALL, seed=12, tile_id=3, on_device=True))
    assert not np.array_equal(a, LC.paint_small_plane(p, dev, *SMALL, seed=11, tile_id=4, on_device=True))
    torch.manual_seed(123)                                       # seed=None: a fresh key from torch's generator
    b = LC.paint_small_plane(p, dev, *SMALL, on_device=True)
    c = LC.paint_small_plane(p, dev, *SMALL, on_device=True)
    assert not np.array_equal(b, c)
    torch.manual_seed(123)
    assert np.array_equal(LC.paint_small_plane(p, dev, *SMALL, on_device=True), b)
    assert any(k[0] == "small" for k in p.__dict__["_plane_device_buffers"])
    p.release_paint_buffers()
    assert "_plane_device_buffers" not in p.__dict__
    assert np.array_equal(LC.paint_small_plane(p, dev, *SMALL, seed=11, tile_id=3, on_device=True), a)


@pytest.mark.parametrize("kind", ["two fields", "two fields, split scale"])
def test_small_plane_of_a_named_field(painters, mass, kind):
    p = painters(kind)
    host, dev = mass
    planes = {}
    for field in MF.LABELS:
        planes[field] = LC.paint_small_plane(p, dev, *SMALL, seed=5, tile_id=2, field=field, on_device=True)
        assert np.array_equal(planes[field], _chain(p, dev, 5, 2, field=field))
        assert np.isfinite(planes[field]).all()
    assert not np.array_equal(planes[MF.LABELS[0]], planes[MF.LABELS[1]])
    assert np.array_equal(LC.paint_small_plane(p, host, *SMALL, seed=5, tile_id=2, field=MF.LABELS[1], on_device=True),
                          planes[MF.LABELS[1]])
    state = torch.get_rng_state()
    with pytest.raises(ValueError):                              # several fields and no name
        LC.paint_small_plane(p, dev, *SMALL, on_device=True)
    with pytest.raises(ValueError):
        LC.paint_small_plane(p, dev, *SMALL, field="stars", on_device=True)
    assert torch.equal(torch.get_rng_state(), state)
    _report_host(p, host, planes[MF.LABELS[0]], seed=5, tile_id=2, field=MF.LABELS[0])


def test_small_plane_of_a_cgan_painter(painters, mass):
    p = painters("cgan")
    host, dev = mass
    for subtract_minimum in (False, True):
        got = LC.paint_small_plane(p, dev, *SMALL, seed=5, tile_id=1, subtract_minimum=subtract_minimum, on_device=True)
        assert got.shape == (32, 32) and np.isfinite(got).all()
        assert np.array_equal(got, _chain(p, dev, 5, 1, subtract_minimum=subtract_minimum))
        assert np.array_equal(got, LC.paint_small_plane(p, host, *SMALL, subtract_minimum=subtract_minimum,
                                                        on_device=True))       # no latent noise: no seed to tell
    _report_host(p, host, got, subtract_minimum=True)
    with pytest.raises(ValueError):                              # no likelihood to draw from
        LC.paint_small_plane(p, dev, *SMALL, pixel_noise=True, on_device=True)


def test_ineligible_painter_raises_before_a_seed_is_drawn(painters, mass):
    q = painters("cvae")
    host, dev = mass

    def doubled(x, field, z, stats):
        return 2.0 * x
    good = q.transform
    try:
        q.transform = type(good)(T.chain_transformations([doubled] + list(good.func.steps)), good.stats)
        n_graphs = len(q.model._graphs)
        state = torch.get_rng_state()
        with pytest.raises(NotImplementedError):
            LC.paint_small_plane(q, dev, *SMALL, on_device=True)
        with pytest.raises(NotImplementedError):
            LC.paint_light_cone(q, [(host, SHIFT, MASS_SIZE)], [Z], [DELTA], TILE_SIZE, TILE, RES, [1.0], on_device=True,
                                small_planes_on_device=True)
        assert torch.equal(torch.get_rng_state(), state)
        assert len(q.model._graphs) == n_graphs
    finally:
        q.transform = good

    class HostOnly:
        def paint(self, input, z=0.0, transform=True, inverse_transform=True):
            return input
    state = torch.get_rng_state()
    with pytest.raises(NotImplementedError):
        LC.paint_small_plane(HostOnly(), dev, *SMALL, on_device=True)
    assert torch.equal(torch.get_rng_state(), state)


# -------------------------------------------------------------------------------------------------- the light cone
KW = dict(tile_size=TILE_SIZE, n_pixel_tile=TILE, resolution=RES, batch_size=8)


def _delta(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (np.exp(rng.standard_normal((n, n)) * 0.5) * 0.05).astype(np.float32)


def _cone():
    """Planes small, zoomed (200 pixels of size 150: 85 -> 64 cuts), plain (150 pixels of size 150), as
    tests/test_gpu_ymap.py's."""
    planes = [(_smooth(256, 256, 43), SHIFT, MASS_SIZE), _smooth(200, 200, 42), _delta(150, 41)]
    z, size = [Z, 0.3, 0.42], [DELTA, 150.0, 150.0]
    scales = LC.y_map_scales([32, 150, 150], RES, 10.0, np.array([200.0, 1100.0, 1500.0]),
                             lambda c: 1 / (1 + c / 3300.0), 0.69)
    return planes, z, size, scales


def test_light_cone_with_small_planes_on_the_device(painters):
    p = painters("cvae")
    planes, z, size, scales = _cone()
    dev, dp = LC.paint_light_cone(p, iter(planes), z, size, scales=scales, seed=6, on_device=True,
                                  small_planes_on_device=True, return_planes=True, **KW)
    assert dev.shape == (RES, RES) and dev.dtype == np.float64 and np.isfinite(dev).all() and np.abs(dev).max() > 0
    # the same planes one by one, under the same key and tile ids: the small plane takes one id, a tiled plane n_side^2
    n1 = LC.plane_geometry(200, TILE_SIZE / 150.0, TILE)["n_side"] ** 2
    one = [LC.paint_small_plane(p, *planes[0][:2], DELTA, TILE_SIZE, MASS_SIZE, TILE, Z, seed=6, tile_id=0,
                                on_device=True),
           LC.paint_plane(p, planes[1], TILE_SIZE / 150.0, TILE, z[1], batch_size=8, seed=6, first_tile_id=1,
                          on_device=True),
           LC.paint_plane(p, planes[2], TILE_SIZE / 150.0, TILE, z[2], batch_size=8, seed=6, first_tile_id=1 + n1,
                          on_device=True)]
    assert [a.shape for a in dp] == [(32, 32), (150, 150), (150, 150)]
    for a, b in zip(dp, one):
        assert isinstance(a, np.ndarray) and np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(dev, LC.project_planes(one, scales, RES, on_device=True))
    # a CUDA mass plane is cut in place: the same bits
    on_dev = [(torch.from_numpy(planes[0][0]).cuda(), SHIFT, MASS_SIZE)] + planes[1:]
    again = LC.paint_light_cone(p, on_dev, z, size, scales=scales, seed=6, on_device=True, small_planes_on_device=True,
                                **KW)
    assert np.array_equal(again, dev)
    # out= is accumulated into
    rng = np.random.Generator(np.random.PCG64(18))
    y0 = rng.standard_normal((RES, RES)) * np.abs(dev).max()
    out = torch.from_numpy(y0).cuda()
    r = LC.paint_light_cone(p, planes, z, size, scales=scales, seed=6, on_device=True, small_planes_on_device=True,
                            out=out, **KW)
    ref = LC.project_planes(one, scales, RES, on_device=True, out=torch.from_numpy(y0).cuda())
    assert r is out and torch.equal(out, ref) and not np.array_equal(out.cpu().numpy(), y0)
    # with the flag off the small plane is the host path's (tests/test_gpu_ymap.py); with it on it is the device's
    try:
        import scipy.ndimage  # noqa: F401
    except ImportError:
        return
    _, hp = LC.paint_light_cone(p, planes, z, size, scales=scales, seed=6, on_device=True, return_planes=True, **KW)
    top = np.abs(hp[0]).max()
    print(f"small plane, device against host: max |difference| = {np.abs(dp[0] - hp[0]).max() / top:.3e} of the "
          f"plane's maximum {top:.3e}")
    for a, b in zip(dp[1:], hp[1:]):
        assert np.array_equal(a, b, equal_nan=True)
    with pytest.raises(ValueError):
        LC.paint_light_cone(p, planes, z, size, scales=scales, seed=6, small_planes_on_device=True, **KW)
