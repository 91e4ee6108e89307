"""GPU: the four entry points of csrc/plane.hip through the C ABI, each against a float64 restatement of the same
operation (tests/plane_ref.py, pinned on the CPU by tests/test_plane_kernels_host.py), at the edges of their contracts.

Every output and scratch buffer lies between MARGIN-element canaries that are checked after every call, every successful
call is made twice and must give the same bits, and every refusal must leave its buffers as they were.

Limits.  The gather and the blend are bit for bit.  A resampled pixel passes within 1 float32 ulp of
float32(plane_ref.zoom(...)) (tests/test_gpu_paint_plane_device.py's limit: device pow and divisions may differ in the
last double bit) or within LIMIT = 1e-12 of max |ref| of its tile (the projection's limit, for pixels that cancel to near
zero, where an ulp is smaller than the float64 rounding of the sixteen taps).  SciPy is compared with from cut = 12 only:
below, its "reflect" prefilter is not the exact spline (tests/test_plane_kernels_host.py).  Tile statistics: 4 float64
ulps of plane_ref.device_tile_stats, from the tt 2^-52 summation bound at tt <= 289; the masks then cannot differ, because
the inputs keep every pixel 1e-9 std away from the threshold (asserted on the CPU)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import plane_cases as PC
import plane_ref as R
from baryon_painter_amd import _lib as L
from baryon_painter_amd import lightcone as LC

import gpu_util as G

pytestmark = pytest.mark.gpu

LIMIT = 1e-12
MARGIN = 1024                                     # elements of canary on either side of every output and scratch
CANARY = -7.25
OK, EINVAL, EUNSUPPORTED, EWORKSPACE = L.BP_OK, L.BP_EINVAL, L.BP_EUNSUPPORTED, L.BP_EWORKSPACE

_T0 = [0.0]


def setup_module(module):
    _T0[0] = time.time()


def teardown_module(module):
    torch.cuda.synchronize()
    print(f"\ntest_gpu_plane_kernels: {time.time() - _T0[0]:.1f} s wall")


class _Buf:
    """``n`` elements between two canary margins.  content=None leaves the inside canary as well."""

    def __init__(self, n, dtype, content=None):
        self.n = n
        self.full = torch.full((n + 2 * MARGIN,), CANARY, dtype=dtype, device="cuda")
        self.inner = self.full[MARGIN:MARGIN + n]
        if content is not None:
            self.inner.copy_(torch.from_numpy(np.ascontiguousarray(content).reshape(-1)))

    @property
    def ptr(self):
        return C.c_void_p(self.inner.data_ptr())

    def get(self):
        torch.cuda.synchronize()
        h = self.full.cpu().numpy()
        assert (h[:MARGIN] == CANARY).all() and (h[MARGIN + self.n:] == CANARY).all(), "written outside the buffer"
        return h[MARGIN:MARGIN + self.n].copy()

    def untouched(self):
        return bool((self.get() == CANARY).all())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(got, ref, what=""):
    """Equal bit patterns (so -0.0 is not +0.0) outside NaNs, and NaNs in the same places."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN positions")
    bad = _bits(got)[~nan] != _bits(ref)[~nan]
    assert not bad.any(), (what, int(bad.sum()), "pixels differ; first at", int(np.flatnonzero(bad)[0]))


def _ulps(a, b):
    ia, ib = (np.asarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _ulps64(a, b):
    ia, ib = (np.asarray(v, np.float64).view(np.int64) for v in (a, b))
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFFFFFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFFFFFFFFFF), ib)
    return np.abs(ia - ib)


# ---------------------------------------------------------------------------------------------------------- cut

class _Cut:
    """One bp_plane_cut call: the plane and origins on the device, `out` and the scratch (canary inside and out, with
    room for the whole workspace whatever scratch_bytes says) in guarded buffers."""

    def __init__(self, plane, origins, cut, tile, lead=0):
        self.lib = L.load()
        self.plane, self.cut, self.tile = plane, cut, tile
        self.n = len(origins)
        self.pd = _dev(plane)
        org = np.asarray(origins, np.int64).astype(np.int32).reshape(-1, 2)
        junk = np.full((lead, 2), 12345, np.int32)                 # the painter passes origins + 2 * a
        self.od = _dev(np.concatenate([junk, org]))
        self.lead = lead
        self.ws = int(self.lib.bp_plane_cut_workspace(self.n, cut, tile))
        self.out = _Buf(self.n * tile * tile, torch.float32)
        self.scratch = _Buf(max(self.ws // 8, 1), torch.float64)

    def call(self, scratch_bytes=None, **over):
        a = dict(plane=L.ptr(self.pd), dtype=L.F32 if self.plane.dtype == np.float32 else L.F64,
                 rows=self.plane.shape[0], cols=self.plane.shape[1],
                 origins=C.c_void_p(self.od.data_ptr() + 8 * self.lead), n=self.n, cut=self.cut, tile=self.tile,
                 scratch=self.scratch.ptr, scratch_bytes=self.ws if scratch_bytes is None else scratch_bytes,
                 out=self.out.ptr)
        a.update(over)
        return self.lib.bp_plane_cut(a["plane"], a["dtype"], a["rows"], a["cols"], a["origins"], a["n"], a["cut"],
                                     a["tile"], a["scratch"], a["scratch_bytes"], a["out"], G.stream())

    def result(self):
        out = self.out.get().reshape(self.n, self.tile, self.tile)
        self.scratch.get()
        assert np.array_equal(_bits(self.pd.cpu().numpy()), _bits(self.plane)), "the plane was modified"
        return out

    def refused(self):
        return self.out.untouched() and self.scratch.untouched()


def _device_cut(plane, origins, cut, tile, scratch_bytes=None, lead=0):
    """The (n, tile, tile) tiles of a call that must succeed, made twice into fresh buffers."""
    outs = []
    for _ in range(2):
        c = _Cut(plane, origins, cut, tile, lead)
        assert c.call(scratch_bytes) == OK
        outs.append(c.result())
        if scratch_bytes is not None:                              # nothing is stored behind scratch_bytes
            s = c.scratch.get()
            assert (s[-(-scratch_bytes // 8):] == CANARY).all(), "stored behind scratch_bytes"
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])), "two calls, two results"
    return outs[0]


def _gather_plane(shape, dtype, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    rows, cols = shape
    if dtype == np.float64:
        p = rng.standard_normal(shape) * 3
        special = [np.nan, np.inf, -np.inf, -0.0,
                   1 + 2.0 ** -24, 3.5e38, 1e-40, 2.0 ** -150, -1e-50,                 # a tie, to inf, subnormal, to +-0
                   1 + 3 * 2.0 ** -24, -(1 + 2.0 ** -24), 1 + 2.0 ** -24 + 2.0 ** -50,   # ties to even, and just above one
                   -1e300, 2.0 ** 128 - 2.0 ** 103, np.nextafter(2.0 ** 128 - 2.0 ** 103, 0),   # to -inf, to inf, to max
                   -1e-40, 2.0 ** -149, 1.5 * 2.0 ** -150, 1e-300, 0.0]
    else:
        p = (rng.standard_normal(shape) * 3).astype(np.float32)
        special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -1e-45, 3.4028235e38, -3.4028235e38], np.float32)
    flat = p.reshape(-1)
    where = rng.permutation(flat.size)[:len(special)]              # (a plane of 9 pixels takes the first nine)
    flat[where] = np.asarray(special, dtype)[:len(where)]
    return p


def _gather_origins(rows, cols, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    fixed = [(0, 0), (-37, 250), (-rows - 3, 3 * cols + 1), (2 ** 31 - 1, -2 ** 31)]
    more = rng.integers(-2 ** 31, 2 ** 31, (max(n - 4, 0), 2))
    return np.concatenate([np.asarray(fixed, np.int64), more])[:n]


def _gather_ref(plane, origins, tile):
    with np.errstate(over="ignore", under="ignore"):
        return np.stack([R.cut_ref(plane, x, y, tile).astype(np.float32) for x, y in origins])


def _check_gather(got, ref, dtype):
    if dtype == np.float32:                                        # a copy: NaNs keep their bits too
        assert np.array_equal(_bits(got), _bits(ref))
    else:
        _same_bits(got, ref)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(150, 130), (5, 7), (1, 9), (9, 1)])
def test_gather_is_the_wrapped_cut_bit_for_bit(shape, dtype):
    plane = _gather_plane(shape, dtype, 11 + shape[0])
    assert np.isnan(plane).any() and np.isinf(plane).any() and (_bits(plane) == _bits(np.array(-0.0, dtype))).any()
    for tile, n, lead in ((1, 7, 0), (2, 5, 3), (5, 7, 1), (16, 4, 0), (64, 5, 2)):
        if tile < 16:
            assert n * tile * tile % 256                           # a ragged last workgroup
        origins = _gather_origins(*shape, n, tile)
        got = _device_cut(plane, origins, tile, tile, lead=lead)
        _check_gather(got, _gather_ref(plane, origins, tile), dtype)


def test_gather_of_65538_single_pixel_tiles():
    plane = _gather_plane((5, 7), np.float64, 3)
    origins = _gather_origins(5, 7, 65538, 4)
    got = _device_cut(plane, origins, 1, 1)
    ix, iy = origins[:, 0] % 5, origins[:, 1] % 7
    with np.errstate(over="ignore", under="ignore"):
        _same_bits(got.reshape(-1), plane[ix, iy].astype(np.float32))


def test_gather_needs_no_scratch():
    plane = _gather_plane((5, 7), np.float32, 5)
    origins = _gather_origins(5, 7, 4, 6)
    c = _Cut(plane, origins, 5, 5)
    assert c.call(scratch=None, scratch_bytes=0) == OK
    _check_gather(c.result(), _gather_ref(plane, origins, 5), np.float32)
    assert c.scratch.untouched()


def _zoom_plane(shape, dtype, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (np.exp(rng.standard_normal(shape) * 0.5) * 0.05 - 0.04).astype(dtype)      # signs of both kinds


def _zoom_ref(plane, origins, cut, tile, zoom=None):
    zoom = R.zoom if zoom is None else zoom
    return np.stack([np.asarray(zoom(R.cut_ref(plane, x, y, cut).astype(np.float64), tile), np.float32)
                     for x, y in origins])


def _scipy_zoom():
    try:
        import scipy.ndimage as nd
    except ImportError:
        return None
    return lambda a, n_out: nd.zoom(a, n_out / a.shape[0], order=3, mode="reflect")


def _check_zoom(got, ref, what):
    """1 float32 ulp or LIMIT * max |ref| of the tile on every pixel; returns the worst of each."""
    assert np.isfinite(got).all(), what
    worst_u, worst_r = 0, 0.0
    for t in range(len(ref)):
        u = _ulps(got[t], ref[t])
        err = np.abs(got[t].astype(np.float64) - ref[t].astype(np.float64))
        top = np.abs(ref[t]).max()
        ok = (u <= 1) | (err <= LIMIT * top)
        worst_u, worst_r = max(worst_u, int(u.max())), max(worst_r, float((err / top).max()))
        assert ok.all(), (what, t, int(u[~ok].max()), float(err[~ok].max() / top))
    return worst_u, worst_r


# origins on a (150, 130) plane that wrap on neither axis, on rows, on columns and on both (for every cut from 2 to
# 129), and ones many periods away on either side
_ZOOM_ORIGINS = [(0, 0), (149, 0), (3, 129), (149, 129), (-1000003, 777777), (75, 60), (2 ** 31 - 1, -2 ** 31)]
_PAIRS = [(2, 3), (3, 2), (2, 64), (5, 4), (7, 16), (12, 16), (31, 32), (33, 32), (65, 64), (64, 65), (129, 16), (96, 7)]


@pytest.mark.parametrize("cut,tile", _PAIRS)
def test_zoom_is_the_exact_spline_of_the_wrapped_cut(cut, tile):
    scipy_zoom = _scipy_zoom() if cut >= 12 else None
    planes = [("f32 (150, 130)", _zoom_plane((150, 130), np.float32, cut)),
              ("f64 (150, 130)", _zoom_plane((150, 130), np.float64, cut + 1)),
              ("f64 (5, 7)", _zoom_plane((5, 7), np.float64, cut + 2))]
    for name, plane in planes:
        ref = _zoom_ref(plane, _ZOOM_ORIGINS, cut, tile)
        full = _device_cut(plane, _ZOOM_ORIGINS, cut, tile)
        wu, wr = _check_zoom(full, ref, (cut, tile, name))
        line = f"({cut}, {tile}) {name}: worst {wu} ulp, worst |err| / max|ref| = {wr:.2e}"
        if scipy_zoom is not None:
            su, sr = _check_zoom(full, _zoom_ref(plane, _ZOOM_ORIGINS, cut, tile, scipy_zoom), (cut, tile, name, "scipy"))
            line += f"; against scipy {su} ulp, {sr:.2e}"
        print(line)
        assert 7 * cut % 256 and 3 * cut % 256 and cut % 256       # a ragged last workgroup of lines (m * cut of them)
        for n in (1, 3):                                           # a tile's bits do not depend on the batch
            part = _device_cut(plane, _ZOOM_ORIGINS[:n], cut, tile)
            assert np.array_equal(_bits(part), _bits(full[:n])), (cut, tile, name, n)


@pytest.mark.parametrize("cut,tile", [(33, 32), (85, 64)])
def test_short_scratch_works_in_chunks(cut, tile):
    plane = _zoom_plane((150, 130), np.float32, 70 + cut)
    origins = _ZOOM_ORIGINS[:5]
    share = 16 * cut * cut
    assert L.load().bp_plane_cut_workspace(5, cut, tile) == 5 * share
    full = _device_cut(plane, origins, cut, tile)
    _check_zoom(full, _zoom_ref(plane, origins, cut, tile), (cut, tile))
    for nbytes in (share, 2 * share, 2 * share + share // 2, 2 * share - 1, 5 * share + 8):   # chunks of 1; 2, 2, 1; 2; 1; 5
        got = _device_cut(plane, origins, cut, tile, scratch_bytes=nbytes)
        assert np.array_equal(_bits(got), _bits(full)), nbytes
    c = _Cut(plane, origins, cut, tile)
    assert c.call(scratch_bytes=share - 1) == EWORKSPACE and c.refused()
    assert c.call(scratch_bytes=0) == EWORKSPACE and c.refused()


def test_grid_cap_chunks_of_65535_tiles():
    cut, tile, n = 2, 3, 65538
    plane = _zoom_plane((150, 130), np.float32, 90)
    rng = np.random.Generator(np.random.PCG64(91))
    origins = rng.integers(-2 ** 31, 2 ** 31, (n, 2))
    assert L.load().bp_plane_cut_workspace(n, cut, tile) == 16 * n * 4
    got = _device_cut(plane, origins, cut, tile)                   # chunks of 65535 and 3
    pick = np.concatenate([[0, 65534, 65535, 65537], rng.integers(0, n, 100)])
    _check_zoom(got[pick], _zoom_ref(plane, origins[pick], cut, tile), "grid cap")
    first = _device_cut(plane, origins[:40000], cut, tile)
    rest = _device_cut(plane, origins[40000:], cut, tile)
    assert np.array_equal(_bits(got), _bits(np.concatenate([first, rest])))


def test_tiles_are_independent_of_batch_position_and_neighbours():
    cut, tile = 33, 32
    plane = _zoom_plane((150, 130), np.float64, 95)
    origins = [(0, 0), (40, 40), (80, 80), (100, 0), (40, 90), (110, 50), (0, 60)]      # no window overlaps tile 0's
    full = _device_cut(plane, origins, cut, tile)
    back = _device_cut(plane, origins[::-1], cut, tile, scratch_bytes=3 * 16 * cut * cut)
    assert np.array_equal(_bits(back[::-1]), _bits(full))
    for t in (0, 3, 6):
        assert np.array_equal(_bits(_device_cut(plane, origins[t:t + 1], cut, tile)[0]), _bits(full[t]))
    poisoned = plane.copy()
    poisoned[17, 20] = np.nan                                      # inside tile 0's window only
    got = _Cut(poisoned, origins, cut, tile)
    assert got.call() == OK
    out = got.result()
    assert np.isnan(out[0]).any()
    assert np.array_equal(_bits(out[1:]), _bits(full[1:]))


def test_cut_return_codes_leave_everything_untouched():
    lib = L.load()
    plane = _zoom_plane((5, 7), np.float32, 96)
    origins = [(0, 0), (3, 4)]
    big = 1 << 40                                                  # scratch_bytes is never the reason below

    def refused(code, base=(4, 3), **over):
        c = _Cut(plane, origins, *base)
        assert c.call(**over) == code, (code, base, over)
        assert c.refused(), (base, over)

    for base in ((4, 3), (4, 4)):
        for null in ("plane", "origins", "out"):
            refused(EINVAL, base, **{null: None})
        for name in ("rows", "cols", "n", "cut", "tile"):
            for v in (0, -1, -2 ** 31):
                refused(EINVAL, base, **{name: v})
        for dtype in (1, 3, -1):
            refused(EINVAL, base, dtype=dtype)
    refused(EINVAL, scratch=None)
    refused(EINVAL, cut=1, tile=3)
    refused(EINVAL, cut=3, tile=1)
    # products at 2^31: small real buffers, nothing is dereferenced before the refusal
    refused(EUNSUPPORTED, rows=65536, cols=32768, scratch_bytes=big)
    refused(EUNSUPPORTED, cut=64, tile=64, n=2 ** 31 // 64 ** 2)
    refused(EUNSUPPORTED, cut=64, tile=2, n=2 ** 31 // 64 ** 2, scratch_bytes=big)
    refused(EUNSUPPORTED, cut=2, tile=64, n=2 ** 31 // 64 ** 2, scratch_bytes=big)
    refused(EWORKSPACE, scratch_bytes=16 * 16 - 1)
    # order: BP_EINVAL, then BP_EUNSUPPORTED, then BP_EWORKSPACE
    refused(EINVAL, rows=65536, cols=32768, dtype=1)
    refused(EINVAL, n=0, scratch_bytes=0)
    refused(EUNSUPPORTED, rows=65536, cols=32768, scratch_bytes=0)
    refused(EUNSUPPORTED, cut=64, tile=2, n=2 ** 31 // 64 ** 2, scratch_bytes=0)
    # just below the limits nothing is refused on these grounds (the workspace is what is missing)
    refused(EWORKSPACE, cut=64, tile=2, n=2 ** 31 // 64 ** 2 - 1, scratch_bytes=0)
    for n, cut, tile, want in ((0, 4, 3, 0), (-1, 4, 3, 0), (3, 0, 3, 0), (3, -2, 3, 0), (3, 4, 4, 0), (3, 1, 1, 0),
                               (3, 4, 3, 16 * 3 * 16), (1, 2, 64, 64), (65538, 2, 3, 16 * 65538 * 4), (7, 129, 16, 16 * 7 * 129 ** 2),
                               (3, 4, 0, 16 * 3 * 16)):
        assert lib.bp_plane_cut_workspace(n, cut, tile) == want, (n, cut, tile)


# -------------------------------------------------------------------------------------------------------- blend

class _Blend:
    """Accumulators (fields, rows, cols) and stats (n * fields, 2) in guarded buffers; tiles (n, fields, tile, tile)."""

    def __init__(self, tiles, dst, rows, cols, weight, acc0, wsum0):
        self.lib = L.load()
        self.n, self.fields, self.tile = tiles.shape[0], tiles.shape[1], tiles.shape[-1]
        self.rows, self.cols = rows, cols
        self.td = _dev(np.ascontiguousarray(tiles, np.float32))
        self.dd = _dev(np.asarray(dst, np.int32).reshape(-1, 2))
        self.wd = _dev(np.asarray(weight, np.float64))
        self.acc = _Buf(self.fields * rows * cols, torch.float64, acc0)
        self.wsum = _Buf(self.fields * rows * cols, torch.float64, wsum0)
        self.stats = _Buf(2 * self.n * self.fields, torch.float64)

    def call(self, box, reg=None, use_fields=None, a=0, m=None, **over):
        m = self.n - a if m is None else m
        use_fields = self.fields > 1 if use_fields is None else use_fields
        tt = self.tile * self.tile
        k = dict(tiles=C.c_void_p(self.td.data_ptr() + 4 * a * self.fields * tt), n=m, fields=self.fields, tile=self.tile,
                 dst=C.c_void_p(self.dd.data_ptr() + 8 * a), bx0=box[0], by0=box[1], bx1=box[2], by1=box[3],
                 weight=L.ptr(self.wd), regularise=0 if reg is None else 1, regularise_std=0.0 if reg is None else float(reg),
                 stats=C.c_void_p(self.stats.inner.data_ptr() + 16 * a * self.fields), acc=self.acc.ptr, wsum=self.wsum.ptr,
                 rows=self.rows, cols=self.cols)
        k.update(over)
        if use_fields:
            return self.lib.bp_plane_blend_fields(
                k["tiles"], k["n"], k["fields"], k["tile"], k["dst"], k["bx0"], k["by0"], k["bx1"], k["by1"], k["weight"],
                k["regularise"], k["regularise_std"], k["stats"], k["acc"], k["wsum"], k["rows"], k["cols"], G.stream())
        assert k["fields"] == 1
        return self.lib.bp_plane_blend(
            k["tiles"], k["n"], k["tile"], k["dst"], k["bx0"], k["by0"], k["bx1"], k["by1"], k["weight"], k["regularise"],
            k["regularise_std"], k["stats"], k["acc"], k["wsum"], k["rows"], k["cols"], G.stream())

    def result(self):
        shape = (self.fields, self.rows, self.cols)
        return self.acc.get().reshape(shape), self.wsum.get().reshape(shape), self.stats.get().reshape(-1, 2)


def _device_blend(tiles, dst, rows, cols, weight, box, acc0, wsum0, reg=None, use_fields=None, batches=None,
                  null_stats=False):
    """(acc, wsum, stats) of the batches blended in turn over the same box, done twice into fresh buffers."""
    if tiles.ndim == 3:
        tiles = tiles[:, None]
    res = []
    for _ in range(2):
        b = _Blend(tiles, dst, rows, cols, weight, acc0, wsum0)
        a = 0
        for m in batches or [len(tiles)]:
            over = dict(stats=None) if null_stats else {}
            assert b.call(box, reg, use_fields, a, m, **over) == OK
            a += m
        assert a == len(tiles)
        res.append(b.result())
    for x, y in zip(*res):
        assert np.array_equal(_bits(x), _bits(y)), "two calls, two results"
    return res[0]


def _prior(shape, seed):
    """Accumulators that have been used: random content with -0.0 and a NaN here and there."""
    rng = np.random.Generator(np.random.PCG64(seed))
    acc0, wsum0 = rng.standard_normal(shape) * 5, rng.random(shape) * 3
    for a in (acc0, wsum0):
        flat = a.reshape(-1)
        where = rng.permutation(flat.size)[:24]
        flat[where[:12]] = -0.0
        flat[where[12:]] = np.nan
    return acc0, wsum0


def _weights(tile, kind):
    if kind == "random":
        return np.random.Generator(np.random.PCG64(tile)).random((tile, tile)) * 2 + 1e-3
    return LC.make_weight_map((tile, tile), falloff=0.4, sigma=0.5)


def _overhanging(rows, cols, t):
    """Tiles over each corner and each edge of the plane, some inside, and 40 on one spot."""
    h = (t + 1) // 2                                               # (a 1-pixel tile then lies outside altogether)
    lo, hx, hy = -h, rows - t + h, cols - t + h
    dst = [(lo, lo), (lo, hy), (hx, lo), (hx, hy), (lo, 5), (hx, 7), (4, lo), (9, hy), (3, 2), (10, 4), (-t, 3), (3, cols)]
    return np.asarray(dst + [(6, 5)] * 40, np.int32)


def _check_blend(got, tiles, dst, rows, cols, w, box, acc0, wsum0, what, stats=None, reg=None):
    acc, wsum = got
    ref_a, ref_w = R.blend_box(tiles, dst, rows, cols, w, box, acc0, wsum0, stats, reg)
    _same_bits(acc, ref_a, (what, "acc"))
    _same_bits(wsum, ref_w, (what, "wsum"))
    # what no tile reaches inside the box, and everything outside it, keeps its bits, NaNs included
    reached = np.zeros((rows, cols), bool)
    t = tiles.shape[-1]
    for x, y in np.asarray(dst, np.int64):
        reached[max(x, box[0]):max(min(x + t, box[2]), 0), max(y, box[1]):max(min(y + t, box[3]), 0)] = True
    assert np.array_equal(_bits(acc)[~reached], _bits(acc0)[~reached]), (what, "acc of unreached pixels")
    assert np.array_equal(_bits(wsum)[~reached], _bits(wsum0)[~reached]), (what, "wsum of unreached pixels")
    return reached


@pytest.mark.parametrize("tile", [1, 3, 16, 17])
@pytest.mark.parametrize("rows,cols", [(40, 23), (23, 40)])
def test_blend_is_the_pixel_loop_bit_for_bit(rows, cols, tile):
    dst = _overhanging(rows, cols, tile)
    n = len(dst)
    tiles = PC.wide_tiles((n, tile, tile), 100 + tile)
    acc0, wsum0 = _prior((rows, cols), 200 + tile)
    boxes = {"plane": (0, 0, rows, cols), "pixel": (6, 5, 7, 6), "through": (5, 3, rows - 4, cols - 6)}
    for kind in ("map", "random"):
        w = _weights(tile, kind)
        for name, box in boxes.items():
            what = (rows, cols, tile, kind, name)
            acc, wsum, stats = _device_blend(tiles, dst, rows, cols, w, box, acc0, wsum0)
            reached = _check_blend((acc[0], wsum[0]), tiles, dst, rows, cols, w, box, acc0, wsum0, what)
            assert reached.any() and (stats == CANARY).all()
            if name == "plane":
                assert not reached.all()
            # the same tiles in batches, and through bp_plane_blend_fields with one field
            a2, w2, _ = _device_blend(tiles, dst, rows, cols, w, box, acc0, wsum0, batches=[3, 4, n - 7])
            assert np.array_equal(_bits(a2), _bits(acc)) and np.array_equal(_bits(w2), _bits(wsum)), what
            a3, w3, _ = _device_blend(tiles, dst, rows, cols, w, box, acc0, wsum0, use_fields=True, null_stats=True)
            assert np.array_equal(_bits(a3), _bits(acc)) and np.array_equal(_bits(w3), _bits(wsum)), what
    # 40 + 2 terms in one pixel, summed in tile order: another order gives other bits
    if tile > 1:
        z = np.zeros((rows, cols))
        w = _weights(tile, "random")
        fwd = R.blend_box(tiles, dst, rows, cols, w, boxes["plane"], z, z)[0]
        bwd = R.blend_box(tiles[::-1], dst[::-1], rows, cols, w, boxes["plane"], z, z)[0]
        assert not np.array_equal(fwd, bwd)


def test_blend_with_tiles_in_one_corner_of_a_used_plane():
    rows, cols, tile = 40, 23, 3
    dst = np.asarray([(37, 20), (38, 21), (36, 19), (39, 22)], np.int32)
    tiles = PC.wide_tiles((4, tile, tile), 7)
    acc0, wsum0 = _prior((rows, cols), 8)
    w = _weights(tile, "map")
    box = (0, 0, rows, cols)
    acc, wsum, _ = _device_blend(tiles, dst, rows, cols, w, box, acc0, wsum0)
    reached = _check_blend((acc[0], wsum[0]), tiles, dst, rows, cols, w, box, acc0, wsum0, "corner")
    assert reached.sum() == 4 * 4 - 2 and np.isnan(acc0[~reached]).any()        # rows 36-39 x columns 19-22 less two corners


def _check_stats(stats, tiles, what):
    """The device's statistics against tile_stats_kernel's order restated: within 4 ulps; reports whether bit-equal."""
    n, fields = tiles.shape[:2]
    ref = np.array([R.device_tile_stats(tiles[t, f]) for t in range(n) for f in range(fields)])
    assert np.array_equal(np.isnan(stats), np.isnan(ref)), (what, stats, ref)
    inf = np.isinf(ref)
    assert np.array_equal(stats[inf], ref[inf]), what
    ok = np.isfinite(ref)
    u = int(_ulps64(stats[ok], ref[ok]).max())
    print(f"{what}: stats " + ("bit-equal to the restatement" if u == 0 else f"within {u} ulp of the restatement"))
    assert u <= 4, (what, u)
    return ref


@pytest.mark.parametrize("name", sorted(PC.regularise_cases()))
def test_regularised_blend(name):
    tiles, reg = PC.regularise_cases()[name]
    n, fields, tile = tiles.shape[0], tiles.shape[1], tiles.shape[-1]
    rows, cols = 40, 23
    rng = np.random.Generator(np.random.PCG64(n + tile))
    dst = np.stack([rng.integers(-tile // 2, rows - tile // 2, n), rng.integers(-tile // 2, cols - tile // 2, n)], 1)
    w = _weights(tile, "map")
    box = (0, 0, rows, cols)
    acc0, wsum0 = _prior((fields, rows, cols), 300 + tile)
    acc, wsum, stats = _device_blend(tiles, dst, rows, cols, w, box, acc0, wsum0, reg=reg, batches=[2, n - 2])
    restated = _check_stats(stats, tiles, name)
    plain = _device_blend(tiles, dst, rows, cols, w, box, acc0, wsum0)
    assert (plain[2] == CANARY).all()                              # regularise = 0: stats is not written
    masked = False
    for f in range(fields):
        for st in (stats.reshape(n, fields, 2)[:, f], restated.reshape(n, fields, 2)[:, f]):
            _check_blend((acc[f], wsum[f]), tiles[:, f], dst, rows, cols, w, box, acc0[f], wsum0[f], (name, f), st, reg)
        masked |= not np.array_equal(_bits(wsum[f]), _bits(plain[1][f]))
    assert masked                                                  # some weight was taken out


def test_blend_fields_planes_and_stats_rows():
    """fields = 3 on a plane that is not square: plane f at f * rows * cols, stats row t * fields + f (checked against
    bp_plane_blend on each field's tiles alone), and fields = 300 for the grid's y axis."""
    rows, cols, tile = 40, 23, 17
    tiles, reg = PC.regularise_cases()["fields3"]
    n = len(tiles)
    dst = _overhanging(rows, cols, tile)[:n]
    w = _weights(tile, "map")
    box = (2, 1, rows, cols - 3)
    acc0, wsum0 = _prior((3, rows, cols), 9)
    for r in (None, reg):
        acc, wsum, stats = _device_blend(tiles, dst, rows, cols, w, box, acc0, wsum0, reg=r)
        for f in range(3):
            a1, w1, s1 = _device_blend(np.ascontiguousarray(tiles[:, f]), dst, rows, cols, w, box, acc0[f], wsum0[f], reg=r)
            assert np.array_equal(_bits(a1[0]), _bits(acc[f])) and np.array_equal(_bits(w1[0]), _bits(wsum[f])), (r, f)
            assert np.array_equal(_bits(s1), _bits(stats.reshape(n, 3, 2)[:, f])), (r, f)
    rows, cols, tile, fields, n = 23, 40, 2, 300, 6
    tiles = PC.wide_tiles((n, fields, tile, tile), 10)
    dst = np.asarray([(-1, -1), (22, 39), (5, 5), (5, 6), (6, 5), (5, 5)], np.int32)
    w = _weights(tile, "random")
    acc0, wsum0 = _prior((fields, rows, cols), 11)
    acc, wsum, _ = _device_blend(tiles, dst, rows, cols, w, (0, 0, rows, cols), acc0, wsum0)
    for f in range(fields):
        _check_blend((acc[f], wsum[f]), tiles[:, f], dst, rows, cols, w, (0, 0, rows, cols), acc0[f], wsum0[f], ("F300", f))


@pytest.mark.parametrize("use_fields", [False, True])
def test_blend_return_codes_leave_everything_untouched(use_fields):
    rows, cols, tile, n = 23, 40, 3, 4
    tiles = PC.regularise_cases()["after_refusal"][0]
    dst = np.asarray([(0, 0), (5, 5), (20, 37), (-1, 4)], np.int32)
    acc0, wsum0 = _prior((1, rows, cols), 13)
    b = _Blend(tiles, dst, rows, cols, _weights(tile, "map"), acc0, wsum0)
    box = (0, 0, rows, cols)

    def refused(code, box=box, reg=None, **over):
        assert b.call(box, reg, use_fields, **over) == code, (code, box, reg, over)
        acc, wsum, stats = b.result()
        assert np.array_equal(_bits(acc), _bits(acc0)) and np.array_equal(_bits(wsum), _bits(wsum0)), (box, reg, over)
        assert (stats == CANARY).all(), (box, reg, over)

    for reg in (None, 1.5):
        for null in ("tiles", "dst", "weight", "acc", "wsum"):
            refused(EINVAL, reg=reg, **{null: None})
        for name in ("n", "tile", "rows", "cols") + (("fields",) if use_fields else ()):
            for v in (0, -1):
                refused(EINVAL, reg=reg, **{name: v})
        for bad in ((-1, 0, rows, cols), (0, -1, rows, cols), (0, 0, rows + 1, cols), (0, 0, rows, cols + 1),
                    (5, 5, 5, 9), (5, 5, 9, 5), (9, 5, 5, 9), (5, 9, 9, 5), (0, 0, cols, cols)):
            refused(EINVAL, box=bad, reg=reg)
        refused(EUNSUPPORTED, reg=reg, rows=65536, cols=32768, box=(0, 0, 1, 1))
        refused(EUNSUPPORTED, reg=reg, n=2 ** 31 // 64 ** 2, tile=64)
        if use_fields:
            refused(EUNSUPPORTED, reg=reg, fields=65536)
            refused(EUNSUPPORTED, reg=reg, fields=32768, n=16, tile=64)
    refused(EINVAL, reg=1.5, stats=None)
    refused(EINVAL, reg=1.5, stats=None, rows=65536, cols=32768, box=(0, 0, 1, 1))       # BP_EINVAL comes first
    # and the object still works
    assert b.call(box, 1.5, use_fields) == OK
    acc, wsum, stats = b.result()
    _check_blend((acc[0], wsum[0]), tiles[:, 0], dst, rows, cols, _weights(tile, "map"), box, acc0[0], wsum0[0], "after",
                 stats, 1.5)


# ------------------------------------------------------------------------------------------------------- finish

def _finish_inputs(count, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    acc, wsum = rng.standard_normal(count) * np.exp(6 * rng.standard_normal(count)), rng.random(count) * 3 + 1e-3
    special = [(0.0, 0.0), (2.5, 0.0), (-2.5, 0.0), (np.nan, 1.0), (1.0, np.nan), (-0.0, 2.0), (3.0, -0.0), (np.inf, 2.0),
               (1e308, 1e-3), (1e-308, 3.0)]
    where = rng.permutation(count)[:len(special)]
    for k, (a, s) in zip(where, special):                          # (count = 1 takes the first: 0 / 0)
        acc[k], wsum[k] = a, s
    return acc, wsum


@pytest.mark.parametrize("count", [1, 255, 256, 257, 40 * 23])
def test_finish_is_the_float64_quotient(count):
    lib = L.load()
    acc, wsum = _finish_inputs(count, count)
    with np.errstate(all="ignore"):
        ref = acc / wsum
    if count > 1:
        assert np.isnan(ref).sum() >= 3 and np.isposinf(ref).any() and np.isneginf(ref).any()
    outs = []
    for _ in range(2):
        a, s, out = _Buf(count, torch.float64, acc), _Buf(count, torch.float64, wsum), _Buf(count, torch.float64)
        assert lib.bp_plane_finish(a.ptr, s.ptr, count, out.ptr, G.stream()) == OK
        outs.append(out.get())
        assert np.array_equal(_bits(a.get()), _bits(acc)) and np.array_equal(_bits(s.get()), _bits(wsum))
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    _same_bits(outs[0], ref, count)
    a, s = _Buf(count, torch.float64, acc), _Buf(count, torch.float64, wsum)            # in place, as the ensembles do
    assert lib.bp_plane_finish(a.ptr, s.ptr, count, a.ptr, G.stream()) == OK
    assert np.array_equal(_bits(a.get()), _bits(outs[0])) and np.array_equal(_bits(s.get()), _bits(wsum))


def test_finish_return_codes_leave_everything_untouched():
    lib = L.load()
    acc, wsum = _finish_inputs(300, 1)
    a, s, out = _Buf(300, torch.float64, acc), _Buf(300, torch.float64, wsum), _Buf(300, torch.float64)
    for args in ((None, s.ptr, 300, out.ptr), (a.ptr, None, 300, out.ptr), (a.ptr, s.ptr, 300, None),
                 (a.ptr, s.ptr, 0, out.ptr), (a.ptr, s.ptr, -1, out.ptr), (a.ptr, s.ptr, -2 ** 40, out.ptr),
                 (a.ptr, s.ptr, 0, a.ptr)):
        assert lib.bp_plane_finish(*args, G.stream()) == EINVAL, args
        assert out.untouched()
        assert np.array_equal(_bits(a.get()), _bits(acc)) and np.array_equal(_bits(s.get()), _bits(wsum))
