"""GPU: the two kernels of painters with several label fields against the single-field entry points they restate --
``bp_paint_store_fields`` against ``bp_paint_store_mode`` / ``bp_paint_store_scales_mode`` on channel-slice views, and
``bp_plane_blend_fields`` against ``bp_plane_blend`` on each field's tiles in a contiguous buffer.  Both sides run the
same arithmetic on the same values, so the condition is equal bits (NaNs where the other side has them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gpu_util as G
import range_modes_ref as R
from baryon_painter_amd import _lib as L
from baryon_painter_amd.utils import data_transforms as T

pytestmark = pytest.mark.gpu
N = 3
ZS = np.array(R.Z_CASES)
# field modes such that all six occur at either number of fields
MODE_SETS = {2: [(0, 3), (4, 1), (2, 5)], 3: [(0, 1, 2), (5, 4, 3)]}


def _records(mode_ids):
    """(N, F, 4) records: field j in mode mode_ids[j] with the statistics of one of two fields."""
    cols = []
    for j, m in enumerate(mode_ids):
        name = R.MODES[m]
        inv = T.create_range_compress_transforms({R.FIELD: R.K_SETS[name][j % 2]}, {R.FIELD: name}, eps=R.EPS,
                                                 sqrt_of_mean=bool(j % 2))[1]
        rc = T.device_shift_log(inv, 1, R.FIELD)
        assert rc.mode == m
        cols.append(rc.records(R.stats()[("dm", "pressure")[j % 2]], ZS))
    return np.ascontiguousarray(np.stack(cols, axis=1))


def _head(F, levels, h, w, seed):
    """Activations (N, F * levels, h, w) in [-1.6, 1.6] with every field's edge values -- -1, a value below it, NaN, and
    the float32 neighbours of -1 -- in the first pixels, where a sum over the levels gives exactly them (the other
    levels hold 0 there), as ``range_modes_ref.EDGE`` places them."""
    rng = np.random.Generator(np.random.PCG64([seed, F, levels, h]))
    a = (rng.random((N, F * levels, h, w)) * 3.2 - 1.6).astype(np.float32)
    edge = np.array([-1.0, -1.5, np.nan, np.nextafter(np.float32(-1), np.float32(0)),
                     np.nextafter(np.float32(-1), np.float32(-2))], np.float32)
    for j in range(F):
        a[:, j * levels:(j + 1) * levels, 0, :5] = 0.0
        a[:, j * levels, 0, :5] = edge
    return a


def _pointwise(c, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return G.pointwise(rng.random(c) * 1.5 + 0.25, rng.random(c) - 0.5, rng.random(c) * 0.5)


def _slice_pw(ts, j, levels):
    return L.Pointwise(*(t.data_ptr() + 4 * j * levels for t in ts))


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("h,w", [(8, 12), (16, 16)])
def test_store_fields_equals_the_single_field_stores_on_channel_slices(h, w, F, levels):
    """hw = 96 is no power of two and no multiple of the workgroup's 256 threads, so workgroups straddle planes of
    different modes; hw = 256 takes the shift in the index arithmetic.  The view has cstride > c and coff != 0."""
    lib = L.load()
    c = F * levels
    head = _head(F, levels, h, w, seed=3)
    buf, view = G.to_nhwc(head, cstride=c + 3, coff=2)
    pw_ts, pw = _pointwise(c, seed=5)
    cases = 0
    for mode_ids in MODE_SETS[F]:
        rec = _records(mode_ids)
        rec_d = G.dev(rec, torch.float64)
        modes = (C.c_int32 * F)(*mode_ids)
        for inc in (0, 1):
            for use_pw in (False, True):
                for softplus in (0, 1):
                    got = torch.full((N, F, h, w), 12345.0, device="cuda")
                    assert lib.bp_paint_store_fields(modes, F, levels, inc, C.byref(view), C.byref(pw) if use_pw else None,
                                                     softplus, L.ptr(rec_d), L.ptr(got), G.stream()) == L.BP_OK
                    for j, m in enumerate(mode_ids):
                        sview = L.View(buf.data_ptr(), N, h, w, levels, c + 3, 2 + j * levels)
                        spw = _slice_pw(pw_ts, j, levels)
                        rec_j = G.dev(rec[:, j], torch.float64)
                        ref = torch.full((N, 1, h, w), 54321.0, device="cuda")
                        pwp = C.byref(spw) if use_pw else None
                        if levels == 1:
                            code = lib.bp_paint_store_mode(m, C.byref(sview), pwp, softplus, L.ptr(rec_j), L.ptr(ref),
                                                           G.stream())
                        else:
                            code = lib.bp_paint_store_scales_mode(m, C.byref(sview), pwp, softplus, inc, L.ptr(rec_j),
                                                                  L.ptr(ref), G.stream())
                        torch.cuda.synchronize()
                        assert code == L.BP_OK
                        a, b = got[:, j].cpu().numpy(), ref[:, 0].cpu().numpy()
                        assert np.array_equal(a, b, equal_nan=True), (mode_ids, j, inc, use_pw, softplus)
                        assert not (b == 54321.0).any()
                    cases += 1
    assert cases == len(MODE_SETS[F]) * 8
    assert bool((buf[..., :2] == 7.5).all()) and bool((buf[..., 2 + c:] == 7.5).all())       # the view was only read


def test_store_fields_return_codes_leave_the_destination_untouched():
    """One case per code of include/bp_hip.h, each before anything is written."""
    lib = L.load()
    F, levels, h, w = 2, 3, 8, 12
    c = F * levels
    buf, view = G.to_nhwc(_head(F, levels, h, w, seed=4))
    rec_d = G.dev(_records((1, 4)), torch.float64)
    dst = torch.full((N, F, h, w), float("nan"), device="cuda")
    ok = (C.c_int32 * 2)(1, 4)

    def call(modes=ok, fields=F, lv=levels, v=view, rec=rec_d, out=dst):
        return lib.bp_paint_store_fields(modes, fields, lv, 0, C.byref(v) if v is not None else None, None, 0, L.ptr(rec),
                                         L.ptr(out), G.stream())
    # BP_EINVAL: a null pointer, a malformed view
    assert call(modes=None) == call(v=None) == call(rec=None) == call(out=None) == L.BP_EINVAL
    assert call(v=L.View(buf.data_ptr(), N, h, w, c, c - 1, 0)) == L.BP_EINVAL
    # ... src->c != fields * levels
    assert call(fields=3) == call(lv=2) == L.BP_EINVAL
    # ... a mode outside 0 ... 5
    assert call(modes=(C.c_int32 * 2)(1, 6)) == call(modes=(C.c_int32 * 2)(-1, 0)) == L.BP_EINVAL
    # ... fields < 1, levels < 1
    assert call(fields=0) == call(fields=-2) == call(lv=0) == L.BP_EINVAL
    # BP_EUNSUPPORTED: a bf16 view
    half = torch.zeros((N, h, w, c), dtype=torch.bfloat16, device="cuda")
    assert call(v=L.View(half.data_ptr(), N, h, w, c, c, 0, L.BF16)) == L.BP_EUNSUPPORTED
    # ... more than 16 levels (a view of 2 x 17 channels), more than 64 fields (65 x 1)
    wide = torch.zeros((1, 2, 2, 65), device="cuda")
    many = (C.c_int32 * 65)(*([0] * 65))
    rec_w = torch.ones((1, 65, 4), dtype=torch.float64, device="cuda")
    assert call(v=L.View(wide.data_ptr(), 1, 2, 2, 34, 65, 0), lv=17, rec=rec_w) == L.BP_EUNSUPPORTED
    assert call(v=L.View(wide.data_ptr(), 1, 2, 2, 65, 65, 0), modes=many, fields=65, lv=1, rec=rec_w) == L.BP_EUNSUPPORTED
    # ... n * H * W * c = 2^31 (the geometry alone: nothing is launched)
    big = L.View(buf.data_ptr(), 1 << 14, 1 << 8, 1 << 8, 2, 2, 0)
    assert call(v=big, fields=2, lv=1) == L.BP_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all()) and bool((half == 0).all())


# ---------------------------------------------------------------------------------------------------- the blend
TILE, PLANE, FB = 8, 20, 2
ORIGINS = np.array([(1, 2), (5, 6), (9, 3), (4, 10), (10, 10)], np.int32)        # 5 overlapping tiles, none at the border


@pytest.mark.parametrize("regularise_std", [None, 1.0])
@pytest.mark.parametrize("box", ["of the tiles", "cropped"])
def test_blend_fields_equals_the_single_field_blend_per_field(regularise_std, box):
    """5 tiles of 8^2 in a 20 x 20 plane, two fields; the bounding box of the tiles is smaller than the plane, the
    cropped one cuts through tiles (their pixels outside it are not blended).  The accumulators start from seeded
    values on both sides; both sides take the tile statistics from the same device reduction."""
    lib = L.load()
    n = len(ORIGINS)
    rng = np.random.Generator(np.random.PCG64(17))
    tiles = np.exp(rng.standard_normal((n, FB, TILE, TILE))).astype(np.float32)
    tiles[:, 1] *= np.float32(40.0)
    weight = G.dev(rng.random((TILE, TILE)) + 0.1, torch.float64)
    start = rng.random((2, FB, PLANE, PLANE))
    bx0, by0 = int(ORIGINS[:, 0].min()), int(ORIGINS[:, 1].min())
    bx1, by1 = int(ORIGINS[:, 0].max()) + TILE, int(ORIGINS[:, 1].max()) + TILE
    assert (bx0, by0) != (0, 0) and bx1 < PLANE and by1 < PLANE
    if box == "cropped":
        bx0, by0, bx1, by1 = bx0 + 3, by0 + 2, bx1 - 4, by1 - 1
    reg, thr = (1, float(regularise_std)) if regularise_std is not None else (0, 0.0)
    dst_d = torch.from_numpy(ORIGINS).cuda()
    td = G.dev(tiles)
    acc, wsum = G.dev(start[0], torch.float64), G.dev(start[1], torch.float64)
    stats = torch.full((2 * n * FB,), float("nan"), dtype=torch.float64, device="cuda")
    assert lib.bp_plane_blend_fields(L.ptr(td), n, FB, TILE, L.ptr(dst_d), bx0, by0, bx1, by1, L.ptr(weight), reg, thr,
                                     L.ptr(stats), L.ptr(acc), L.ptr(wsum), PLANE, PLANE, G.stream()) == L.BP_OK
    torch.cuda.synchronize()
    dropped = 0
    for f in range(FB):
        tf = td[:, f].contiguous()
        acc_f, wsum_f = G.dev(start[0, f], torch.float64), G.dev(start[1, f], torch.float64)
        stats_f = torch.full((2 * n,), float("nan"), dtype=torch.float64, device="cuda")
        assert lib.bp_plane_blend(L.ptr(tf), n, TILE, L.ptr(dst_d), bx0, by0, bx1, by1, L.ptr(weight), reg, thr,
                                  L.ptr(stats_f), L.ptr(acc_f), L.ptr(wsum_f), PLANE, PLANE, G.stream()) == L.BP_OK
        torch.cuda.synchronize()
        assert torch.equal(acc[f], acc_f) and torch.equal(wsum[f], wsum_f)
        outside = torch.ones((PLANE, PLANE), dtype=torch.bool, device="cuda")
        outside[bx0:bx1, by0:by1] = False
        assert torch.equal(acc[f][outside], G.dev(start[0, f], torch.float64)[outside])
        assert bool((acc[f][~outside] != G.dev(start[0, f], torch.float64)[~outside]).any())
        if reg:
            assert torch.equal(stats.view(n, FB, 2)[:, f].reshape(-1), stats_f)
            t64 = tiles[:, f].astype(np.float64)
            dropped += int((np.abs(t64 - t64.mean(axis=(1, 2), keepdims=True)) >
                            t64.std(axis=(1, 2), keepdims=True) * thr).sum())
        else:
            assert bool(torch.isnan(stats).all())
    assert dropped > 0 if reg else dropped == 0
    # finish over all planes at once
    out = torch.empty((FB, PLANE, PLANE), dtype=torch.float64, device="cuda")
    assert lib.bp_plane_finish(L.ptr(acc), L.ptr(wsum), FB * PLANE * PLANE, L.ptr(out), G.stream()) == L.BP_OK
    torch.cuda.synchronize()
    assert torch.equal(out, acc / wsum)


def test_blend_fields_return_codes():
    lib = L.load()
    n = len(ORIGINS)
    td = torch.ones((n, FB, TILE, TILE), device="cuda")
    dst_d = torch.from_numpy(ORIGINS).cuda()
    weight = torch.ones((TILE, TILE), dtype=torch.float64, device="cuda")
    acc = torch.zeros((FB, PLANE, PLANE), dtype=torch.float64, device="cuda")
    wsum = torch.zeros_like(acc)

    def call(fields=FB, tiles=td, bx1=18, stats=None, reg=0):
        return lib.bp_plane_blend_fields(L.ptr(tiles), n, fields, TILE, L.ptr(dst_d), 1, 2, bx1, 18, L.ptr(weight), reg, 1.0,
                                         L.ptr(stats), L.ptr(acc), L.ptr(wsum), PLANE, PLANE, G.stream())
    assert call(fields=0) == call(tiles=None) == call(bx1=PLANE + 1) == call(reg=1) == L.BP_EINVAL
    assert call(fields=65536) == L.BP_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((acc == 0).all()) and bool((wsum == 0).all())
    assert call() == L.BP_OK
    torch.cuda.synchronize()
    assert bool((wsum[:, 1:18, 2:18] > 0).any())
