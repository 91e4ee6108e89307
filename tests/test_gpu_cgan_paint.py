"""GPU: the CGAN on the device paint path -- bp_paint_load_cam / bp_paint_store_cam against the float64 restatement
(tests/cgan_paint_ref.py), the inference plan against the training plan's eval forward, and CGANPainter.paint_batch /
paint_stream / device planes / light cones against per-tile paint() and against the host paths."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

import cgan_paint_ref as R
import gpu_util as G
from baryon_painter_amd import _lib as L
from baryon_painter_amd import lightcone as LC
from baryon_painter_amd.utils import datasets as D

pytestmark = pytest.mark.gpu

NAN = float("nan")
TILE = 64
# inside the tabulated range (0 .. 2), on its knots, and clamped at either end
REDSHIFTS = np.array([-0.2, 0.0, 0.06, 0.125, 0.3, 0.77, 1.0, 1.6, 2.0, 2.5, 3.1])


# ------------------------------------------------------------------------------------------------------- kernels
def _xf(rng, n, order):
    sig, k0, k1 = rng.uniform(0.3, 3.0, n), np.full(n, 4.0), np.full(n, 1.0)
    sig[0] = 1.0
    cols = {"s": sig, "0": k0, "1": k1}
    return np.stack([cols[c] for c in order], axis=1)


def _untouched(buf, c, coff):
    keep = np.ones(buf.shape[-1], bool)
    keep[coff:coff + c] = False
    assert torch.isnan(buf[..., torch.from_numpy(keep).cuda()]).all(), "stores outside the view"


@pytest.mark.parametrize("coff", [0, 1])
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 64, 64)], ids=["ragged", "tile"])
def test_load_kernel(shape, coff):
    """out = (float) (log((double) raw / sigma + 1) / k0 - k1): a double logarithm (which may differ from NumPy's in the
    last bit of the double) and ONE rounding to float32, so every value is within one float32 ulp of the rounded
    reference and all but a handful are equal; the aux planes are copies."""
    lib, st = L.load(), G.stream()
    n, h, w = shape
    rng = np.random.default_rng(n * 100 + h + coff)
    raw = (10.0 ** rng.uniform(-3, 2, (n, 1, h, w))).astype(np.float32)
    raw[0, 0, 0, :3] = [0.0, 1e-30, 3e4]
    xf = _xf(rng, n, "s01")
    aux = rng.uniform(-1.2, 2.1, (n, 1)).astype(np.float32)
    ref = R.load(raw, xf, aux).astype(np.float32)
    ob, ov = G.empty_nhwc(n, h, w, 2, cstride=4, coff=coff)
    rd, xd, ad = G.dev(raw), G.dev(xf, torch.float64), G.dev(aux)
    L.check(lib.bp_paint_load_cam(L.ptr(rd), 1, L.ptr(xd), L.ptr(ad), 1, C.byref(ov), st), "paint_load_cam")
    got = ob[..., coff:coff + 2].cpu().numpy()
    d = R.ulps32(got[..., 0], ref[..., 0])
    print(f"load {shape} coff {coff}: max {d.max()} ulp, {100 * (d == 0).mean():.3f} % equal")
    assert d.max() <= 1 and (d == 0).mean() >= 0.999
    assert np.array_equal(got[..., 1], ref[..., 1])
    _untouched(ob, 2, coff)


def _device_tanh(src_nhwc):
    """bp_unary_forward(kind 1) of an (n, h, w, 1) array: the generator head's own float32 tanh."""
    lib = L.load()
    n, h, w, _ = src_nhwc.shape
    sb = G.dev(src_nhwc)
    ob = torch.empty_like(sb)
    sv, ov = L.View(sb.data_ptr(), n, h, w, 1, 1, 0, L.F32), L.View(ob.data_ptr(), n, h, w, 1, 1, 0, L.F32)
    L.check(lib.bp_unary_forward(C.byref(sv), None, 1, C.byref(ov), G.stream()), "tanh")
    return ob.cpu().numpy()


@pytest.mark.parametrize("coff", [0, 1])
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 64, 64)], ids=["ragged", "tile"])
def test_store_kernel(shape, coff):
    """dst = (float) ((exp(((double) tanhf(s) + k1) * k0) - 1) * sigma).

    Against the float64 expression on np.tanh(s): with t = tanh(s) and r(t) = (exp((t + k1) k0) - 1) sigma,
    dr/dt = k0 sigma exp((t + k1) k0) = k0 sigma e.  The float32 tanhf is allowed 4 ulp of float32 at t (the limit
    tests/test_gpu_pointwise.py holds bp_unary_forward's tanh to), which the exponential passes on as
    k0 sigma e * 4 ulp32(t) (the second-order term, a factor exp(k0 * 4 ulp32) - 1 < 2e-6 of that, rides on the 1e-5
    margin); the double arithmetic behind it (one exp, three operations: <= 4 * 2^-52 of sigma e) and the single rounding
    of the result to float32 (<= ulp32(r) / 2, taken as a whole ulp) complete the bound:
        |dst - r| <= 4 k0 sigma e ulp32(t) (1 + 1e-5) + 2^-50 sigma e + ulp32(r).
    Against the same expression on the DEVICE's tanh (bp_unary_forward's output, a float32), the transform alone is
    left: the same double value up to libm's exp, rounded once -- within one float32 ulp."""
    lib, st = L.load(), G.stream()
    n, h, w = shape
    rng = np.random.default_rng(n * 100 + h + coff + 1)
    src = rng.uniform(-4.0, 4.0, (n, h, w, 1)).astype(np.float32)
    src[0, 0, :3, 0] = [-4.0, 0.0, 4.0]
    xf = _xf(rng, n, "01s")
    sb, sv = G.to_nhwc(np.ascontiguousarray(src.transpose(0, 3, 1, 2)), cstride=4, coff=coff)
    dst = torch.full((n, 1, h, w), NAN, device="cuda")
    xd = G.dev(xf, torch.float64)
    L.check(lib.bp_paint_store_cam(C.byref(sv), L.ptr(xd), L.ptr(dst), st), "paint_store_cam")
    got = dst.cpu().numpy()
    assert np.isfinite(got).all()
    t = np.tanh(src.astype(np.float64))
    ref = R.store(t, xf)
    sig = xf[:, 2, None, None, None]
    e = (ref / sig + 1.0)                                                # exp((t + k1) k0), NCHW
    tol = 4 * 4.0 * sig * e * R.ulp32(t).transpose(0, 3, 1, 2) * (1 + 1e-5) + 2.0 ** -50 * sig * e + R.ulp32(ref)
    err = np.abs(got - ref)
    print(f"store {shape} coff {coff}: worst error / bound vs np.tanh {np.max(err / tol):.3f}")
    assert (err <= tol).all(), np.max(err / tol)
    ref_dev = R.store(_device_tanh(src), xf).astype(np.float32)
    d = R.ulps32(got, ref_dev)
    print(f"store {shape} coff {coff}: max {d.max()} ulp vs the device tanh, {100 * (d == 0).mean():.3f} % equal")
    assert d.max() <= 1


def test_kernel_refusals_write_nothing():
    lib, st = L.load(), G.stream()
    n, h, w = 2, 5, 7
    raw = torch.ones((n, 1, h, w), device="cuda")
    xf = torch.ones((n, 3), dtype=torch.float64, device="cuda")
    aux = torch.zeros((n, 1), device="cuda")
    ob, ov = G.empty_nhwc(n, h, w, 2, cstride=4, coff=0)
    bf = torch.full((n, h, w, 4), NAN, dtype=torch.bfloat16, device="cuda")
    bv = L.View(bf.data_ptr(), n, h, w, 2, 4, 0, L.BF16)
    dst = torch.full((n, 1, h, w), NAN, device="cuda")
    load, store = lib.bp_paint_load_cam, lib.bp_paint_store_cam
    assert load(L.ptr(raw), 1, L.ptr(xf), L.ptr(aux), 1, C.byref(bv), st) == L.BP_EUNSUPPORTED
    assert load(None, 1, L.ptr(xf), L.ptr(aux), 1, C.byref(ov), st) == L.BP_EINVAL
    assert load(L.ptr(raw), 1, None, L.ptr(aux), 1, C.byref(ov), st) == L.BP_EINVAL
    assert load(L.ptr(raw), 1, L.ptr(xf), None, 1, C.byref(ov), st) == L.BP_EINVAL               # caux > 0 without aux
    assert load(L.ptr(raw), 0, L.ptr(xf), L.ptr(aux), 1, C.byref(ov), st) == L.BP_EINVAL         # c < 1
    assert load(L.ptr(raw), 2, L.ptr(xf), L.ptr(aux), 1, C.byref(ov), st) == L.BP_EINVAL         # c + caux != view's
    assert load(L.ptr(raw), 1, L.ptr(xf), L.ptr(aux), 1, None, st) == L.BP_EINVAL
    sb, sv = G.empty_nhwc(n, h, w, 1, cstride=4, coff=1)
    sb.fill_(0.5)
    b1 = L.View(bf.data_ptr(), n, h, w, 1, 4, 1, L.BF16)
    assert store(C.byref(b1), L.ptr(xf), L.ptr(dst), st) == L.BP_EUNSUPPORTED
    assert store(None, L.ptr(xf), L.ptr(dst), st) == L.BP_EINVAL
    assert store(C.byref(sv), None, L.ptr(dst), st) == L.BP_EINVAL
    assert store(C.byref(sv), L.ptr(xf), None, st) == L.BP_EINVAL
    bad = L.View(sb.data_ptr(), n, h, w, 1, 4, 4, L.F32)                                         # coff + c > cstride
    assert store(C.byref(bad), L.ptr(xf), L.ptr(dst), st) == L.BP_EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(ob).all() and torch.isnan(dst).all() and torch.isnan(bf.float()).all()
    # and the accepted calls do write
    L.check(load(L.ptr(raw), 1, L.ptr(xf), L.ptr(aux), 1, C.byref(ov), st), "load")
    L.check(store(C.byref(sv), L.ptr(xf), L.ptr(dst), st), "store")
    assert torch.isfinite(ob[..., :2]).all() and torch.isfinite(dst).all()


# ------------------------------------------------------------------------------------------------------- painters
@pytest.fixture(scope="module")
def painters(tmp_path_factory):
    """A 64^2, one-block CGAN painter trained for two iterations (batch-norm running statistics and spectral-norm
    state off their initial values), the same painter restored from its (state, meta) checkpoint, 11 distinct raw
    tiles and their redshifts."""
    from baryon_painter_amd.painter import CGANPainter
    torch.manual_seed(4)
    ds = D.SyntheticTileDataset(n_sample=16, tile_size=TILE, seed=3)
    p = CGANPainter(training_data_set=ds, tile_size=TILE, compute_device="cuda:0", n_res=1)
    p.train(n_iter=2, batch_size=2)
    d = tmp_path_factory.mktemp("cgan_ckpt")
    files = (str(d / "state"), str(d / "meta"))
    p.save_state_to_file(files)
    p.checkpoint_dir = str(d)
    q = CGANPainter(filename=files, compute_device="cuda:0", tile_size=512, n_res=9)      # (geometry: the checkpoint's)
    tiles = np.stack([ds.raw_fields(i)[0] for i in range(len(REDSHIFTS))])
    assert tiles.dtype == np.float32 and len({t.tobytes() for t in tiles}) == len(tiles)
    return p, q, tiles, REDSHIFTS


@pytest.fixture(scope="module")
def per_tile(painters):
    """paint(tile, z) tile by tile, float64: the reference of the stream, batch and checkpoint tests (computed once)."""
    p, q, tiles, zs = painters
    return np.stack([np.asarray(p.paint(t, z=float(z)), np.float64) for t, z in zip(tiles, zs)])


def _within_3e7(out, ref):
    # same network bits; host: the float64 inverse transform; device: the same value rounded to float32 (exp may
    # differ in the last bit of the double)
    for i in range(len(ref)):
        tol = 3e-7 * np.abs(ref[i]).max()
        err = np.abs(np.asarray(out[i], np.float64) - ref[i]).max()
        assert err <= tol, (i, err, tol)


@pytest.mark.parametrize("n", [1, 4])
def test_eval_generate_is_the_training_plans_eval_forward(painters, n):
    """generate() in eval mode runs the inference plan; its values are those of the path it replaces: a _GanPlan driven
    directly (plan.generate(y, zc, False) + bp_view_to_nchw of the fake half's pressure channel)."""
    from baryon_painter_amd.models.cgan import _GanPlan
    p, q, tiles, zs = painters
    m = p.model
    y = np.stack([p.transform(t, "dm", float(z)) for t, z in zip(tiles[:n], zs[:n])])[:, None]
    z = torch.tensor(zs[:n], dtype=torch.float32)
    m.train(False)
    had = n in m._plans
    got = m.generate(torch.from_numpy(y), z)
    assert n in m._paint_plans and (n in m._plans) == had            # (no training plan is built for it)
    with torch.no_grad():
        yd, zc = m._inputs(torch.from_numpy(y), z)
        plan = _GanPlan(m, n)
        plan.generate(yd, zc, False)
        ref = torch.empty((n, 1, TILE, TILE), device="cuda")
        L.check(m._lib.bp_view_to_nchw(C.byref(plan.v_fake_x), None, 0, L.ptr(ref), G.stream()), "fake layout")
    assert got.shape == ref.shape and float(got.abs().max()) <= 1.0 and float(got.std()) > 0
    assert torch.equal(got, ref)
    assert torch.equal(m.generate(torch.from_numpy(y), z), ref)      # (and again, from the cached plan)


def test_paint_stream_equals_per_tile_paint(painters, per_tile):
    p, q, tiles, zs = painters
    out = p.paint_stream(tiles, zs, batch_size=4)
    assert out.shape == tiles.shape and out.dtype == np.float32 and np.isfinite(out).all()
    _within_3e7(out, per_tile)
    assert len({o.tobytes() for o in out}) == len(out)
    with pytest.raises(ValueError):
        p.paint_stream(tiles[:, :32], zs)


def test_paint_stream_is_independent_of_batching_sharding_and_seed(painters):
    p, q, tiles, zs = painters
    ref = p.paint_stream(tiles, zs, batch_size=4, seed=7)
    assert np.array_equal(p.paint_stream(tiles, zs, batch_size=11, seed=7), ref)
    assert np.array_equal(p.paint_stream(tiles, zs, batch_size=3, seed=7), ref)
    for world in (2, 3):
        parts = [p.paint_stream(tiles, zs, batch_size=4, seed=7, rank=r, world_size=world) for r in range(world)]
        assert parts[0][1][0] == 0 and parts[-1][1][1] == len(tiles)
        assert all(a[1][1] == b[1][0] for a, b in zip(parts, parts[1:]))
        assert np.array_equal(np.concatenate([a[0] for a in parts]), ref)
    # no latent noise: the seed and the tile ids are accepted and change nothing
    assert np.array_equal(p.paint_stream(tiles, zs, batch_size=4, seed=8), ref)
    assert np.array_equal(p.paint_stream(tiles, zs, batch_size=4, seed=7, tile_ids=np.arange(11)[::-1] + 2 ** 40), ref)
    # pinned torch tensors in and out: no staging copies on the host
    tin = torch.from_numpy(tiles).pin_memory()
    tout = torch.empty(tiles.shape, dtype=torch.float32).pin_memory()
    r = p.paint_stream(tin, zs, batch_size=4, seed=7, out=tout)
    assert r is tout and np.array_equal(tout.numpy(), ref)
    # a scalar redshift is every tile's
    assert np.array_equal(p.paint_stream(tiles[:3], 0.3, batch_size=2), p.paint_stream(tiles[:3], [0.3] * 3, batch_size=3))


def test_paint_batch_equals_per_tile_paint(painters, per_tile):
    p, q, tiles, zs = painters
    out = p.paint_batch(tiles, zs, batch_size=4)                       # 4 + 4 + 3: the last batch is ragged
    assert out.shape == tiles.shape and out.dtype == np.float64
    _within_3e7(out, per_tile)
    raw = p.paint_batch(tiles[:3], zs[:3], inverse_transform=False, batch_size=2)
    assert raw.shape == (3, 1, TILE, TILE) and raw.dtype == np.float32 and np.abs(raw).max() <= 1.0
    assert np.array_equal(raw[0], p.paint(tiles[0], z=float(zs[0]), inverse_transform=False)[0])
    with pytest.raises(ValueError):
        p.paint_batch(tiles[:, :32], zs)


def test_checkpointed_painter_paints_the_same_bits(painters, per_tile):
    p, q, tiles, zs = painters
    assert q is not p and q.model is not p.model and (q.model.tile_size, q.n_res) == (TILE, 1)
    assert q.can_paint_stream(0.3) and q.stats == p.stats
    for i in (0, 5, 10):
        assert np.array_equal(np.asarray(q.paint(tiles[i], z=float(zs[i])), np.float64), per_tile[i])
    assert np.array_equal(q.paint_stream(tiles, zs, batch_size=4), p.paint_stream(tiles, zs, batch_size=4))
    # a bare state dict restores the network, not the statistics: it cannot transform, and says so up front
    from baryon_painter_amd.painter import CGANPainter
    path = os.path.join(p.checkpoint_dir, "bare")
    p.save_state_to_file(path)
    b = CGANPainter(filename=path, tile_size=TILE, n_res=1, compute_device="cuda:0")
    assert b.stats is None and not b.can_paint_stream()
    with pytest.raises(NotImplementedError):
        b.paint_stream(tiles, zs)
    raw = b.paint(p.transform(tiles[0], "dm", 0.0), z=0.0, transform=False, inverse_transform=False)
    assert np.array_equal(raw, p.paint(tiles[0], z=0.0, inverse_transform=False))


def test_inference_plan_is_smaller_than_the_training_plan(painters):
    """n = 4 at 64^2: the inference plan holds the generator's activations and forward weight images; the training plan
    adds the discriminator input (2n x H x W x 4), two discriminator unit sets and every gradient buffer."""
    from baryon_painter_amd.models.cgan import _GanPaintPlan, _GanPlan
    p, q, tiles, zs = painters
    m = p.model
    # Nothing but the two constructors may change the allocator's count between the readings: garbage of earlier tests
    # (reference cycles that hold device tensors) is collected first, and the collector stays off in between -- a
    # collection that ran inside a constructor freed more than the plan allocated.
    gc.collect()
    gc.disable()
    try:
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        a = _GanPaintPlan(m, 4)
        torch.cuda.synchronize()
        m1 = torch.cuda.memory_allocated()
        b = _GanPlan(m, 4)
        torch.cuda.synchronize()
        m2 = torch.cuda.memory_allocated()
    finally:
        gc.enable()
    print(f"inference plan {(m1 - m0) / 2 ** 20:.2f} MiB, training plan {(m2 - m1) / 2 ** 20:.2f} MiB at n = 4, 64^2")
    assert 0 < m1 - m0 < m2 - m1
    assert not hasattr(a, "d_in") and all(u.packed_bwd is None and u.out.grad_buf is None for u in a.units)
    assert b.d_in.buf.shape == (8, TILE, TILE, 4)
    # release_paint_buffers drops the model's inference plans and graphs and the painter's staging buffers
    p.paint_stream(tiles[:4], zs[:4], batch_size=4)
    assert p.model._paint_graphs and "_paint_host_buffers" in p.__dict__
    p.release_paint_buffers()
    assert not p.model._paint_graphs and not p.model._paint_plans and "_paint_host_buffers" not in p.__dict__


# --------------------------------------------------------------------------------------------------------- planes
def _delta(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (np.exp(rng.standard_normal((n, n)) * 0.5) * 0.05).astype(np.float32)


def _smooth_delta(n, seed):
    """A smooth positive periodic plane (the spline resampling of white noise overshoots below -sigma, where the
    transform is NaN on both paths)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    k = np.fft.fftfreq(n) * n
    f = np.fft.ifft2(np.fft.fft2(rng.standard_normal((n, n))) * (np.hypot(k[:, None], k[None, :]) < n / 10)).real
    return (np.exp(f / f.std() * 0.5) * 0.05).astype(np.float32)


def _close(dev, host, rel):
    ok = np.isfinite(host)
    assert np.array_equal(np.isfinite(dev), ok) and ok.mean() > 0.9
    scale = np.abs(host[ok]).max()
    err = np.abs(dev[ok] - host[ok]).max()
    print(f"max |dev - host| = {err:.3e} of {scale:.3e}")
    assert err <= rel * scale, (err, scale)


def test_host_plane_equals_the_per_tile_loop(painters):
    """lightcone.paint_plane with a CGANPainter (through paint_stream) against the reference's serial loop
    (get_tile -> paint -> weight -> accumulate)."""
    p, q, tiles, zs = painters
    delta = _delta(150, 31)
    rel, z = TILE / 150, 0.42
    plane = LC.paint_plane(p, delta, rel, TILE, z, batch_size=4)
    origins, slices = LC.generate_tiling(150, TILE, 0.5)
    acc, wsum = np.zeros((150, 150)), np.zeros((150, 150))
    for j, xs in enumerate(origins):
        for k, ys in enumerate(origins):
            tile = np.asarray(LC.get_tile(delta, (xs, ys), rel), np.float32)
            painted = np.asarray(p.paint(tile, z=z), np.float64)
            w = LC.make_weight_map(tile.shape, falloff=0.05, sigma=0.5)
            acc[slices[j][k]] += w * painted
            wsum[slices[j][k]] += w
    with np.errstate(invalid="ignore"):
        ref = acc / wsum
    ok = np.isfinite(ref)
    assert plane.shape == (150, 150) and np.array_equal(np.isfinite(plane), ok) and ok.mean() > 0.95
    assert np.abs(plane[ok] - ref[ok]).max() <= 1e-6 * np.abs(ref[ok]).max()


def test_device_plane_equals_host_plane(painters):
    p, q, tiles, zs = painters
    delta = _delta(150, 41)
    rel, z = TILE / 150, 0.42
    host = LC.paint_plane(p, delta, rel, TILE, z, seed=5, batch_size=4)
    dev = LC.paint_plane(p, delta, rel, TILE, z, seed=5, batch_size=4, on_device=True)
    assert dev.shape == host.shape == (150, 150) and dev.dtype == np.float64
    ok = np.isfinite(host)
    assert np.array_equal(np.isfinite(dev), ok) and ok.mean() > 0.9
    assert np.array_equal(dev[ok], host[ok]), np.abs(dev[ok] - host[ok]).max()       # cut == tile: the same bits
    # a CUDA tensor is used in place; out= keeps the plane on the device and is what comes back
    out = torch.full((150, 150), 3.0, dtype=torch.float64, device="cuda")
    r = LC.paint_plane(p, torch.from_numpy(delta).cuda(), rel, TILE, z, batch_size=4, on_device=True, out=out)
    assert r is out
    got = out.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(dev)) and np.array_equal(got[ok], dev[ok])
    # regularise_std (float64 statistics on the device, float32 on the host: equal outside the tie band)
    host = LC.paint_plane(p, delta, rel, TILE, z, regularise_std=3)
    dev = LC.paint_plane(p, delta, rel, TILE, z, regularise_std=3, on_device=True)
    _close(dev, host, 1e-5)


def test_device_plane_with_zoom_equals_host_plane(painters):
    pytest.importorskip("scipy.ndimage")              # (the host path zooms with SciPy)
    p, q, tiles, zs = painters
    delta = _smooth_delta(200, 42)
    rel = TILE / 150
    assert LC.plane_geometry(200, rel, TILE)["cut"] == 85
    host = LC.paint_plane(p, delta, rel, TILE, 0.42)
    dev = LC.paint_plane(p, delta, rel, TILE, 0.42, on_device=True)
    _close(dev, host, 1e-5)


def test_light_cone_on_the_device(painters):
    """Two tiled planes (150 pixels, no resampling) and one small plane (32 < 64, from a 256-pixel mass plane) into a
    96-pixel map: the planes of the two paths have the same bits, so the maps differ by the projection alone --
    1e-12 of the largest pixel, the limit of tests/test_gpu_ymap.py."""
    pytest.importorskip("scipy.ndimage")              # (small planes are cut and zoomed with SciPy on either path)
    p, q, tiles, zs = painters
    planes = [(_smooth_delta(256, 43), (0.9, 0.85), 128.0), _delta(150, 46), _delta(150, 47)]
    z, size, scales = [0.05, 0.42, 1.3], [32.0, 150.0, 150.0], [1.5, 0.5, 2.0]
    kw = dict(tile_size=64.0, n_pixel_tile=TILE, resolution=96, batch_size=8, scales=scales)
    host, hp = LC.paint_light_cone(p, planes, z, size, return_planes=True, **kw)
    dev, dp = LC.paint_light_cone(p, iter(planes), z, size, on_device=True, return_planes=True, **kw)
    assert [a.shape for a in dp] == [(32, 32), (150, 150), (150, 150)] and dev.shape == (96, 96)
    for a, b in zip(dp, hp):
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
    assert np.isfinite(dev).all() and np.abs(host).max() > 0
    err, top = np.abs(dev - host).max(), np.abs(host).max()
    print(f"max |y_dev - y_host| = {err:.3e} = {err / top:.3e} of max |y|")
    assert err <= 1e-12 * top, (err, top)


def test_stream_at_512_with_nine_blocks():
    """The fiducial geometry: 512^2 tiles, nine residual blocks, 3 tiles in batches of 2 (one full, one ragged)."""
    from baryon_painter_amd.painter import CGANPainter
    torch.manual_seed(9)
    ds = D.SyntheticTileDataset(n_sample=4, tile_size=512, seed=5)
    p = CGANPainter(training_data_set=ds, tile_size=512, compute_device="cuda:0", n_res=9)
    tiles = np.stack([ds.raw_fields(i)[0] for i in range(3)])
    zs = np.array([0.1, 0.9, 2.4])
    out = p.paint_stream(tiles, zs, batch_size=2)
    assert out.shape == (3, 512, 512) and out.dtype == np.float32 and np.isfinite(out).all()
    _within_3e7(out, [np.asarray(p.paint(t, z=float(z)), np.float64) for t, z in zip(tiles, zs)])
    p.release_paint_buffers()
