"""GPU: the six range-compression modes on every device surface -- the mode-taking load / store entry points against
the host transforms, their split-scale forms against the plain ones pushed through bp_split_scale, the batch assembly
of a ``log`` / ``shift-log-2p`` training set against the host dataset, and painters of two mode pairs on the stream,
checkpoint and light-cone plane paths (on the commit before, such painters answer ``can_paint_stream() == False`` and
``on_device=True`` raises)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gpu_util as G
import host_cases as HC
import range_modes_ref as R
from baryon_painter_amd import _lib as L
from baryon_painter_amd import lightcone as LC
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils import synthetic as syn
from baryon_painter_amd.utils.datasets import BAHAMASDataset, DeviceTileAssembler
from oracle.philox import tile_normals
from test_gpu_assemble import _split_nchw, permutation_indices, tile_dataset

pytestmark = pytest.mark.gpu
ZS = np.array(R.Z_CASES)                     # three tiles, three different records


def _transforms(mode, ki=0, sq=False):
    return T.create_range_compress_transforms({R.FIELD: R.K_SETS[mode][ki]}, {R.FIELD: mode}, eps=R.EPS, sqrt_of_mean=sq)


def _records(mode, direction, ki=0, sq=False):
    rc = T.device_shift_log(_transforms(mode, ki, sq)[direction], direction, R.FIELD)
    return rc, rc.records(R.stats()[R.FIELD], ZS)


def _load(mode_id, raw, rec_d, view, caux=0, aux=None):
    return L.load().bp_paint_load_mode(mode_id, L.ptr(raw), 1, L.ptr(rec_d), L.ptr(aux), caux, C.byref(view), G.stream())


# ---------------------------------------------------------------------------------------------- 1. load / store
@pytest.mark.parametrize("sq", [False, True])
@pytest.mark.parametrize("mode", R.MODES)
def test_load_equals_the_host_transform(mode, sq):
    """Forward: the float64 evaluation rounded once, so within one float32 spacing of the host value (a rounding
    boundary); the branch values (x <= 0, NaN) are constants of the record: equal bits."""
    lib = L.load()
    x = np.stack([R.raw_tile(5), R.raw_tile(6) * np.float32(3), R.raw_tile(7) * np.float32(0.01)])
    rc, rec = _records(mode, 0, sq=sq)
    raw, rec_d = G.dev(x[:, None]), G.dev(rec, torch.float64)
    buf, view = G.empty_nhwc(3, 32, 32, 2, cstride=3, coff=1)
    aux = G.dev(ZS.astype(np.float32)[:, None])
    assert _load(rc.mode, raw, rec_d, view, 1, aux) == L.BP_OK
    buf2a, v2a = G.empty_nhwc(3, 32, 32, 2)
    buf2b, v2b = G.empty_nhwc(3, 32, 32, 2, cstride=4, coff=2)
    assert lib.bp_paint_load2_mode(rc.mode, L.ptr(raw), 1, L.ptr(rec_d), L.ptr(aux), 1, C.byref(v2a), C.byref(v2b),
                                   G.stream()) == L.BP_OK
    torch.cuda.synchronize()
    got = G.from_nhwc(buf, 2, 1)
    assert np.array_equal(G.from_nhwc(buf2a, 2), got, equal_nan=True)
    assert np.array_equal(G.from_nhwc(buf2b, 2, 2), got, equal_nan=True)
    assert bool(torch.isnan(buf[..., 0]).all()) and np.array_equal(got[:, 1], np.broadcast_to(aux.cpu().numpy()[:, :, None],
                                                                                           (3, 32, 32)))
    fwd = _transforms(mode, sq=sq)[0]
    worst = 0.0
    for n in range(3):
        with np.errstate(all="ignore"):
            host = np.asarray(fwd(x[n], R.FIELD, float(ZS[n]), R.stats()), np.float64)
        nan = np.isnan(host)
        assert np.array_equal(np.isnan(got[n, 0]), nan)
        if mode in ("log", "log-tanh", "1/x"):
            branch = ~(x[n] > 0) if mode != "1/x" else ~(x[n].astype(np.float64) / rec[n, 0] > -1)
            assert branch.sum() >= 1 and np.array_equal(got[n, 0][branch], host[branch].astype(np.float32))
        err, tol = np.abs(got[n, 0].astype(np.float64) - host)[~nan], R.forward_tolerance(host)[~nan]
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (n, err.max())
    print(mode, "forward: worst err / (one float32 spacing)", worst)


def _store(mode_id, y, rec, softplus=0):
    buf, view = G.to_nhwc(y[:, None], cstride=3, coff=1)
    dst = torch.full((y.shape[0], 1, *y.shape[1:]), float("nan"), device="cuda")
    rc = L.load().bp_paint_store_mode(mode_id, C.byref(view), None, softplus, L.ptr(G.dev(rec, torch.float64)), L.ptr(dst),
                                      G.stream())
    torch.cuda.synchronize()
    return rc, dst.cpu().numpy()[:, 0]


INVERSE_ERRORS = {}


@pytest.mark.parametrize("mode", R.MODES)
def test_store_equals_the_host_inverse(mode):
    """Inverse: the host float32 path's worst relative error against the formula evaluated in float64 is the
    reference's own error; the device is allowed max(1 float32 ulp, 4 x that) -- HIP's float32 functions are specified
    to 1-2 ulp and pass through the same conditioning as the host's.  Edge values (y = -1, y < -1, NaN): exact."""
    k = R.K_SETS[mode][0]
    y = np.stack([R.activation_tile(mode, k, seed=s) for s in (6, 7, 8)])
    rc, rec = _records(mode, 1, sq=True)
    code, got = _store(rc.mode, y, rec)
    assert code == L.BP_OK
    inv = _transforms(mode, sq=True)[1]
    host_rel = dev_rel = 0.0
    body = np.ones((32, 32), bool)
    body[R.EDGE] = False
    for n in range(3):
        s = T.interpolate_z(R.stats()[R.FIELD], float(ZS[n]))
        with np.errstate(all="ignore"):
            host = np.asarray(inv(y[n], R.FIELD, float(ZS[n]), R.stats()))
            exact = R.inverse_f64(mode, k, np.sqrt(s["var"]), np.sqrt(s["mean"]), R.EPS, y[n])
        assert host.dtype == np.float64
        # edge values: the branch results of the host, rounded to float32 as everything the kernel stores
        assert np.array_equal(got[n][R.EDGE], host[R.EDGE].astype(np.float32), equal_nan=True), (got[n][R.EDGE], host[R.EDGE])
        assert np.isfinite(exact[body]).all() and (exact[body] != 0).all()
        host_rel = max(host_rel, float((np.abs(host - exact)[body] / np.abs(exact[body])).max()))
        dev_rel = max(dev_rel, float((np.abs(got[n].astype(np.float64) - exact)[body] / np.abs(exact[body])).max()))
    tol = max(2.0 ** -23, 4 * host_rel)
    INVERSE_ERRORS[mode] = (host_rel, dev_rel)
    print(mode, "inverse: host rel err", host_rel, "device rel err", dev_rel, "allowed", tol)
    assert dev_rel <= tol, (mode, dev_rel, tol)


def test_shift_log_mode_is_the_entry_point_without_mode():
    """bp_paint_load / bp_paint_store are the `_mode` forms at shift-log: the same bits from either."""
    lib = L.load()
    x = np.stack([R.raw_tile(5), R.raw_tile(6), R.raw_tile(7)])
    rc, rec = _records("shift-log", 0)
    raw = G.dev(x[:, None])
    b0, v0 = G.empty_nhwc(3, 32, 32, 1)
    b1, v1 = G.empty_nhwc(3, 32, 32, 1)
    assert _load(rc.mode, raw, G.dev(rec, torch.float64), v0) == L.BP_OK
    assert lib.bp_paint_load(L.ptr(raw), 1, L.ptr(G.dev(rec[:, :2], torch.float64)), None, 0, C.byref(v1),
                             G.stream()) == L.BP_OK
    torch.cuda.synchronize()
    assert torch.equal(b0.view(torch.int32), b1.view(torch.int32))
    y = np.stack([R.activation_tile("shift-log", 4.0, seed=s) for s in (6, 7, 8)])
    _, rec = _records("shift-log", 1)
    code, got = _store(rc.mode, y, rec, softplus=1)
    buf, view = G.to_nhwc(y[:, None])
    dst = torch.empty((3, 1, 32, 32), device="cuda")
    assert lib.bp_paint_store(C.byref(view), None, 1, L.ptr(G.dev(rec[:, 1::-1], torch.float64)), L.ptr(dst),
                              G.stream()) == L.BP_OK
    torch.cuda.synchronize()
    assert code == L.BP_OK and np.array_equal(got, dst.cpu().numpy()[:, 0], equal_nan=True)


def test_return_codes_leave_the_destination_untouched():
    lib = L.load()
    x = np.stack([R.raw_tile(5)] * 3)
    _, rec = _records("log", 0)
    raw, rec_d = G.dev(x[:, None]), G.dev(rec, torch.float64)
    for mode_id in (-1, 6, 99):
        buf, view = G.empty_nhwc(3, 32, 32, 1)
        assert _load(mode_id, raw, rec_d, view) == L.BP_EINVAL
        assert lib.bp_paint_load2_mode(mode_id, L.ptr(raw), 1, L.ptr(rec_d), None, 0, C.byref(view), C.byref(view),
                                       G.stream()) == L.BP_EINVAL
        code, got = _store(mode_id, x, rec)
        torch.cuda.synchronize()
        assert code == L.BP_EINVAL and np.isnan(got).all() and bool(torch.isnan(buf).all())
    buf, view = G.empty_nhwc(3, 32, 32, 1)
    assert _load(1, raw, None, view) == L.BP_EINVAL and _load(1, None, rec_d, view) == L.BP_EINVAL
    half = torch.zeros((3, 32, 32, 1), dtype=torch.bfloat16, device="cuda")
    bview = L.View(half.data_ptr(), 3, 32, 32, 1, 1, 0, L.BF16)
    dst = torch.full((3, 1, 32, 32), float("nan"), device="cuda")
    assert _load(1, raw, rec_d, bview) == L.BP_EUNSUPPORTED
    assert lib.bp_paint_store_mode(1, C.byref(bview), None, 0, L.ptr(rec_d), L.ptr(dst), G.stream()) == L.BP_EUNSUPPORTED
    assert lib.bp_paint_store_scales_mode(1, C.byref(bview), None, 0, 0, L.ptr(rec_d), L.ptr(dst), G.stream()) == \
        L.BP_EUNSUPPORTED
    assert lib.bp_paint_store_scales_mode(7, C.byref(view), None, 0, 0, L.ptr(rec_d), L.ptr(dst), G.stream()) == L.BP_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all()) and bool((half == 0).all()) and bool(torch.isnan(buf).all())


# ---------------------------------------------------------------------------------------------- 2. split-scale forms
def test_split_scale_forms_equal_the_plain_forms_through_split_scale():
    """One mode, 64^2 tiles, n_scale = 3 at step 4 (radii 6 and 24: the coarse level's halo reaches 24 rows past the
    edge, through the reflection), with and without the original: bit for bit."""
    lib = L.load()
    mode, n, t, n_scale = "log-tanh", 3, 64, 3
    rng = np.random.Generator(np.random.PCG64(12))
    x = np.exp(rng.random((n, t, t)) * 9.0 - 6.0).astype(np.float32)
    x[0, 0, :3] = (0.0, -1.0, np.float32(1e-3))
    rc, rec = _records(mode, 0)
    raw, rec_d = G.dev(x[:, None]), G.dev(rec, torch.float64)
    radii, w = T.split_scale_tables(n_scale, 4, 3.0)
    assert radii[2] == 24
    wd, rad = G.dev(w, torch.float64), (C.c_int32 * len(radii))(*radii)
    ws = int(lib.bp_split_scale_workspace(n, t, t))
    scratch = torch.empty(ws // 4, device="cuda")
    vbuf, vview = G.empty_nhwc(n, t, t, 1)
    assert _load(rc.mode, raw, rec_d, vview) == L.BP_OK
    v = vbuf[..., 0].contiguous()
    aux = G.dev(ZS.astype(np.float32)[:, None])
    _, rec_out = _records(mode, 1)
    rec_out_d = G.dev(rec_out, torch.float64)
    for inc in (0, 1):
        levels = n_scale + inc
        ref_buf, ref_view = G.empty_nhwc(n, t, t, levels)
        assert lib.bp_split_scale(L.ptr(v), n, t, t, n_scale, inc, L.ptr(wd), rad, L.ptr(scratch), ws, C.byref(ref_view),
                                  G.stream()) == L.BP_OK
        b0, v0 = G.empty_nhwc(n, t, t, levels + 1)
        b1, v1 = G.empty_nhwc(n, t, t, levels + 1, cstride=levels + 3, coff=2)
        assert lib.bp_paint_load_scales2_mode(rc.mode, L.ptr(raw), L.ptr(rec_d), L.ptr(aux), 1, n_scale, inc, L.ptr(wd),
                                              rad, L.ptr(scratch), ws, C.byref(v0), C.byref(v1), G.stream()) == L.BP_OK
        torch.cuda.synchronize()
        assert torch.equal(b0[..., :levels], ref_buf) and torch.equal(b1[..., 2:2 + levels], ref_buf)
        assert torch.equal(b0[..., levels], aux[:, 0, None, None].expand(n, t, t))
        # the store: activation per channel, channel 0 or the float32 sum in channel order, then the plain store
        act = (rng.random((n, levels, t, t)) * 0.6 - 0.3).astype(np.float32)
        act[0, :, 0, 0] = -1.0
        sbuf, sview = G.to_nhwc(act)
        got = torch.full((n, 1, t, t), float("nan"), device="cuda")
        assert lib.bp_paint_store_scales_mode(rc.mode, C.byref(sview), None, 0, inc, L.ptr(rec_out_d), L.ptr(got),
                                              G.stream()) == L.BP_OK
        summed = act[:, 0] if inc else (act[:, 0] + act[:, 1]) + act[:, 2]
        code, ref = _store(rc.mode, summed, rec_out)
        torch.cuda.synchronize()
        assert code == L.BP_OK and np.array_equal(got.cpu().numpy()[:, 0], ref, equal_nan=True)
    bad = lib.bp_paint_load_scales2_mode(9, L.ptr(raw), L.ptr(rec_d), L.ptr(aux), 1, n_scale, 1, L.ptr(wd), rad,
                                         L.ptr(scratch), ws, C.byref(v0), C.byref(v1), G.stream())
    assert bad == L.BP_EINVAL


# ---------------------------------------------------------------------------------------------- 3. the gather
GATHER_MODES, GATHER_K = {"dm": "log", "pressure": "shift-log-2p"}, {"dm": 2.0, "pressure": (0.5, 3.0)}


@pytest.mark.parametrize("kind", ["single scale", "minimum and scales"])
def test_assembled_batch_of_a_log_and_a_two_parameter_field_equals_the_host_dataset(kind):
    """``get_batch`` against ``dataset[i]``: single scale within the forward tolerance (one float32 spacing of the host
    value); ``subtract_minimum`` + split-scale: the pyramid of the gathered tile, bit-equal to bp_split_scale of the
    single-scale batch of the same tiles, which is held to the forward tolerance."""
    fwd, inv = T.create_range_compress_transforms(GATHER_K, GATHER_MODES)
    sub = kind != "single scale"
    single = tile_dataset(16, transform=T.chain_transformations([fwd, T.atleast_3d, T.as_float32]), sub=sub)
    idx = permutation_indices(single)
    asm = DeviceTileAssembler(single, "cuda:0")
    assert set(asm.compress) == {"dm", "pressure"} and asm.levels == 1
    x, y, z = asm.get_batch(idx)
    assert x.shape == y.shape == (len(idx), 1, 16, 16)
    worst = 0.0
    for n, i in enumerate(idx):
        (dm, pr), _, zz = single[i]
        if sub:
            assert dm.min() == np.float32(np.log(R.EPS) / 2.0)        # the minimum pixel is 0: log's branch value
        for got, host in ((y[n, 0], dm), (x[n, 0], pr)):
            err = np.abs(got.cpu().numpy().astype(np.float64) - np.asarray(host[0], np.float64))
            worst = max(worst, float((err / R.forward_tolerance(host[0])).max()))
    print(kind, "worst err / (one float32 spacing)", worst)
    assert worst <= 1.0
    if not sub:
        return
    split = T.create_split_scale_transform(3, 4, True)[0]
    multi = tile_dataset(16, transform=T.chain_transformations([fwd, T.as_float32, split, T.atleast_3d]), sub=True,
                         n_feature_per_field=4)
    asm3 = DeviceTileAssembler(multi, "cuda:0")
    assert asm3.levels == 4
    x3, y3, z3 = asm3.get_batch(idx)
    assert torch.equal(y3, _split_nchw(y[:, 0].contiguous(), 3, 1)) and torch.equal(x3, _split_nchw(x[:, 0].contiguous(), 3, 1))
    assert torch.equal(z3, z)


# ---------------------------------------------------------------------------------------------- 4. painters
SIZE = 64
PAIRS = {"log, shift-log-2p": ({"dm": "log", "pressure": "shift-log-2p"}, {"dm": 2.0, "pressure": (0.5, 3.0)}),
         "x/(1+x), 1/x": ({"dm": "x/(1+x)", "pressure": "1/x"}, {"dm": (2.0, 1.0), "pressure": 2.0})}


def _build_painter(pair, tmp_path_factory):
    """A 64^2 fiducial painter of one mode pair, loaded from checkpoint files (tests/test_gpu_paint_pipeline.py)."""
    from baryon_painter_amd.painter import CVAEPainter
    modes, ks = PAIRS[pair]
    fwd, inv = T.create_range_compress_transforms(ks, modes, sqrt_of_mean=True)
    tr = T.chain_transformations([fwd, T.atleast_3d, T.as_float32])
    itr = T.chain_transformations([T.squeeze, inv])
    ds = BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=1,
                        n_stack=3, transform=tr, inverse_transform=itr, scale_to_SLICS=True)
    torch.manual_seed(3)
    p = CVAEPainter(training_data_set=ds, test_data_set=ds, architecture=A.fiducial_architecture(SIZE),
                    compute_device="cuda:0")
    x, y, aux = syn.synthetic_batch(4, SIZE, SIZE, seed=77)
    with torch.no_grad():
        p.model(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
    d = tmp_path_factory.mktemp("ckpt")
    files = (str(d / "state"), str(d / "meta"))
    p.save_state_to_file(files)
    q = CVAEPainter(filename=files, compute_device="cuda:0")
    q.checkpoint_files = files
    tiles = np.stack([np.asarray(ds.get_input_sample(i % len(ds), transform=False), np.float32) for i in range(5)])
    tiles *= (1.0 + 0.1 * np.arange(5, dtype=np.float32))[:, None, None]
    tiles[0, 0, :2] = (0.0, -0.05)                                # the forward branch values on the way in
    return q, tiles, np.array([0.0, 0.3, 2.5, 0.5, -0.2]), pair


@pytest.fixture(scope="module")
def painters(tmp_path_factory):
    """pair -> (painter, raw tiles, redshifts, pair), built once per pair."""
    cache = {}

    def get(pair):
        if pair not in cache:
            cache[pair] = _build_painter(pair, tmp_path_factory)
        return cache[pair]
    return get


@pytest.mark.parametrize("pair", list(PAIRS))
def test_paint_stream_equals_per_tile_paint_with_host_transforms(painters, pair):
    """5 tiles at batch 2 (a short last batch) against per-tile ``paint`` under the oracle's Philox normals.  Limit, per
    tile, as a multiple of the largest pixel: what tests/test_gpu_paint_pipeline.py allows a shift-log painter, 3e-7 --
    the two network inputs agree to one float32 ulp of the transformed tile, as there -- with its share for the
    inverse replaced by the measured one: 4 x the host float32 inverse's own worst error against the formula in
    float64 on this tile's activations (the bound of test_store_equals_the_host_inverse), plus the host formula's
    response to 4 float32 ulps of the activation, which is how far an input ulp may move it."""
    q, tiles, zs, pair = painters(pair)
    assert q.can_paint_stream()
    modes, ks = PAIRS[pair]
    seed, ids = 99, np.arange(5, dtype=np.int64) + 1000
    out = q.paint_stream(tiles, zs, batch_size=2, tile_ids=ids, seed=seed)
    assert out.shape == tiles.shape and out.dtype == np.float32
    g = next(v for k, v in q.model._graphs.items() if isinstance(k, tuple) and "modes" in k)
    assert g["slots"][0]["xf_in"].shape == (2, 4) and g["slots"][0]["xf_out"].shape == (2, 4)
    per_tile = int(np.prod(q.model.dim_z))
    stats, mode, k = q.inverse_transform.stats["pressure"], modes["pressure"], ks["pressure"]
    for i in range(len(tiles)):
        q.model._eps_override = tile_normals(seed, [ids[i]], per_tile).reshape(1, 1, *q.model.dim_z)
        with np.errstate(invalid="ignore"):                       # (the host's np.where evaluates log at the pixel below 0)
            ref = np.asarray(q.paint(tiles[i], z=float(zs[i])), np.float64)
            act = np.asarray(q.paint(tiles[i], z=float(zs[i]), inverse_transform=False), np.float32)[0, 0]
        assert ref.shape == (SIZE, SIZE) and np.isfinite(ref).all()
        s = T.interpolate_z(stats, float(zs[i]))
        args = (mode, k, np.sqrt(s["var"]), np.sqrt(s["mean"]), 1e-3)
        exact = R.inverse_f64(*args, act)
        host_err = np.abs(ref - exact).max()
        moved = np.abs(R.inverse_f64(*args, act + 4 * np.spacing(act)) - exact).max()
        scale = np.abs(ref).max()
        tol = 3e-7 * scale + 4 * host_err + moved
        err = np.abs(out[i] - ref).max()
        print(pair, "tile", i, "err / max|ref|", err / scale, "limit / max|ref|", tol / scale,
              "in float32 roundings:", tol / scale * 2 ** 24)
        assert err <= tol, (i, err, tol)
    q.model._eps_override = None
    assert np.array_equal(q.paint_stream(tiles, zs, batch_size=5, tile_ids=ids, seed=seed), out)


@pytest.mark.parametrize("pair", list(PAIRS))
def test_saved_and_loaded_painter_paints_the_same_bits(painters, pair):
    from baryon_painter_amd.painter import CVAEPainter
    q, tiles, zs, pair = painters(pair)
    again = CVAEPainter(filename=q.checkpoint_files, compute_device="cuda:0")
    assert again.can_paint_stream()
    a = q.paint_stream(tiles, zs, batch_size=2, seed=5)
    assert np.array_equal(again.paint_stream(tiles, zs, batch_size=2, seed=5), a)


def test_device_plane_equals_host_plane(painters):
    """The limit of tests/test_gpu_paint_plane_device.py: both paths paint through the same kernels and blend in
    float64.  On the commit before, ``on_device=True`` raises for this painter."""
    q, tiles, zs, pair = painters("log, shift-log-2p")
    rng = np.random.Generator(np.random.PCG64(41))
    delta = (np.exp(rng.standard_normal((160, 160)) * 0.5) * 0.05).astype(np.float32)
    rel, z = SIZE / 160, 0.42
    host = LC.paint_plane(q, delta, rel, SIZE, z, seed=5, batch_size=4)
    dev = LC.paint_plane(q, delta, rel, SIZE, z, seed=5, batch_size=4, on_device=True)
    assert dev.shape == host.shape == (160, 160) and dev.dtype == np.float64
    ok = np.isfinite(host)
    assert np.array_equal(np.isfinite(dev), ok) and ok.mean() > 0.9
    err, scale = np.abs(dev[ok] - host[ok]).max(), np.abs(host[ok]).max()
    print("plane err / scale", err / scale)
    assert err <= 1e-6 * scale
