"""GPU: painting draws from the likelihood (``pixel_noise=True``) on every paint surface of a two-head CVAE painter --
``sample_P`` against the float32 restatement of the draw, ``paint_stream`` against per-tile ``paint``, batching and
sharding, seeds and ids without new graphs, weights changed after the capture, planes on the host and device paths, a
two-field and a split-scale painter, the bf16 trunk, and the painters that have no variance head.

The fiducial heads have no bias (arch.fiducial_architecture), so the painters here give the LAST convolution of the
variance head one and set it to -4: the scatter, exp(-2) in network units, is then a fraction of the signal."""
import numpy as np
import pytest
import torch

import host_cases as HC
import multi_field_cases as MF
from baryon_painter_amd import lightcone as LC
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils import synthetic as syn
from baryon_painter_amd.utils.datasets import BAHAMASDataset
from oracle.philox import tile_normals

import pixel_noise_ref as R

pytestmark = pytest.mark.gpu
SIZE = 64


def two_head_architecture(**kw):
    arch = A.fiducial_architecture(SIZE, predict_var=True, **kw)
    mu, var = arch["p_y_z_out"]
    name, cfg = var[-1]
    assert name == "conv"
    arch["p_y_z_out"] = (mu, list(var[:-1]) + [(name, dict(cfg, bias=True))])
    return arch


def var_last(model):
    """The last convolution of the variance head (the one with the bias)."""
    return [m for m in model.p_var_out.modules() if getattr(m, "bias", None) is not None][-1]


def build(tmp, arch, ds, channel_scale=None):
    """A painter of ``arch`` on ``ds`` with non-trivial running statistics and the variance bias at -4, saved and
    reloaded from (state, meta) files as in tests/test_gpu_paint_pipeline.py."""
    from baryon_painter_amd.painter import CVAEPainter
    torch.manual_seed(3)
    p = CVAEPainter(training_data_set=ds, test_data_set=ds, architecture=arch, compute_device="cuda:0")
    x, y, aux = syn.synthetic_batch(4, SIZE, SIZE, seed=77)
    sx = 1.0 if channel_scale is None else channel_scale(arch["dim_x"][0])
    sy = 1.0 if channel_scale is None else channel_scale(arch["dim_y"][0])
    with torch.no_grad():
        p.model(torch.from_numpy(x * sx), torch.from_numpy(y * sy), torch.from_numpy(aux))
        var_last(p.model).bias.fill_(-4.0)
    files = (str(tmp / "state"), str(tmp / "meta"))
    p.save_state_to_file(files)
    q = CVAEPainter(filename=files, compute_device="cuda:0")
    q.checkpoint_files = files
    return q


def single_field_dataset():
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    tr = T.chain_transformations([fwd, T.atleast_3d, T.as_float32])
    itr = T.chain_transformations([T.squeeze, inv])
    return BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=1,
                          n_stack=3, transform=tr, inverse_transform=itr, scale_to_SLICS=True)


def raw_tiles(ds, n):
    tiles = np.stack([np.asarray(ds.get_input_sample(i % len(ds), transform=False), np.float32) for i in range(n)])
    return tiles * (1.0 + 0.1 * np.arange(n, dtype=np.float32))[:, None, None]


ZS = np.array([0.0, 0.3, 2.0, 0.5, 1.1, 0.0, 2.0, 0.125, 1.9, 0.7, 0.3])


@pytest.fixture(scope="module")
def painter(tmp_path_factory):
    ds = single_field_dataset()
    q = build(tmp_path_factory.mktemp("ckpt"), two_head_architecture(), ds)
    return q, raw_tiles(ds, 11), ZS


def per_tile_reference(q, tiles, zs, seed, ids, noise_ids=None, origins=None):
    """Tile-by-tile ``paint(pixel_noise=True)`` under the oracle's latent normals for (seed, tile id)."""
    per_tile = int(np.prod(q.model.dim_z))
    out = []
    try:
        for i in range(len(tiles)):
            q.model._eps_override = tile_normals(seed, [ids[i]], per_tile).reshape(1, 1, *q.model.dim_z)
            out.append(np.asarray(q.paint(tiles[i], z=float(zs[i]), pixel_noise=True, seed=seed,
                                          noise_id=int(ids[i] if noise_ids is None else noise_ids[i]),
                                          noise_origin=(0, 0) if origins is None else tuple(origins[i])), np.float64))
    finally:
        q.model._eps_override = None
    return np.stack(out)


def assert_stream_equals_per_tile(out, ref, limit, what):
    for i in range(len(ref)):
        scale = np.abs(ref[i]).max()
        err = np.abs(out[i] - ref[i]).max()
        print(what, "tile", i, "err / max|ref|", err / scale, "limit", limit)
        assert err <= limit * scale, (what, i, err / scale, limit)


def test_sample_P_draw_equals_the_restatement_of_its_two_heads(painter):
    q, tiles, zs = painter
    m = q.model
    n = 3
    _, y, aux = syn.synthetic_batch(n, SIZE, SIZE, seed=5)
    z = syn.synthetic_eps((n, *m.dim_z), seed=6)
    seed, ids, org = 2 ** 40 + 17, np.array([3, 2 ** 33 + 5, 3], np.int64), np.array([(0, 0), (9, 70), (5, 6)], np.int32)
    m.train(False)
    mean = m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux), z=z).cpu().numpy()
    got = m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux), z=z,
                     pixel_noise={"seed": seed, "ids": ids, "origins": org}).cpu().numpy()
    plan = m._paint_plan(n)
    assert plan.draw.buf.dtype == torch.float32 and plan.draw.shape() == plan.mu_head.shape()
    mu, lv = torch.empty((n, 1, SIZE, SIZE), device="cuda"), torch.empty((n, 1, SIZE, SIZE), device="cuda")
    m._head_to_nchw(plan.mu_head, plan.mu_softplus, mu)
    m._head_to_nchw(plan.var_head, False, lv)
    mu, lv = mu.cpu().numpy(), lv.cpu().numpy()
    assert np.array_equal(mu, mean) and abs(lv.mean() + 4) < 1
    e = R.lattice_normals(seed, ids, org, SIZE, SIZE, 1).transpose(0, 3, 1, 2)
    ref, p = R.draw_ref(mu, lv, e)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    assert (err <= R.draw_bound(ref, p)).all(), float((err / R.draw_bound(ref, p)).max())
    assert np.abs(got - mean).max() > 0.1 and np.isfinite(got).all()
    # null origins are zero origins; the mean is what it was
    a = m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux), z=z,
                   pixel_noise={"seed": seed, "ids": ids, "origins": None}).cpu().numpy()
    assert np.array_equal(a[0], got[0]) and not np.array_equal(a[1], got[1]) and not np.array_equal(a[2], got[2])
    assert np.array_equal(m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux), z=z).cpu().numpy(), mean)
    with pytest.raises(ValueError):
        m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux), z=z,
                   pixel_noise={"seed": seed, "ids": ids, "origins": -org})


def test_paint_stream_with_noise_equals_per_tile_paint(painter):
    """11 tiles at batch 4 within 3e-7 max|ref| (tests/test_gpu_paint_pipeline.py,
    test_paint_stream_equals_per_tile_paint); the mean painting before and after keeps its bits and its graph."""
    q, tiles, zs = painter
    seed, ids = 99, np.arange(11, dtype=np.int64) + 1000
    before = q.paint_stream(tiles, zs, batch_size=4, tile_ids=ids, seed=seed)
    n_graphs = len(q.model._graphs)
    out = q.paint_stream(tiles, zs, batch_size=4, tile_ids=ids, seed=seed, pixel_noise=True)
    assert out.shape == tiles.shape and out.dtype == np.float32 and np.isfinite(out).all()
    assert len(q.model._graphs) == n_graphs + 1
    key, g = next((k, v) for k, v in q.model._graphs.items() if isinstance(k, tuple) and "noise" in k)
    assert key == (4, "pipeline", "noise") and list(g["block_layout"])[-2:] == ["noise_ids", "noise_org"]
    assert g["plans"][0].draw.buf.dtype == torch.float32
    assert_stream_equals_per_tile(out, per_tile_reference(q, tiles, zs, seed, ids), 3e-7, "single field")
    rel = np.abs(out - before).max(axis=(1, 2)) / np.abs(before).max(axis=(1, 2))
    assert (rel > 1e-2).all(), rel                                  # a draw, not the mean
    after = q.paint_stream(tiles, zs, batch_size=4, tile_ids=ids, seed=seed)
    assert np.array_equal(after, before) and len(q.model._graphs) == n_graphs + 1
    # ids and origins of the caller's choice: tiles 0 and 1 share a lattice and overlap
    nid = np.array([5, 5] + list(range(20, 29)), np.int64)
    org = np.zeros((11, 2), np.int32)
    org[1] = (5, 6)
    org[4] = (2 ** 20, 2 ** 23)
    out2 = q.paint_stream(tiles, zs, batch_size=4, tile_ids=ids, seed=seed, pixel_noise=True, noise_ids=nid,
                          noise_origins=org)
    ref2 = per_tile_reference(q, tiles, zs, seed, ids, nid, org)
    assert_stream_equals_per_tile(out2, ref2, 3e-7, "ids and origins")
    assert not np.array_equal(out2[2], out[2])
    with pytest.raises(ValueError):
        q.paint_stream(tiles, zs, batch_size=4, pixel_noise=True, noise_origins=-org)
    with pytest.raises(ValueError):
        q.paint_stream(tiles, zs, batch_size=4, pixel_noise=True, noise_origins=org + 2 ** 24 - 64)


def test_noise_is_independent_of_batching_and_sharding_and_needs_one_graph(painter):
    q, tiles, zs = painter
    ref = q.paint_stream(tiles, zs, batch_size=4, seed=7, pixel_noise=True)
    assert np.array_equal(q.paint_stream(tiles, zs, batch_size=11, seed=7, pixel_noise=True), ref)
    assert np.array_equal(q.paint_stream(tiles, zs, batch_size=3, seed=7, pixel_noise=True), ref)
    for world in (2, 3):
        parts = [q.paint_stream(tiles, zs, batch_size=4, seed=7, pixel_noise=True, rank=r, world_size=world)
                 for r in range(world)]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), ref)
    # several seeds and noise ids: no new graph, no new plan
    n_graphs, n_plans = len(q.model._graphs), len(q.model._plans)
    outs = [q.paint_stream(tiles[:4], zs[:4], batch_size=4, seed=s, pixel_noise=True, noise_ids=np.arange(4) + k)
            for s, k in ((7, 0), (8, 0), (2 ** 63 + 5, 0), (7, 100), (7, 0))]
    assert (len(q.model._graphs), len(q.model._plans)) == (n_graphs, n_plans)
    assert np.array_equal(outs[0], ref[:4]) and np.array_equal(outs[4], outs[0])
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])
    assert not np.array_equal(outs[0], outs[3])
    # paint_batch: the same draws under the same latent normals are not to be had (its latent noise is torch's), but
    # its keywords reach sample_P: reproducible under a seed for a given latent
    per_tile = int(np.prod(q.model.dim_z))
    try:
        q.model._eps_override = tile_normals(7, [0, 1], per_tile).reshape(1, 2, *q.model.dim_z)
        pb = q.paint_batch(tiles[:2], zs[:2], batch_size=2, pixel_noise=True, seed=7)
    finally:
        q.model._eps_override = None
    for i in range(2):
        assert np.abs(pb[i] - ref[i]).max() <= 3e-7 * np.abs(ref[i]).max()


def test_weights_changed_after_the_capture_reach_the_draw(painter):
    from baryon_painter_amd.painter import CVAEPainter
    q, tiles, zs = painter
    w = CVAEPainter(filename=q.checkpoint_files, compute_device="cuda:0")
    first = w.paint_stream(tiles[:4], zs[:4], batch_size=4, seed=3, pixel_noise=True)
    head = var_last(w.model)
    with torch.no_grad():
        head.bias.add_(2.0)
        head.weight.mul_(0.5)        # (a bias is read where it lies; a weight is packed, and re-packed by the graph's units)
    second = w.paint_stream(tiles[:4], zs[:4], batch_size=4, seed=3, pixel_noise=True)
    files = (q.checkpoint_files[0] + ".changed", q.checkpoint_files[1])
    torch.save({k: v.detach().cpu().clone() for k, v in w.model.state_dict().items()}, files[0])
    fresh = CVAEPainter(filename=files, compute_device="cuda:0")
    assert np.array_equal(fresh.paint_stream(tiles[:4], zs[:4], batch_size=4, seed=3, pixel_noise=True), second)
    assert not np.array_equal(second, first)


def _plane_delta(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (np.exp(rng.standard_normal((n, n)) * 0.5) * 0.05).astype(np.float32)


def test_planes_with_noise_on_host_and_device_paths(painter):
    """The host-path plane against the per-tile loop of test_paint_plane_equals_the_per_tile_loop (1e-6 max|ref|) with
    every tile on the lattice ``first_tile_id`` at its destination origin, and the device plane against the host plane
    under test_gpu_paint_plane_device.py's condition (the same finite pixels, 1e-6 of the largest)."""
    q, tiles, zs = painter
    delta = _plane_delta(150, 31)
    rel, z, seed, first = SIZE / 150, 0.42, 5, 40
    mean_plane = LC.paint_plane(q, delta, rel, SIZE, z, seed=seed, first_tile_id=first, batch_size=4)
    plane = LC.paint_plane(q, delta, rel, SIZE, z, seed=seed, first_tile_id=first, batch_size=4, pixel_noise=True)
    origins, slices = LC.generate_tiling(150, SIZE, 0.5)
    geo = LC.plane_geometry(150, rel, SIZE, 0.5)
    acc, wsum = np.zeros((150, 150)), np.zeros((150, 150))
    per_tile = int(np.prod(q.model.dim_z))
    tid = 0
    try:
        for j, xs in enumerate(origins):
            for k, ys in enumerate(origins):
                tile = np.asarray(LC.get_tile(delta, (xs, ys), rel), np.float32)
                dst = (slices[j][k][0].start, slices[j][k][1].start)
                assert dst == tuple(geo["dst"][tid])
                q.model._eps_override = tile_normals(seed, [first + tid], per_tile).reshape(1, 1, *q.model.dim_z)
                painted = np.asarray(q.paint(tile, z=z, pixel_noise=True, seed=seed, noise_id=first, noise_origin=dst),
                                     np.float64)
                w = LC.make_weight_map(tile.shape, falloff=0.05, sigma=0.5)
                acc[slices[j][k]] += w * painted
                wsum[slices[j][k]] += w
                tid += 1
    finally:
        q.model._eps_override = None
    with np.errstate(invalid="ignore"):
        ref = acc / wsum
    ok = np.isfinite(ref)
    assert np.array_equal(np.isfinite(plane), ok) and ok.mean() > 0.95
    assert np.abs(plane[ok] - ref[ok]).max() <= 1e-6 * np.abs(ref[ok]).max()
    assert np.abs(plane[ok] - mean_plane[ok]).max() > 1e-2 * np.abs(mean_plane[ok]).max()
    dev = LC.paint_plane(q, delta, rel, SIZE, z, seed=seed, first_tile_id=first, batch_size=4, pixel_noise=True,
                         on_device=True)
    assert dev.shape == (150, 150) and dev.dtype == np.float64 and np.array_equal(np.isfinite(dev), ok)
    err, scale = np.abs(dev[ok] - plane[ok]).max(), np.abs(plane[ok]).max()
    print("device plane against host plane: err / max", err / scale)
    assert err <= 1e-6 * scale, (err, scale)
    # the mean plane on the device is what it was
    assert np.array_equal(np.isfinite(LC.paint_plane(q, delta, rel, SIZE, z, seed=seed, first_tile_id=first,
                                                     batch_size=4, on_device=True)), ok)


def test_two_field_painter_streams_its_draws(tmp_path):
    """n_fields = 2, both fields shift-log (multi_field_cases.ALL_SHIFT_LOG): the store is bp_paint_store_fields."""
    tr, itr = MF.chains(T, *MF.ALL_SHIFT_LOG)
    ds = BAHAMASDataset(data=MF.data_dict3(), redshifts=list(HC.REDSHIFTS), label_fields=list(MF.LABELS), n_tile=1,
                        n_stack=3, transform=tr, inverse_transform=itr, scale_to_SLICS=True)
    q = build(tmp_path, two_head_architecture(n_fields=2), ds,
              lambda c: (1.0 - 0.15 * np.arange(c, dtype=np.float32))[None, :, None, None])
    tiles, zs = raw_tiles(ds, 5), ZS[:5]
    seed, ids = 99, np.arange(5, dtype=np.int64) + 1000
    out = q.paint_stream(tiles, zs, batch_size=2, tile_ids=ids, seed=seed, pixel_noise=True)
    assert out.shape == (5, 2, SIZE, SIZE) and np.isfinite(out).all()
    assert any(isinstance(k, tuple) and "fields" in k and k[-1] == "noise" for k in q.model._graphs)
    ref = per_tile_reference(q, tiles, zs, seed, ids)
    for f in range(2):
        assert_stream_equals_per_tile(out[:, f], ref[:, f], 3e-7, f"field {f}")
    mean = q.paint_stream(tiles, zs, batch_size=2, tile_ids=ids, seed=seed)
    assert all(np.abs(out[:, f] - mean[:, f]).max() > 1e-2 * np.abs(mean[:, f]).max() for f in range(2))


def test_split_scale_painter_streams_its_draws(tmp_path):
    """n_scale = 3 without the original: every head channel gets its own draw before bp_paint_store_scales sums them."""
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    split, unsplit = T.create_split_scale_transform(3, 4, False)
    tr = T.chain_transformations([fwd, T.as_float32, split, T.atleast_3d])
    itr = T.chain_transformations([unsplit, inv, T.squeeze])
    ds = BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=1,
                        n_stack=3, transform=tr, inverse_transform=itr, n_feature_per_field=3, scale_to_SLICS=True)
    q = build(tmp_path, two_head_architecture(n_scale=3), ds,
              lambda c: (1.0 - 0.2 * np.arange(c, dtype=np.float32))[None, :, None, None])
    tiles, zs = raw_tiles(ds, 5), ZS[:5]
    seed, ids = 99, np.arange(5, dtype=np.int64) + 1000
    out = q.paint_stream(tiles, zs, batch_size=4, tile_ids=ids, seed=seed, pixel_noise=True)
    assert out.shape == tiles.shape and np.isfinite(out).all()
    assert any(isinstance(k, tuple) and "scales" in k and k[-1] == "noise" for k in q.model._graphs)
    assert_stream_equals_per_tile(out, per_tile_reference(q, tiles, zs, seed, ids), 3e-7, "split scale")


def test_bf16_painter_paints_with_noise(painter):
    from baryon_painter_amd.painter import CVAEPainter
    q, tiles, zs = painter
    b = CVAEPainter(filename=q.checkpoint_files, compute_device="cuda:0", dtype="bf16")
    out = b.paint_stream(tiles[:4], zs[:4], batch_size=4, seed=3, pixel_noise=True)
    assert np.isfinite(out).all() and not np.array_equal(out, b.paint_stream(tiles[:4], zs[:4], batch_size=4, seed=3))
    g = next(v for k, v in b.model._graphs.items() if isinstance(k, tuple) and "noise" in k)
    assert g["plans"][0].h.buf.dtype == torch.bfloat16 and g["plans"][0].draw.buf.dtype == torch.float32


def test_painters_without_a_variance_head_refuse(tmp_path):
    """A mean-only CVAEPainter and a CGANPainter: ValueError before any capture and before a random number is drawn."""
    from baryon_painter_amd.painter import CGANPainter, CVAEPainter
    from baryon_painter_amd.utils import datasets as D
    ds = single_field_dataset()
    torch.manual_seed(3)
    m = CVAEPainter(training_data_set=ds, test_data_set=ds, architecture=A.fiducial_architecture(SIZE),
                    compute_device="cuda:0")
    gan = CGANPainter(training_data_set=D.SyntheticTileDataset(n_sample=4, tile_size=SIZE, seed=3), tile_size=SIZE,
                      compute_device="cuda:0", n_res=1)
    tiles, delta = raw_tiles(ds, 2), _plane_delta(100, 2)
    def graphs(model):                         # (the CGAN keeps its captured pipelines under a name of its own)
        return len(model._graphs if hasattr(model, "_graphs") else model._paint_graphs)
    for p in (m, gan):
        n_graphs, state = graphs(p.model), torch.get_rng_state()
        calls = [lambda: p.paint(tiles[0], z=0.3, pixel_noise=True),
                 lambda: p.paint_batch(tiles, 0.3, pixel_noise=True),
                 lambda: p.paint_stream(tiles, 0.3, batch_size=2, pixel_noise=True),
                 lambda: LC.paint_plane(p, delta, SIZE / 100, SIZE, 0.3, pixel_noise=True),
                 lambda: LC.paint_plane(p, delta, SIZE / 100, SIZE, 0.3, pixel_noise=True, on_device=True),
                 lambda: LC.paint_light_cone(p, [delta], [0.3], [100.0], 64.0, SIZE, 32, [1.0], pixel_noise=True)]
        for call in calls:
            with pytest.raises(ValueError):
                call()
        assert graphs(p.model) == n_graphs and torch.equal(torch.get_rng_state(), state)
    with pytest.raises(ValueError, match="no variance head"):
        m.model.train(False)
        m.model.paint_graph(4, pixel_noise=True)
    with pytest.raises(ValueError, match="no variance head"):
        _, y, aux = syn.synthetic_batch(1, SIZE, SIZE, seed=5)
        m.model.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux),
                         pixel_noise={"seed": 1, "ids": [0], "origins": None})
    assert len(m.model._graphs) == 0 and len(m.model._plans) == 0
