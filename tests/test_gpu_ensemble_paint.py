"""GPU: ``CVAEPainter.paint_ensemble`` -- K latent draws per tile, mean and variance reduced on the device -- on 64^2
tiles with the painters of tests/test_gpu_pixel_noise_paint.py (two heads, the variance bias at -4, restored from their
(state, meta) files).  Every draw against per-tile ``paint`` under the oracle's latent normals for (seed, tile id, draw),
within that file's 3e-7 of the reference tile's maximum; draw 0 against ``paint_stream``; the moments against the float64
loop of tests/ensemble_ref.py over the returned draws, bit for bit; batching, sharding, seeds, pixel noise, a two-field,
a split-scale and an L = 2 painter, and weights changed after the capture."""
import numpy as np
import pytest
import torch

import ensemble_ref as E
import host_cases as HC
import multi_field_cases as MF
import test_gpu_pixel_noise_paint as PN
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils import synthetic as syn
from baryon_painter_amd.utils.datasets import BAHAMASDataset
from golden import make_goldens_cond_net as CN
from oracle.philox import tile_normals

pytestmark = pytest.mark.gpu
SIZE = PN.SIZE
LIMIT = 3e-7
SEED = 99
IDS = np.arange(5, dtype=np.int64) + 1000


@pytest.fixture(scope="module")
def painter(tmp_path_factory):
    ds = PN.single_field_dataset()
    q = PN.build(tmp_path_factory.mktemp("ckpt"), PN.two_head_architecture(), ds)
    # One training-mode forward leaves the running statistics a tenth of the way from their initial values: in eval mode
    # p_z_in's batch-norm layers then hardly normalise, h_z stays tiny beside y, and the draws of a tile differ by less
    # than the 3e-7 they are compared within.  Thirty more (no gradients, the weights stay) settle the statistics, as
    # training would, and the latent matters; the checkpoint files keep the state PN.build saved.
    x, y, aux = syn.synthetic_batch(4, SIZE, SIZE, seed=77)
    q.model.train(True)
    with torch.no_grad():
        for _ in range(30):
            q.model(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
    q.model.train(False)
    return q, PN.raw_tiles(ds, 5), PN.ZS[:5]


def per_draw_reference(q, tiles, zs, seed, ids, K, pixel_noise=False):
    """(n, K, [F,] H, W) float64: draw k of tile i as per-tile ``paint`` under the latent normals of counter
    (g, k, id_i); with ``pixel_noise`` on the lattice id_i + (k << 40)."""
    per_tile = int(np.prod(q.model.dim_z))
    eps = tile_normals(seed, list(ids), per_tile, L=K)
    out = []
    try:
        for i in range(len(tiles)):
            row = []
            for k in range(K):
                q.model._eps_override = eps[k, i].reshape(1, 1, *q.model.dim_z)
                kw = {"pixel_noise": True, "seed": seed, "noise_id": int(ids[i]) + (k << 40)} if pixel_noise else {}
                row.append(np.asarray(q.paint(tiles[i], z=float(zs[i]), **kw), np.float64))
            out.append(np.stack(row))
    finally:
        q.model._eps_override = None
    return np.stack(out)


def assert_draws_equal(draws, ref, what):
    """Every (tile, draw[, field]) plane within LIMIT of the reference plane's maximum."""
    H, W = draws.shape[-2:]
    PN.assert_stream_equals_per_tile(draws.reshape(-1, H, W), ref.reshape(-1, H, W), LIMIT, what)


def assert_moments_of(mean, var, draws):
    m, v = E.moments(draws, axis=1)
    assert mean.dtype == var.dtype == draws.dtype == np.float32
    assert E.same_bits(mean, m) and E.same_bits(var, v)


def test_draws_equal_per_tile_paint_and_the_moments_are_those_of_the_draws(painter):
    """5 tiles at mixed redshifts, 4 draws, batch_size 8: two tiles per batch, a ragged last batch."""
    q, tiles, zs = painter
    mean, var, draws = q.paint_ensemble(tiles, zs, draws=4, batch_size=8, tile_ids=IDS, seed=SEED, return_draws=True)
    assert mean.shape == var.shape == tiles.shape and draws.shape == (5, 4, SIZE, SIZE) and np.isfinite(draws).all()
    key = (2, "ensemble", 4, "modes", 0, 0, "draws")
    assert key in q.model._graphs and tuple(q.model._graphs[key]["slots"][0]["draws"].shape) == (2, 4, 1, SIZE, SIZE)
    assert_draws_equal(draws, per_draw_reference(q, tiles, zs, SEED, IDS, 4), "single field")
    assert_moments_of(mean, var, draws)
    assert (var > 0).any() and (var >= 0).all()
    rel = np.sqrt(var).max(axis=(1, 2)) / np.abs(mean).max(axis=(1, 2))
    print("largest scatter over largest mean, per tile", rel)
    assert (rel > 1e-4).all()                                      # the draws differ
    # draw 0 is the tile paint_stream paints for the same seed and id
    stream = q.paint_stream(tiles, zs, batch_size=4, tile_ids=IDS, seed=SEED)
    assert_draws_equal(draws[:, 0], stream.astype(np.float64), "draw 0 against paint_stream")
    # without the draws: a graph of its own, the same moments
    mean2, var2 = q.paint_ensemble(tiles, zs, draws=4, batch_size=8, tile_ids=IDS, seed=SEED)
    assert E.same_bits(mean2, mean) and E.same_bits(var2, var)
    assert key[:-1] in q.model._graphs and "draws" not in q.model._graphs[key[:-1]]["slots"][0]


def test_one_draw_has_no_variance(painter):
    q, tiles, zs = painter
    mean, var, draws = q.paint_ensemble(tiles, zs, draws=1, batch_size=4, tile_ids=IDS, seed=SEED, return_draws=True)
    assert draws.shape == (5, 1, SIZE, SIZE) and (var == 0).all() and E.same_bits(mean, draws[:, 0])
    assert_draws_equal(draws, per_draw_reference(q, tiles, zs, SEED, IDS, 1), "one draw")


def test_draws_do_not_depend_on_batching_or_sharding(painter):
    q, tiles, zs = painter
    kw = {"draws": 4, "tile_ids": IDS, "seed": 7, "return_draws": True}
    ref = q.paint_ensemble(tiles, zs, batch_size=8, **kw)
    wide = q.paint_ensemble(tiles, zs, batch_size=16, **kw)
    assert_draws_equal(wide[2], ref[2].astype(np.float64), "batch 16 against batch 8")
    assert_moments_of(*wide)
    parts = [q.paint_ensemble(tiles, zs, batch_size=8, rank=r, world_size=2, **kw) for r in range(2)]
    assert [p[1] for p in parts] == [(0, 3), (3, 5)]
    for (m, v, d), (lo, hi) in parts:
        assert m.shape == (hi - lo, SIZE, SIZE) and d.shape == (hi - lo, 4, SIZE, SIZE)
        assert_moments_of(m, v, d)
    assert_draws_equal(np.concatenate([p[0][2] for p in parts]), ref[2].astype(np.float64), "two ranks against one")


def test_a_second_seed_changes_the_draws_and_captures_nothing(painter):
    q, tiles, zs = painter
    kw = {"draws": 4, "batch_size": 8, "tile_ids": IDS, "return_draws": True}
    first = q.paint_ensemble(tiles, zs, seed=7, **kw)
    n_graphs, n_plans = len(q.model._graphs), len(q.model._paint_plans)
    second = q.paint_ensemble(tiles, zs, seed=2 ** 63 + 5, **kw)
    again = q.paint_ensemble(tiles, zs, seed=7, **kw)
    assert (len(q.model._graphs), len(q.model._paint_plans)) == (n_graphs, n_plans)
    assert not np.array_equal(second[2], first[2]) and all(np.array_equal(a, b) for a, b in zip(again, first))
    assert_moments_of(*second)
    # other tile ids: other draws, the same graph
    other = q.paint_ensemble(tiles, zs, seed=7, **dict(kw, tile_ids=IDS + 50))
    assert not np.array_equal(other[2], first[2]) and len(q.model._graphs) == n_graphs


def test_pixel_noise_draws_equal_per_tile_paint_on_the_lattices_of_the_draws(painter):
    q, tiles, zs = painter
    plain = q.paint_ensemble(tiles, zs, draws=4, batch_size=8, tile_ids=IDS, seed=SEED, return_draws=True)
    mean, var, draws = q.paint_ensemble(tiles, zs, draws=4, batch_size=8, tile_ids=IDS, seed=SEED, return_draws=True,
                                        pixel_noise=True)
    assert (2, "ensemble", 4, "modes", 0, 0, "noise", "draws") in q.model._graphs
    assert_draws_equal(draws, per_draw_reference(q, tiles, zs, SEED, IDS, 4, pixel_noise=True), "pixel noise")
    assert_moments_of(mean, var, draws)
    rel = np.abs(draws - plain[2]).max(axis=(2, 3)) / np.abs(plain[2]).max(axis=(2, 3))
    assert (rel > 1e-2).all(), rel                                  # draws from the likelihood, not its means
    # four tiles per batch: the graph paints them as two sub-batches, each with the lattice ids of its own draws
    wide = q.paint_ensemble(tiles, zs, draws=4, batch_size=16, tile_ids=IDS, seed=SEED, return_draws=True,
                            pixel_noise=True)
    g = q.model._graphs[(4, "ensemble", 4, "modes", 0, 0, "noise", "draws")]
    assert g["parts"] == 2 and g["block_layout"]["noise_ids"][2] == (2, 4, 2) and "noise_org" not in g["block_layout"]
    assert_draws_equal(wide[2], draws.astype(np.float64), "pixel noise, batch 16 against batch 8")
    assert_moments_of(*wide)
    # lattice ids of the caller's choice
    nid = np.array([5, 5, 20, 21, 2 ** 40 - 1], np.int64)
    other = q.paint_ensemble(tiles, zs, draws=4, batch_size=8, tile_ids=IDS, seed=SEED, return_draws=True,
                             pixel_noise=True, noise_ids=nid)
    assert not np.array_equal(other[2], draws)
    n_graphs = len(q.model._graphs)
    with pytest.raises(ValueError):
        q.paint_ensemble(tiles, zs, draws=4, batch_size=8, pixel_noise=True, noise_ids=nid + 1)
    assert len(q.model._graphs) == n_graphs


def test_two_field_painter(tmp_path):
    """n_fields = 2 in the modes of multi_field_cases (log and shift-log-2p): field planes side by side."""
    tr, itr = MF.chains(T)
    ds = BAHAMASDataset(data=MF.data_dict3(), redshifts=list(HC.REDSHIFTS), label_fields=list(MF.LABELS), n_tile=1,
                        n_stack=3, transform=tr, inverse_transform=itr, scale_to_SLICS=True)
    q = PN.build(tmp_path, PN.two_head_architecture(n_fields=2), ds,
                 lambda c: (1.0 - 0.15 * np.arange(c, dtype=np.float32))[None, :, None, None])
    tiles, zs = PN.raw_tiles(ds, 5), PN.ZS[:5]
    mean, var, draws = q.paint_ensemble(tiles, zs, draws=4, batch_size=8, tile_ids=IDS, seed=SEED, return_draws=True)
    assert mean.shape == (5, 2, SIZE, SIZE) and draws.shape == (5, 4, 2, SIZE, SIZE) and np.isfinite(draws).all()
    assert any(isinstance(k, tuple) and k[1] == "ensemble" and "fields" in k for k in q.model._graphs)
    ref = per_draw_reference(q, tiles, zs, SEED, IDS, 4)
    for f in range(2):
        assert_draws_equal(draws[:, :, f], ref[:, :, f], f"field {f}")
    assert_moments_of(mean, var, draws)
    assert (var > 0).any()


def test_split_scale_painter(tmp_path):
    """n_scale = 3 without the original: the store sums the head's channels in front of the inverse, per draw."""
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    split, unsplit = T.create_split_scale_transform(3, 4, False)
    tr = T.chain_transformations([fwd, T.as_float32, split, T.atleast_3d])
    itr = T.chain_transformations([unsplit, inv, T.squeeze])
    ds = BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=1,
                        n_stack=3, transform=tr, inverse_transform=itr, n_feature_per_field=3, scale_to_SLICS=True)
    q = PN.build(tmp_path, PN.two_head_architecture(n_scale=3), ds,
                 lambda c: (1.0 - 0.2 * np.arange(c, dtype=np.float32))[None, :, None, None])
    tiles, zs = PN.raw_tiles(ds, 5), PN.ZS[:5]
    mean, var, draws = q.paint_ensemble(tiles, zs, draws=4, batch_size=8, tile_ids=IDS, seed=SEED, return_draws=True)
    assert draws.shape == (5, 4, SIZE, SIZE) and np.isfinite(draws).all()
    assert any(isinstance(k, tuple) and k[1] == "ensemble" and "scales" in k for k in q.model._graphs)
    assert_draws_equal(draws, per_draw_reference(q, tiles, zs, SEED, IDS, 4), "split scale")
    assert_moments_of(mean, var, draws)
    q.release_paint_buffers()
    assert not any(isinstance(k, tuple) and "scales" in k for k in q.model._graphs)


def test_a_model_with_two_latent_samples_and_a_p_y_in_network(tmp_path):
    """Case b of tests/golden/make_goldens_cond_net.py: L = 2 and a p_y_in network.  The number of draws is the
    argument's, not the model's; ``paint_stream`` still refuses the model."""
    from baryon_painter_amd.painter import CVAEPainter
    arch = CN.architectures()["b"]
    ds = PN.single_field_dataset()
    torch.manual_seed(3)
    p = CVAEPainter(training_data_set=ds, test_data_set=ds, architecture=arch, compute_device="cuda:0")
    x, y, aux = syn.synthetic_batch(4, SIZE, SIZE, seed=77)
    with torch.no_grad():
        p.model(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
    files = (str(tmp_path / "state"), str(tmp_path / "meta"))
    p.save_state_to_file(files)
    q = CVAEPainter(filename=files, compute_device="cuda:0")
    assert q.model.L == 2 and q.model.has_p_y_in
    tiles, zs = PN.raw_tiles(ds, 5), PN.ZS[:5]
    mean, var, draws = q.paint_ensemble(tiles, zs, draws=4, batch_size=8, tile_ids=IDS, seed=SEED, return_draws=True)
    assert_draws_equal(draws, per_draw_reference(q, tiles, zs, SEED, IDS, 4), "L = 2 with p_y_in")
    assert_moments_of(mean, var, draws)
    assert (var > 0).any()
    assert not q.can_paint_stream()
    with pytest.raises(NotImplementedError):
        q.paint_stream(tiles, zs, batch_size=4)
    # sample_P(samples=K): the same plan without the transforms, under the same normals
    per_tile = int(np.prod(q.model.dim_z))
    yt = np.stack([np.asarray(q.transform(t, field=q.input_field, z=float(z))) for t, z in zip(tiles[:2], zs[:2])])
    try:
        q.model._eps_override = tile_normals(SEED, list(IDS[:2]), per_tile, L=4).reshape(4, 2, *q.model.dim_z)
        net = q.model.sample_P(torch.from_numpy(yt.reshape(2, *q.model.dim_y)), aux_label=torch.from_numpy(zs[:2]),
                               samples=4).cpu().numpy()
    finally:
        q.model._eps_override = None
    assert net.shape == (2, 4, 1, SIZE, SIZE)
    for i in range(2):
        for k in range(4):
            phys = np.asarray(q.inverse_transform(net[i, k], field=q.label_fields[0], z=float(zs[i])), np.float64)
            assert np.abs(draws[i, k] - phys).max() <= LIMIT * np.abs(phys).max(), (i, k)


def test_weights_changed_after_the_capture_reach_the_next_ensemble(painter):
    from baryon_painter_amd.painter import CVAEPainter
    q, tiles, zs = painter
    w = CVAEPainter(filename=q.checkpoint_files, compute_device="cuda:0")
    kw = {"draws": 4, "batch_size": 8, "tile_ids": IDS, "seed": 3}
    first = w.paint_ensemble(tiles, zs, **kw)
    head = [m for m in w.model.p_mu_out.modules() if isinstance(getattr(m, "weight", None), torch.Tensor)][-1]
    with torch.no_grad():
        head.weight.mul_(0.5)                    # (a weight is packed, and re-packed by the graph's units)
    second = w.paint_ensemble(tiles, zs, **kw)
    files = (q.checkpoint_files[0] + ".ensemble", q.checkpoint_files[1])
    torch.save({k: v.detach().cpu().clone() for k, v in w.model.state_dict().items()}, files[0])
    fresh = CVAEPainter(filename=files, compute_device="cuda:0").paint_ensemble(tiles, zs, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(fresh, second))
    assert not np.array_equal(second[0], first[0])
