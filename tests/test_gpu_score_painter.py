"""GPU: ``CVAEPainter.score`` and ``CVAEPainter.reconstruct`` -- raw tiles in, the forward transforms on the device, the
normals of counter (g, k, tile id) -- against ``model.score`` / ``model.reconstruct`` on the HOST-transformed tiles under
``oracle.philox.tile_normals``, for the painters of tests/test_gpu_score_model.py, the two-field painter of
tests/multi_field_cases.py, a ``log`` / ``log-tanh`` painter and a split-scale painter (which is refused).

Limits are the model-level ones of tests/test_gpu_score_model.py (per log-weight: four times the float32 CPU twin's
deviation from float64, floor 2e-5 of the sum of magnitudes; the largest of a tile for its columns 0-3).  If every
log-weight of a tile moves by at most d, the effective sample size (sum w)^2 / sum w^2 moves by a factor within
exp(+-4 d): that is its limit here."""
import numpy as np
import pytest
import torch

import host_cases as HC
import multi_field_cases as MF
import score_ref as S
import test_gpu_pixel_noise_paint as PN
import test_gpu_score_model as SM
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils.datasets import BAHAMASDataset
from oracle.philox import tile_normals

pytestmark = pytest.mark.gpu
SIZE = PN.SIZE
K, SEED = 4, 99
IDS = np.arange(5, dtype=np.int64) + 1000
ZS = PN.ZS[:5]


def raw_truths(ds, n):
    """(n, F, H, W) raw label tiles, scaled per tile as ``PN.raw_tiles`` scales the inputs."""
    t = np.stack([np.stack([np.asarray(f, np.float32) for f in ds.get_label_sample(i % len(ds), transform=False)])
                  for i in range(n)])
    return t * (1.0 + 0.1 * np.arange(n, dtype=np.float32))[:, None, None, None]


def host_tiles(q, tiles, truths, zs):
    """(x, y): the tiles through the painter's HOST transforms, (n, F, H, W) and (n, 1, H, W) float32."""
    y = np.stack([np.asarray(q.transform(t, field=q.input_field, z=float(z)), np.float32).reshape(1, SIZE, SIZE)
                  for t, z in zip(tiles, zs)])
    x = np.stack([np.stack([np.asarray(q.transform(tr[j], field=f, z=float(z)), np.float32).reshape(SIZE, SIZE)
                            for j, f in enumerate(q.label_fields)]) for tr, z in zip(truths, zs)])
    return x, y


def per_tile_reference(q, tiles, truths, zs, seed, ids, draws):
    """((n, 5) of ``model.score`` tile by tile on the host-transformed tiles under the oracle's normals, (n,) limits)."""
    m = q.model
    per_tile = int(np.prod(m.dim_z))
    eps = tile_normals(seed, list(ids), per_tile, L=draws)
    x, y = host_tiles(q, tiles, truths, zs)
    out, limits = [], []
    for i in range(len(tiles)):
        e = np.asarray(eps[:, i], np.float32).reshape(draws, 1, *m.dim_z)
        aux = np.asarray(zs[i:i + 1], np.float32)
        out.append(m.score(torch.from_numpy(x[i:i + 1]), torch.from_numpy(y[i:i + 1]), torch.from_numpy(aux),
                           draws=draws, eps=e).cpu().numpy()[0])
        limits.append(SM.log_weight_limits(m, x[i:i + 1], y[i:i + 1], aux, e)[3].max())
    return np.stack(out), np.array(limits)


def as_array(d):
    assert tuple(d) == S.COLUMNS and all(v.dtype == np.float64 and v.ndim == 1 for v in d.values())
    return np.stack([d[k] for k in S.COLUMNS], axis=1)


def assert_scores_close(got, ref, limits, what):
    err = np.abs(got[:, :4] - ref[:, :4]) / limits[:, None]
    print(what, "columns 0-3: |a - b| / limit of the tile\n", err)
    assert (err <= 1.0).all(), (what, err.max())
    ratio = got[:, 4] / ref[:, 4]
    print(what, "ess ratio - 1", ratio - 1, "limit", np.expm1(4 * limits))
    assert (np.abs(np.log(ratio)) <= 4 * limits).all(), what


@pytest.fixture(scope="module")
def two_heads(tmp_path_factory):
    q = SM.make_painter("two heads", tmp_path_factory.mktemp("ckpt"))
    ds = PN.single_field_dataset()
    tiles, truths = PN.raw_tiles(ds, 5), raw_truths(ds, 5)
    ref, limits = per_tile_reference(q, tiles, truths, ZS, SEED, IDS, K)
    return q, tiles, truths, ref, limits


def test_score_equals_model_score_on_host_transformed_tiles(two_heads):
    """5 tiles at mixed redshifts, 4 draws, batch_size 8: two tiles per batch, a ragged last batch."""
    q, tiles, truths, ref, limits = two_heads
    assert q.can_score() and q.can_score(ZS)
    d = q.score(tiles, truths[:, 0], ZS, draws=K, batch_size=8, tile_ids=IDS, seed=SEED)
    got = as_array(d)
    assert got.shape == (5, 5) and np.isfinite(got).all()
    assert_scores_close(got, ref, limits, "batch 8")
    assert (got[:, 4] >= 1 - 1e-9).all() and (got[:, 4] <= K).all()
    # truths as (N, F, H, W); the same call twice: equal bits
    again = as_array(q.score(tiles, truths, ZS, draws=K, batch_size=8, tile_ids=IDS, seed=SEED))
    assert np.array_equal(again, got)
    # another seed, other ids: other draws
    other = as_array(q.score(tiles, truths, ZS, draws=K, batch_size=8, tile_ids=IDS, seed=SEED + 1))
    assert not np.array_equal(other[:, 0], got[:, 0])


def test_score_does_not_depend_on_batching_or_sharding(two_heads):
    q, tiles, truths, ref, limits = two_heads
    kw = {"draws": K, "tile_ids": IDS, "seed": SEED}
    got = as_array(q.score(tiles, truths, ZS, batch_size=8, **kw))
    wide = as_array(q.score(tiles, truths, ZS, batch_size=16, **kw))
    assert_scores_close(wide, got, limits, "batch 16 against batch 8")
    parts = []
    for rank in range(2):
        d, (lo, hi) = q.score(tiles, truths, ZS, batch_size=8, rank=rank, world_size=2, **kw)
        assert (lo, hi) == ((0, 3), (3, 5))[rank]
        parts.append(as_array(d))
    assert_scores_close(np.concatenate(parts), got, limits, "two ranks against one")


def test_bad_arguments_are_refused(two_heads):
    q, tiles, truths, _, _ = two_heads
    for kw in ({"draws": 3, "batch_size": 8}, {"draws": 0}, {"draws": 65}, {"draws": 16, "batch_size": 8}):
        with pytest.raises(ValueError):
            q.score(tiles, truths, ZS, **kw)
    with pytest.raises(ValueError):
        q.score(tiles[:, :32], truths, ZS, draws=K, batch_size=8)
    with pytest.raises(ValueError):
        q.score(tiles, truths[:4], ZS, draws=K, batch_size=8)


def test_reconstruct_is_the_host_inverse_of_model_reconstruct(two_heads):
    q, tiles, truths, _, _ = two_heads
    m = q.model
    x, y = host_tiles(q, tiles, truths, ZS)
    out = q.reconstruct(tiles, truths, ZS, batch_size=2)
    assert out.shape == q.paint_batch(tiles, ZS).shape == (5, SIZE, SIZE)
    per_tile = int(np.prod(m.dim_z))
    eps = tile_normals(SEED, list(IDS), per_tile, L=1)
    drawn = q.reconstruct(tiles, truths, ZS, batch_size=4, sample=True, seed=SEED, tile_ids=IDS)
    for i in range(5):
        args = (torch.from_numpy(x[i:i + 1]), torch.from_numpy(y[i:i + 1]),
                torch.from_numpy(np.asarray(ZS[i:i + 1], np.float32)))
        for got, e in ((out, None), (drawn, np.asarray(eps[:, i], np.float32).reshape(1, 1, *m.dim_z))):
            net = m.reconstruct(*args, eps=e).cpu().numpy()
            ref = np.asarray(q.inverse_transform(net[0][None], field=q.label_fields[0], z=float(ZS[i])), np.float64)
            # (the limit of tests/test_gpu_pixel_noise_paint.py for the same situation: device against host transforms
            #  in front of the same network)
            PN.assert_stream_equals_per_tile(got[i:i + 1].reshape(1, SIZE, SIZE), ref.reshape(1, SIZE, SIZE), 3e-7,
                                             f"reconstruct tile {i} sample={e is not None}")
    assert not np.array_equal(drawn, out)


def test_bf16_painter_is_scored_as_it_is(two_heads):
    """``dtype="bf16"``: the trunk's slots are bf16, the one-channel tails of the heads are fp32 slots, and those are what
    the score kernels read.  The rounding of a bf16 trunk has no bound here: the score is finite and its identities hold."""
    from baryon_painter_amd.painter import CVAEPainter
    q, tiles, truths, _, _ = two_heads
    b = CVAEPainter(filename=q.checkpoint_files, compute_device="cuda:0", dtype="bf16")
    got = as_array(b.score(tiles[:2], truths[:2], ZS[:2], draws=K, batch_size=8, tile_ids=IDS[:2], seed=SEED))
    assert np.isfinite(got).all() and (got[:, 4] >= 1 - 1e-9).all() and (got[:, 4] <= K).all()
    assert (got[:, 0] >= got[:, 1] - 1e-12 * np.abs(got[:, 1])).all()
    plan = b.model._paint_plans[("score", 2, K)]
    assert plan.h.buf.dtype == torch.bfloat16
    assert plan.mu_head.buf.dtype == plan.var_head.buf.dtype == torch.float32
    assert b.reconstruct(tiles[:2], truths[:2], ZS[:2]).shape == (2, SIZE, SIZE)


def _score_against_reference(q, ds, n, what):
    tiles, truths, zs, ids = PN.raw_tiles(ds, n), raw_truths(ds, n), PN.ZS[:n], IDS[:n]
    ref, limits = per_tile_reference(q, tiles, truths, zs, SEED, ids, K)
    got = as_array(q.score(tiles, truths, zs, draws=K, batch_size=8, tile_ids=ids, seed=SEED))
    assert np.isfinite(got).all()
    assert_scores_close(got, ref, limits, what)
    return tiles, truths, zs


def test_two_field_painter_scores_both_fields(tmp_path):
    """Label fields in two different modes (shift-log-2p, log), the input in a third (log): every field is loaded with
    its own forward record into its channel of the plan's x slot."""
    tr, itr = MF.chains(T)
    ds = BAHAMASDataset(data=MF.data_dict3(), redshifts=list(HC.REDSHIFTS), label_fields=list(MF.LABELS), n_tile=1,
                        n_stack=3, transform=tr, inverse_transform=itr, scale_to_SLICS=True)
    q = SM.settle(PN.build(tmp_path, PN.two_head_architecture(n_fields=2), ds,
                           lambda c: (1.0 - 0.15 * np.arange(c, dtype=np.float32))[None, :, None, None]))
    assert q.can_score()
    tiles, truths, zs = _score_against_reference(q, ds, 3, "two fields")
    with pytest.raises(ValueError):
        q.score(tiles, truths[:, 0], zs, draws=K, batch_size=8)              # one truth for two label fields
    out = q.reconstruct(tiles, truths, zs, batch_size=2)
    assert out.shape == (3, 2, SIZE, SIZE)


def test_log_and_log_tanh_painter(tmp_path):
    fwd, inv = T.create_range_compress_transforms({"dm": 2.0, "pressure": 6.0}, {"dm": "log", "pressure": "log-tanh"},
                                                  eps=1e-3)
    tr = T.chain_transformations([fwd, T.atleast_3d, T.as_float32])
    itr = T.chain_transformations([T.squeeze, inv])
    ds = BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=1,
                        n_stack=3, transform=tr, inverse_transform=itr, scale_to_SLICS=True)
    q = SM.settle(PN.build(tmp_path, PN.two_head_architecture(), ds))
    assert q.can_score()
    _score_against_reference(q, ds, 3, "log / log-tanh")


def test_split_scale_painter_is_refused_before_any_random_number(tmp_path):
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    split, unsplit = T.create_split_scale_transform(3, 4, False)
    tr = T.chain_transformations([fwd, T.as_float32, split, T.atleast_3d])
    itr = T.chain_transformations([unsplit, inv, T.squeeze])
    ds = BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=1,
                        n_stack=3, transform=tr, inverse_transform=itr, n_feature_per_field=3, scale_to_SLICS=True)
    q = PN.build(tmp_path, PN.two_head_architecture(n_scale=3), ds,
                 lambda c: (1.0 - 0.2 * np.arange(c, dtype=np.float32))[None, :, None, None])
    tiles, truths = PN.raw_tiles(ds, 2), raw_truths(ds, 2)
    assert not q.can_score() and q.can_paint_stream()
    plans = len(q.model._paint_plans)
    state = torch.get_rng_state(), torch.cuda.get_rng_state()
    with pytest.raises(NotImplementedError):
        q.score(tiles, truths, PN.ZS[:2], draws=K, batch_size=8)
    with pytest.raises(NotImplementedError):
        q.reconstruct(tiles, truths, PN.ZS[:2])
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])
    assert len(q.model._paint_plans) == plans
