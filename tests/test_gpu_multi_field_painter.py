"""GPU: a CVAE painter with two label fields in two different range-compression modes (tests/multi_field_cases.py), one
with single-channel fields and one with split-scale fields (levels = 2, dim_x[0] = 4), on every paint surface:
``paint_stream`` against per-tile ``paint``, batching and sharding, the checkpoint round trip, the reference fixture
(tests/golden/multi_field.npz), device planes against host planes, the light cone's ``field=``, and a single-field
painter whose results and graph keys stay what they were.  On the commit before, these painters raise
NotImplementedError from ``paint`` and answer ``can_paint_stream() == False``."""
import os

import numpy as np
import pytest
import torch

import host_cases as HC
import multi_field_cases as MF
import range_modes_ref as R
import scales_ref
from baryon_painter_amd import lightcone as LC
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils import synthetic as syn
from baryon_painter_amd.utils.datasets import BAHAMASDataset
from oracle.philox import tile_normals

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SIZE, F = MF.SIZE, len(MF.LABELS)
KINDS = {"single scale": None, "split scale": (2, 4, False)}


def _build(kind, tmp, labels=MF.LABELS):
    """A 64^2 fiducial painter of ``labels``, loaded from (state, meta) files as in tests/test_gpu_range_modes.py."""
    from baryon_painter_amd.painter import CVAEPainter
    scales = KINDS[kind]
    levels = 1 if scales is None else scales[0] + int(scales[2])
    tr, itr = MF.chains(T, scales=scales)
    ds = BAHAMASDataset(data=MF.data_dict3(), redshifts=list(HC.REDSHIFTS),
                        label_fields=list(labels), n_tile=1, n_stack=3, transform=tr, inverse_transform=itr,
                        n_feature_per_field=levels, scale_to_SLICS=True)
    arch = A.fiducial_architecture(SIZE, n_fields=len(labels), n_scale=levels)
    torch.manual_seed(3)
    p = CVAEPainter(training_data_set=ds, test_data_set=ds, architecture=arch, compute_device="cuda:0")
    x, y, aux = syn.synthetic_batch(4, SIZE, SIZE, seed=77)
    sx = (1.0 - 0.15 * np.arange(arch["dim_x"][0], dtype=np.float32))[None, :, None, None]
    sy = (1.0 - 0.2 * np.arange(levels, dtype=np.float32))[None, :, None, None]
    with torch.no_grad():                                  # non-trivial running statistics
        p.model(torch.from_numpy(x * sx), torch.from_numpy(y * sy), torch.from_numpy(aux))
    files = (str(tmp / "state"), str(tmp / "meta"))
    p.save_state_to_file(files)
    q = CVAEPainter(filename=files, compute_device="cuda:0")
    q.checkpoint_files = files
    tiles = np.stack([np.asarray(ds.get_input_sample(i % len(ds), transform=False), np.float32) for i in range(5)])
    tiles *= (1.0 + 0.1 * np.arange(5, dtype=np.float32))[:, None, None]
    tiles[0, 0, :2] = (0.0, -0.05)                         # the forward branch values of "log" on the way in
    return q, tiles, np.array([0.0, 0.3, 2.5, 0.5, -0.2])


@pytest.fixture(scope="module")
def painters(tmp_path_factory):
    """kind -> (painter, raw tiles, redshifts), built once per kind."""
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = _build(kind, tmp_path_factory.mktemp("ckpt"))
        return cache[kind]
    return get


@pytest.mark.parametrize("kind", list(KINDS))
def test_paint_stream_equals_per_tile_paint_per_field(painters, kind):
    """5 tiles at batch 2 (a short last batch) against per-tile ``paint`` under the oracle's Philox normals, per tile and
    per field.  The limit is that of tests/test_gpu_range_modes.py
    (test_paint_stream_equals_per_tile_paint_with_host_transforms), derived per field from the field's own mode: 3e-7 of
    the largest pixel for the network between two inputs that agree to one float32 ulp of the transformed tile -- times
    scales_ref.rounding_count(n_scale) where the inputs are two float32 pyramids of it, as in
    tests/test_gpu_scales_paint.py -- plus 4 x the host float32 inverse's own worst error against the formula in float64
    on this tile's activations, plus the formula's response to 4 float32 ulps of the activation."""
    q, tiles, zs = painters(kind)
    scales = KINDS[kind]
    levels = 1 if scales is None else scales[0] + int(scales[2])
    assert q.can_paint_stream() and q.model.dim_x[0] == F * levels and q.model.dim_y[0] == levels
    seed, ids = 99, np.arange(5, dtype=np.int64) + 1000
    out = q.paint_stream(tiles, zs, batch_size=2, tile_ids=ids, seed=seed)
    assert out.shape == (5, F, SIZE, SIZE) and out.dtype == np.float32
    key, g = next((k, v) for k, v in q.model._graphs.items() if isinstance(k, tuple) and "fields" in k)
    assert key[-F - 3:] == ("modes", T.MODE_IDS[MF.MODES["dm"]], "fields") + tuple(T.MODE_IDS[MF.MODES[f]] for f in MF.LABELS)
    sl = g["slots"][0]
    assert sl["xf_in"].shape == (2, 4) and sl["xf_out"].shape == (2, 4 * F) and sl["out"].shape == (2, F, SIZE, SIZE)
    assert sl["raw"].shape == (2, 1, SIZE, SIZE)
    network = 3e-7 * (1 if scales is None else scales_ref.rounding_count(scales[0]))
    per_tile = int(np.prod(q.model.dim_z))
    for i in range(len(tiles)):
        q.model._eps_override = tile_normals(seed, [ids[i]], per_tile).reshape(1, 1, *q.model.dim_z)
        with np.errstate(invalid="ignore"):                       # (the host's np.where evaluates log at the pixel below 0)
            ref = np.asarray(q.paint(tiles[i], z=float(zs[i])), np.float64)
            head = np.asarray(q.paint(tiles[i], z=float(zs[i]), inverse_transform=False), np.float32)
        assert ref.shape == (F, SIZE, SIZE) and head.shape == (1, F * levels, SIZE, SIZE) and np.isfinite(ref).all()
        for j, f in enumerate(MF.LABELS):
            act = head[0, j * levels:(j + 1) * levels].sum(axis=0) if levels > 1 else head[0, j]
            assert act.dtype == np.float32
            s = T.interpolate_z(q.inverse_transform.stats[f], float(zs[i]))
            args = (MF.MODES[f], MF.K_VALUES[f], np.sqrt(s["var"]), np.sqrt(s["mean"]), MF.EPS)
            exact = R.inverse_f64(*args, act)
            host_err = np.abs(ref[j] - exact).max()
            moved = np.abs(R.inverse_f64(*args, act + 4 * np.spacing(act)) - exact).max()
            scale = np.abs(ref[j]).max()
            tol = network * scale + 4 * host_err + moved
            err = np.abs(out[i, j] - ref[j]).max()
            print(kind, "tile", i, f, "err / max|ref|", err / scale, "limit / max|ref|", tol / scale)
            assert err <= tol, (i, f, err, tol)
    q.model._eps_override = None
    # the two fields are two different tiles
    assert not np.array_equal(out[:, 0], out[:, 1])
    # paint_batch slices the same way
    pb = q.paint_batch(tiles[:3], zs[:3], batch_size=3, use_graph=False)
    assert pb.shape == (3, F, SIZE, SIZE) and np.isfinite(pb).all()


@pytest.mark.parametrize("kind", list(KINDS))
def test_result_does_not_depend_on_batches_or_ranks(painters, kind):
    q, tiles, zs = painters(kind)
    seed, ids = 99, np.arange(5, dtype=np.int64) + 1000
    out = q.paint_stream(tiles, zs, batch_size=2, tile_ids=ids, seed=seed)
    assert np.array_equal(q.paint_stream(tiles, zs, batch_size=5, tile_ids=ids, seed=seed), out)
    parts = [q.paint_stream(tiles, zs, batch_size=2, tile_ids=ids, seed=seed, rank=r, world_size=2) for r in range(2)]
    assert [p[1] for p in parts] == [(0, 3), (3, 5)] and parts[1][0].shape == (2, F, SIZE, SIZE)
    assert np.array_equal(np.concatenate([p[0] for p in parts]), out)
    # out=: a pinned tensor of the result's shape is filled in place; another shape is refused
    dst = torch.empty((5, F, SIZE, SIZE), dtype=torch.float32).pin_memory()
    assert q.paint_stream(tiles, zs, batch_size=2, tile_ids=ids, seed=seed, out=dst) is dst
    assert np.array_equal(dst.numpy(), out)
    with pytest.raises(ValueError, match="out"):
        q.paint_stream(tiles, zs, batch_size=2, out=torch.empty((5, SIZE, SIZE)).pin_memory())
    assert all(k[-1] == F for k in q._paint_host_buffers)


@pytest.mark.parametrize("kind", list(KINDS))
def test_saved_and_loaded_painter_paints_the_same_bits(painters, kind):
    from baryon_painter_amd.painter import CVAEPainter
    q, tiles, zs = painters(kind)
    again = CVAEPainter(filename=q.checkpoint_files, compute_device="cuda:0")
    assert again.label_fields == list(MF.LABELS) and again.can_paint_stream()
    a = q.paint_stream(tiles, zs, batch_size=2, seed=5)
    assert np.array_equal(again.paint_stream(tiles, zs, batch_size=2, seed=5), a)


def test_sample_P_and_the_per_field_inverse_match_the_reference_fixture():
    """The reference's ``sample_P(y, aux, z=given)`` of the two-field 64^2 network and its own inverses per field: the
    head to the x_mu limit of the cond-net parity tests (relative L2 <= 1e-4), and the physical tiles of either field
    to the same limit."""
    from baryon_painter_amd.models.cvae import CVAE
    gold = np.load(os.path.join(HERE, "golden", "multi_field.npz"))
    arch = MF.architecture(A)
    m = CVAE(arch, "cuda:0")
    named = dict(m.named_parameters())
    names = str(gold["params"]).split(",")
    assert sorted(names) == sorted(named)
    vals = syn.fill_params({k: tuple(named[k].shape) for k in names}, MF.SEED_W)
    with torch.no_grad():
        for k in names:
            named[k].copy_(torch.from_numpy(vals[k]))
    y, aux, z = MF.fixture_inputs(arch, syn)
    assert np.array_equal(y, gold["y"]) and np.array_equal(aux, gold["aux"]) and np.array_equal(z, gold["z"])
    m.train(False)
    head = m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux), z=z).cpu().numpy()
    assert head.shape == gold["head"].shape == (MF.BATCH, F, SIZE, SIZE)

    def rel_l2(a, ref):
        a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
        return float(np.sqrt(((a - ref) ** 2).sum() / (ref ** 2).sum()))
    print("head rel l2", rel_l2(head, gold["head"]))
    assert rel_l2(head, gold["head"]) <= 1e-4
    _, inv = T.create_range_compress_transforms(MF.K_VALUES, MF.MODES, eps=MF.EPS, sqrt_of_mean=True)
    for n in range(MF.BATCH):
        phys = MF.inverse_fields(inv, head[n], float(MF.FIXTURE_Z[n]), MF.stats())
        for j, f in enumerate(MF.LABELS):
            print("tile", n, f, "rel l2", rel_l2(phys[j], gold["physical"][n, j]))
            assert rel_l2(phys[j], gold["physical"][n, j]) <= 1e-4


def _delta():
    rng = np.random.Generator(np.random.PCG64(41))
    return (np.exp(rng.standard_normal((160, 160)) * 0.5) * 0.05).astype(np.float32)


@pytest.mark.parametrize("kind", list(KINDS))
def test_device_plane_equals_host_plane_per_field(painters, kind):
    """The limit of tests/test_gpu_paint_plane_device.py: both paths paint through the same kernels and blend in
    float64.  The finite pixels are counted on the host path's plane."""
    q, tiles, zs = painters(kind)
    delta, rel, z = _delta(), SIZE / 160, 0.42
    host = LC.paint_plane(q, delta, rel, SIZE, z, seed=5, batch_size=4)
    dev = LC.paint_plane(q, delta, rel, SIZE, z, seed=5, batch_size=4, on_device=True)
    assert dev.shape == host.shape == (F, 160, 160) and dev.dtype == host.dtype == np.float64
    for j, f in enumerate(MF.LABELS):
        ok = np.isfinite(host[j])
        assert np.array_equal(np.isfinite(dev[j]), ok) and ok.mean() > 0.9
        err, scale = np.abs(dev[j][ok] - host[j][ok]).max(), np.abs(host[j][ok]).max()
        print(kind, f, "plane err / scale", err / scale)
        assert err <= 1e-6 * scale
    assert not np.array_equal(host[0], host[1])
    out = torch.full((F, 160, 160), float("nan"), dtype=torch.float64, device="cuda")
    assert LC.paint_plane(q, delta, rel, SIZE, z, seed=5, batch_size=4, on_device=True, out=out) is out
    assert np.array_equal(out.cpu().numpy(), dev, equal_nan=True)
    with pytest.raises(ValueError, match="out"):
        LC.paint_plane(q, delta, rel, SIZE, z, seed=5, batch_size=4, on_device=True, out=out[0])


def test_light_cone_projects_the_named_fields_device_plane(painters):
    q, tiles, zs = painters("single scale")
    delta, z = _delta(), 0.42
    args = dict(z=[z], delta_size=[160.0], tile_size=float(SIZE), n_pixel_tile=SIZE, resolution=48, scales=[0.7],
                batch_size=4, seed=5)
    planes = LC.paint_plane(q, delta, SIZE / 160, SIZE, z, seed=5, batch_size=4, on_device=True)
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="field"):
        LC.paint_light_cone(q, [delta], on_device=True, **args)
    assert torch.equal(torch.get_rng_state(), state)
    for j, f in enumerate(MF.LABELS):
        y_map, kept = LC.paint_light_cone(q, [delta], on_device=True, field=f, return_planes=True, **args)
        assert np.array_equal(kept[0], planes[j], equal_nan=True)
        want = LC.project_planes([planes[j]], [0.7], 48, on_device=True)
        assert y_map.shape == (48, 48) and np.array_equal(y_map, want)


def test_single_field_painter_is_unchanged(tmp_path_factory):
    """One label field of the same transforms: (N, H, W) tiles, (n_plane, n_plane) planes, and the graph key of the
    commit before -- (batch, "pipeline", "modes", input mode, label mode), no further element."""
    q, tiles, zs = _build("single scale", tmp_path_factory.mktemp("one"), labels=("pressure",))
    assert q.label_fields == ["pressure"] and q.model.dim_x[0] == 1
    out = q.paint_stream(tiles, zs, batch_size=2, seed=5)
    assert out.shape == (5, SIZE, SIZE) and out.dtype == np.float32
    keys = [k for k in q.model._graphs if isinstance(k, tuple) and "pipeline" in k]
    assert keys == [(2, "pipeline", "modes", T.MODE_IDS["log"], T.MODE_IDS["shift-log-2p"])]
    sl = q.model._graphs[keys[0]]["slots"][0]
    assert sl["xf_out"].shape == (2, 4) and sl["out"].shape == (2, 1, SIZE, SIZE)
    assert list(q._paint_host_buffers) == [(2, SIZE, SIZE, q.model._graphs[keys[0]]["block_bytes"], "cuda:0")]
    assert q.paint(tiles[1], z=0.3).shape == (SIZE, SIZE)
    plane = LC.paint_plane(q, _delta(), SIZE / 160, SIZE, 0.42, seed=5, batch_size=4, on_device=True)
    assert plane.shape == (160, 160)
