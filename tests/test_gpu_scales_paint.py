"""GPU: a multi-scale CVAE painter (split-scale transform, n_scale = 3, step_size = 4) on the device paint path --
paint_stream against per-tile ``paint`` with the host transforms under the same Philox noise, the (state, meta)
checkpoint round trip, a light-cone plane on the device against the host path, the refusal of chains in another order,
and the single-scale pipeline's launch sequence, which must be what it was before multi-scale painters existed."""
import json
import os

import numpy as np
import pytest
import torch

import host_cases as HC
import scales_ref as R
from baryon_painter_amd import lightcone as LC
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils import synthetic as syn
from baryon_painter_amd.utils.datasets import BAHAMASDataset
from oracle.philox import tile_normals

pytestmark = pytest.mark.gpu

SIZE, N_SCALE, STEP = 64, 3, 4

# tests/test_gpu_paint_pipeline.py compares the single-scale paint_stream with per-tile paint at 3e-7 of the tile's
# maximum: there the two network inputs agree up to one float32 ulp of the transformed tile v (libm's log on either
# side of a rounding boundary), 2^-23 |v| <= 2 u with u = 2^-24 max|v|, and the network carries that to the output.
# Here the inputs are two float32 pyramids of v, SciPy's and the kernel's, each within T u of the exact pyramid
# (T = scales_ref.rounding_count(3) = 16: tests/test_scales_host.py, tests/test_gpu_scales.py), so they agree to 2 T u:
# the input bound is 2 T u / 2 u = T times the single-scale one, and so is the limit.
STREAM_LIMIT = 3e-7 * R.rounding_count(N_SCALE)


def _chains(include_original, order="good"):
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    split, unsplit = T.create_split_scale_transform(N_SCALE, STEP, include_original)
    if order == "good":
        return (T.chain_transformations([fwd, T.as_float32, split, T.atleast_3d]),
                T.chain_transformations([unsplit, inv, T.squeeze]))
    if order == "split first":
        return (T.chain_transformations([T.as_float32, split, fwd, T.as_float32]),
                T.chain_transformations([unsplit, inv, T.squeeze]))
    return (T.chain_transformations([fwd, T.as_float32, split, T.atleast_3d]),        # "inverse swapped"
            T.chain_transformations([inv, unsplit]))


def _painter(tmp, include_original, order="good"):
    from baryon_painter_amd.painter import CVAEPainter
    levels = N_SCALE + int(include_original)
    arch = A.fiducial_architecture(SIZE, n_scale=levels)
    tr, itr = _chains(include_original, order)
    ds = BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=1,
                        n_stack=3, transform=tr, inverse_transform=itr, n_feature_per_field=levels, scale_to_SLICS=True)
    torch.manual_seed(3)
    p = CVAEPainter(training_data_set=ds, test_data_set=ds, architecture=arch, compute_device="cuda:0")
    x, y, aux = syn.synthetic_batch(4, SIZE, SIZE, seed=77)
    scale = (1.0 - 0.2 * np.arange(levels, dtype=np.float32))[None, :, None, None]
    with torch.no_grad():                                  # non-trivial running statistics
        p.model(torch.from_numpy(x * scale), torch.from_numpy(y * scale), torch.from_numpy(aux))
    files = (str(tmp / "state"), str(tmp / "meta"))
    p.save_state_to_file(files)
    q = CVAEPainter(filename=files, compute_device="cuda:0")
    q.checkpoint_files = files
    return q, arch, ds


@pytest.fixture(scope="module", params=[True, False], ids=["with-original", "scales-only"])
def painter(request, tmp_path_factory):
    q, arch, ds = _painter(tmp_path_factory.mktemp("ckpt"), request.param)
    tiles = np.stack([np.asarray(ds.get_input_sample(i % len(ds), transform=False), np.float32) for i in range(7)])
    tiles *= (1.0 + 0.1 * np.arange(7, dtype=np.float32))[:, None, None]
    zs = np.array([0.0, 0.3, 2.0, 0.5, 1.1, 0.0, 0.125])
    return q, arch, tiles, zs, request.param


def test_paint_stream_equals_per_tile_paint_with_host_transforms(painter):
    q, arch, tiles, zs, inc = painter
    assert q.can_paint_stream() and q.model.dim_y[0] == q.model.dim_x[0] == N_SCALE + int(inc)
    seed, ids = 99, np.arange(7, dtype=np.int64) + 1000
    out = q.paint_stream(tiles, zs, batch_size=4, tile_ids=ids, seed=seed)
    assert out.shape == tiles.shape and out.dtype == np.float32 and np.isfinite(out).all()
    g = next(v for k, v in q.model._graphs.items() if isinstance(k, tuple) and "scales" in k)
    assert g["slots"][0]["raw"].shape == (4, 1, SIZE, SIZE) and g["slots"][0]["out"].shape == (4, 1, SIZE, SIZE)
    per_tile = int(np.prod(arch["dim_z"]))
    for i in range(len(tiles)):
        q.model._eps_override = tile_normals(seed, [ids[i]], per_tile).reshape(1, 1, *arch["dim_z"])
        ref = np.asarray(q.paint(tiles[i], z=float(zs[i])), np.float64)
        assert ref.shape == (SIZE, SIZE)
        err, tol = np.abs(out[i] - ref).max(), STREAM_LIMIT * np.abs(ref).max()
        print("tile", i, "err / max|ref|", err / np.abs(ref).max(), "limit", STREAM_LIMIT)
        assert err <= tol, (i, err, tol)
    q.model._eps_override = None
    # batching and sharding do not change a tile
    assert np.array_equal(q.paint_stream(tiles, zs, batch_size=7, tile_ids=ids, seed=seed), out)
    parts = [q.paint_stream(tiles, zs, batch_size=4, tile_ids=ids, seed=seed, rank=r, world_size=2) for r in range(2)]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), out)
    # paint_batch (host transforms) accepts the multi-scale chains as well
    pb = q.paint_batch(tiles[:3], zs[:3], batch_size=3, use_graph=False)
    assert pb.shape == (3, SIZE, SIZE) and np.isfinite(pb).all()
    with pytest.raises(ValueError):
        q.paint_stream(tiles[:, :32], zs)


def test_saved_and_loaded_painter_paints_the_same_bits(painter, tmp_path):
    from baryon_painter_amd.painter import CVAEPainter
    q, arch, tiles, zs, inc = painter
    again = CVAEPainter(filename=q.checkpoint_files, compute_device="cuda:0")
    split = [st for st in again.transform.func.steps if isinstance(st, T._SplitScale)]
    assert len(split) == 1 and (split[0].n_scale, split[0].step_size, split[0].include_original) == (N_SCALE, STEP, inc)
    assert again.can_paint_stream()
    a = q.paint_stream(tiles, zs, batch_size=4, seed=5)
    b = again.paint_stream(tiles, zs, batch_size=4, seed=5)
    assert np.array_equal(a, b)
    again.release_paint_buffers()
    assert not any(isinstance(k, tuple) and "scales" in k for k in again.model._graphs)
    assert np.array_equal(again.paint_stream(tiles, zs, batch_size=4, seed=5), a)       # captured again on next use


def test_device_plane_equals_host_plane(painter):
    """The limit of tests/test_gpu_paint_plane_device.py::test_device_plane_equals_host_plane: both paths paint through
    the same kernels; the blend is float64 on either side."""
    q, arch, tiles, zs, inc = painter
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


@pytest.mark.parametrize("order", ["split first", "inverse swapped"])
def test_chain_in_another_order_has_no_device_form(painter, order):
    q, arch, tiles, zs, inc = painter
    tr, itr = _chains(inc, order)
    good = (q.transform, q.inverse_transform)
    try:
        q.transform = type(good[0])(tr, good[0].stats)
        q.inverse_transform = type(good[1])(itr, good[1].stats)
        n_graphs, n_plans = len(q.model._graphs), len(q.model._plans)
        assert not q.can_paint_stream()
        with pytest.raises(NotImplementedError):
            q.paint_stream(tiles[:2], zs[:2], batch_size=2)
        with pytest.raises(NotImplementedError):
            LC.paint_plane(q, np.ones((100, 100), np.float32), SIZE / 100, SIZE, 0.3, on_device=True)
        assert (len(q.model._graphs), len(q.model._plans)) == (n_graphs, n_plans)         # nothing was captured
    finally:
        q.transform, q.inverse_transform = good
    assert q.can_paint_stream()


def test_levels_must_be_the_models_channels(painter):
    """A split-scale chain on a model with other channel counts: refused before anything is captured."""
    q, arch, tiles, zs, inc = painter
    tr, itr = _chains(not inc)
    good = (q.transform, q.inverse_transform)
    try:
        q.transform = type(good[0])(tr, good[0].stats)
        q.inverse_transform = type(good[1])(itr, good[1].stats)
        assert not q.can_paint_stream()
        with pytest.raises(NotImplementedError):
            q.paint_stream(tiles[:2], zs[:2], batch_size=2)
    finally:
        q.transform, q.inverse_transform = good


class _Recorder:
    """Stands in for the loaded library: every entry point called through it is noted by name."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("bp_") or not callable(fn):
            return fn

        def call(*a, **k):
            self._log.append(name)
            return fn(*a, **k)
        return call


def record_single_scale_sequence(batch=8):
    """(unit names, entry points in call order) of ``paint_graph(batch)`` of a fresh single-scale 64^2 model: what the
    capture of the pipeline (warm-up and two slots) calls.  tests/golden/paint_sequence.json holds this function's
    result on the commit before multi-scale painters."""
    from baryon_painter_amd.models.cvae import CVAE
    torch.manual_seed(11)
    model = CVAE(A.fiducial_architecture(SIZE), "cuda:0")
    model.train(False)
    log = []
    model._lib = _Recorder(model._lib, log)
    g = model.paint_graph(batch)
    torch.cuda.synchronize()
    return {"units": [u.name for u in g["units"]], "entry_points": log}


def test_single_scale_pipeline_launches_what_it_launched_before(painter):
    """Built beside a multi-scale painter: the single-scale pipeline's units and entry points, in order, are those
    recorded before the feature -- bp_paint_load2 / bp_paint_store, none of the new entry points."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paint_sequence.json")) as f:
        before = json.load(f)
    now = record_single_scale_sequence()
    assert now["units"] == before["units"]
    assert now["entry_points"] == before["entry_points"]
    assert "bp_paint_load2" in now["entry_points"] and "bp_paint_store" in now["entry_points"]
    assert not any("scale" in name for name in now["entry_points"])
