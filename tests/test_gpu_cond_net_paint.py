"""GPU: every paint surface with a p_y_in painter (case a of tests/golden/make_goldens_cond_net.py) and a painter without
a prior network (case c): per-tile paint, paint_batch, the captured pipeline (paint_stream), device planes, checkpoints;
and the kernel sequences of the models that existed before, which must not have moved."""
import json
import os

import numpy as np
import pytest
import torch

import host_cases as HC
from baryon_painter_amd import lightcone as LC
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils import synthetic as syn
from baryon_painter_amd.utils.datasets import BAHAMASDataset
from golden import make_goldens_cond_net as CN
from oracle.philox import tile_normals

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _painters(tag, tmp_path_factory):
    """(painter with non-trivial running statistics, the same restored from its (state, meta) files, arch, tiles, zs)."""
    from baryon_painter_amd.painter import CVAEPainter
    arch = CN.architectures()[tag]
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    tr = T.chain_transformations([fwd, T.atleast_3d, T.as_float32])
    itr = T.chain_transformations([T.squeeze, inv])
    ds = BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=1,
                        n_stack=3, transform=tr, inverse_transform=itr, scale_to_SLICS=True)
    torch.manual_seed(3)
    p = CVAEPainter(training_data_set=ds, test_data_set=ds, architecture=arch, compute_device="cuda:0")
    x, y, aux = syn.synthetic_batch(4, CN.SIZE, CN.SIZE, seed=77)
    with torch.no_grad():
        p.model(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
    d = tmp_path_factory.mktemp("ckpt_" + tag)
    files = (str(d / "state"), str(d / "meta"))
    p.save_state_to_file(files)
    q = CVAEPainter(filename=files, compute_device="cuda:0")
    tiles = np.stack([np.asarray(ds.get_input_sample(i % len(ds), transform=False), np.float32) for i in range(6)])
    tiles *= (1.0 + 0.1 * np.arange(6, dtype=np.float32))[:, None, None]
    zs = np.array([0.0, 0.3, 2.0, 0.5, 1.1, 0.125])
    q.checkpoint_files = files
    return p, q, arch, tiles, zs


@pytest.fixture(scope="module")
def painter_a(tmp_path_factory):
    return _painters("a", tmp_path_factory)


@pytest.fixture(scope="module")
def painter_c(tmp_path_factory):
    return _painters("c", tmp_path_factory)


def _philox_eps(arch, seed, ids):
    per_tile = int(np.prod(arch["dim_z"]))
    return tile_normals(seed, list(ids), per_tile).reshape(1, len(ids), *arch["dim_z"])


def test_p_y_in_painter_surfaces_agree(painter_a):
    """paint_stream, paint_batch(use_graph=True) and per-tile paint with the same noise: 3e-7 of the tile's maximum, the
    tolerance of tests/test_gpu_paint_pipeline.py (host float64 product against its float32 rounding, exp within an ulp)."""
    p, q, arch, tiles, zs = painter_a
    assert q.can_paint_stream() and q.model.p_y_in is not None and q.model.prior_network is not None
    seed, ids = 99, np.arange(6, dtype=np.int64) + 1000
    out = q.paint_stream(tiles, zs, batch_size=4, tile_ids=ids, seed=seed)
    assert out.shape == tiles.shape and np.isfinite(out).all()
    for i in range(len(tiles)):
        q.model._eps_override = _philox_eps(arch, seed, [ids[i]])
        ref = np.asarray(q.paint(tiles[i], z=float(zs[i])), np.float64)
        assert np.abs(out[i] - ref).max() <= 3e-7 * np.abs(ref).max(), i
    # paint_batch without the graph, the same Philox noise
    q.model._eps_override = _philox_eps(arch, seed, ids[:4])
    eager = q.paint_batch(tiles[:4], zs[:4], batch_size=4, use_graph=False).reshape(4, *tiles.shape[1:]).astype(np.float64)
    q.model._eps_override = None
    assert np.abs(out[:4] - eager).max() <= 3e-7 * np.abs(eager).max()
    # paint_batch through the captured graph draws its noise in the graph, from torch's generator: an eager draw of the
    # same shape from the same generator state is that noise.  (That is a property of torch -- a captured randn replays
    # from the generator's seed and offset at replay time, with the eager kernel -- and not one this project promises: if
    # a torch upgrade changes it, this comparison is what has to change, not the painter.  The graphed path's arithmetic
    # is also pinned without it: paint_stream above replays the same captured plans on injected Philox noise.)
    q.paint_batch(tiles[:4], zs[:4], batch_size=4, use_graph=True)                  # (captures)
    torch.manual_seed(21)
    graphed = q.paint_batch(tiles[:4], zs[:4], batch_size=4, use_graph=True).reshape(4, *tiles.shape[1:])
    torch.manual_seed(21)
    q.model._eps_override = torch.randn(size=(1, 4, *arch["dim_z"]), device="cuda").cpu().numpy()
    ref = q.paint_batch(tiles[:4], zs[:4], batch_size=4, use_graph=False).reshape(4, *tiles.shape[1:]).astype(np.float64)
    q.model._eps_override = None
    assert np.isfinite(graphed).all()
    assert np.abs(graphed - ref).max() <= 3e-7 * np.abs(ref).max()


def test_no_prior_paint_stream_equals_paint_batch_with_philox_noise(painter_c):
    p, q, arch, tiles, zs = painter_c
    assert q.can_paint_stream() and q.model.prior_network is None
    seed, ids = 7, np.arange(6, dtype=np.int64)
    ref = q.paint_stream(tiles, zs, batch_size=2, seed=seed)
    assert np.isfinite(ref).all()
    for lo in (0, 3):
        q.model._eps_override = _philox_eps(arch, seed, ids[lo:lo + 3])
        host = q.paint_batch(tiles[lo:lo + 3], zs[lo:lo + 3], batch_size=3, use_graph=False)
        host = host.reshape(3, *tiles.shape[1:]).astype(np.float64)
        assert np.abs(ref[lo:lo + 3] - host).max() <= 3e-7 * np.abs(host).max()
    q.model._eps_override = None
    # a tile's noise depends on (seed, global tile id) only: any batching, any sharding, the same bits
    assert np.array_equal(q.paint_stream(tiles, zs, batch_size=3, seed=seed), ref)
    parts = [q.paint_stream(tiles, zs, batch_size=2, seed=seed, rank=r, world_size=2) for r in range(2)]
    assert parts[0][1][0] == 0 and parts[-1][1][1] == len(tiles)
    assert np.array_equal(np.concatenate([pt[0] for pt in parts]), ref)
    assert not np.array_equal(q.paint_stream(tiles, zs, batch_size=2, seed=seed + 1), ref)


@pytest.mark.parametrize("which", ["a", "c"])
def test_device_plane_equals_host_plane(which, painter_a, painter_c):
    """As tests/test_gpu_paint_plane_device.py::test_device_plane_equals_host_plane, on a 100^2 plane."""
    q = (painter_a if which == "a" else painter_c)[1]
    rng = np.random.Generator(np.random.PCG64(41))
    delta = (np.exp(rng.standard_normal((100, 100)) * 0.5) * 0.05).astype(np.float32)
    host = LC.paint_plane(q, delta, 64 / 100, 64, 0.42, seed=5, batch_size=4)
    dev = LC.paint_plane(q, delta, 64 / 100, 64, 0.42, seed=5, batch_size=4, on_device=True)
    assert dev.shape == host.shape == (100, 100) and dev.dtype == np.float64
    ok = np.isfinite(host)
    assert np.array_equal(np.isfinite(dev), ok) and ok.mean() > 0.9
    assert np.abs(dev[ok] - host[ok]).max() <= 1e-6 * np.abs(host[ok]).max()


@pytest.mark.parametrize("which", ["a", "c"])
def test_checkpoint_reloads_and_paints_the_same_tiles(which, painter_a, painter_c):
    p, q, arch, tiles, zs = painter_a if which == "a" else painter_c
    assert list(q.model.state_dict()) == list(p.model.state_dict())
    assert (q.model.p_y_in is None) == (which == "c") and (q.model.prior_network is None) == (which == "c")
    for k, v in p.model.state_dict().items():
        assert torch.equal(v, q.model.state_dict()[k]), k
    # the painter that wrote the files has no transforms of its own: compare the two networks on transformed tiles
    y = np.stack([np.asarray(q.transform(t, field=q.input_field, z=float(z))) for t, z in zip(tiles[:3], zs[:3])])
    q.model._eps_override = p.model._eps_override = _philox_eps(arch, 13, [0, 1, 2])
    kw = dict(transform=False, inverse_transform=False, batch_size=3, use_graph=False)
    assert np.array_equal(p.paint_batch(y, zs[:3], **kw), q.paint_batch(y, zs[:3], **kw))
    q.model._eps_override = p.model._eps_override = None
    # ... and a second restore of the same files paints the same tiles through the captured pipeline
    from baryon_painter_amd.painter import CVAEPainter
    r = CVAEPainter(filename=q.checkpoint_files, compute_device="cuda:0")
    assert np.array_equal(r.paint_stream(tiles, zs, batch_size=3, seed=13), q.paint_stream(tiles, zs, batch_size=3, seed=13))


def test_L2_paints_with_one_draw_and_is_refused_by_the_captured_pipeline_only(tmp_path_factory):
    p, q, arch, tiles, zs = _painters("b", tmp_path_factory)
    assert q.model.L == 2 and not q.can_paint_stream()
    q.model.train(False)
    with pytest.raises(NotImplementedError, match="captured"):
        q.model.paint_graph(2)
    with pytest.raises(NotImplementedError):
        q.paint_stream(tiles[:2], zs[:2], batch_size=2)
    q.model._eps_override = _philox_eps(arch, 3, [0])
    one = np.asarray(q.paint(tiles[0], z=0.3))
    q.model._eps_override = _philox_eps(arch, 3, [0, 1])
    both = q.paint_batch(tiles[:2], np.array([0.3, 0.5]), batch_size=2, use_graph=False)
    q.model._eps_override = None
    assert one.shape == tiles[0].shape and np.isfinite(one).all() and both.shape[0] == 2
    one, first = one.reshape(tiles.shape[1:]).astype(np.float64), both.reshape(2, *tiles.shape[1:])[0]
    assert np.abs(first - one).max() <= 3e-7 * np.abs(one).max()


def test_split_scale_pipeline_refuses_a_p_y_in_network_before_capture(painter_a):
    """bp_paint_load_scales2 writes two destinations and a p_y_in generator reads one: refused until a one-destination
    form exists, before anything is captured (paint / paint_batch take such a painter through the host transforms)."""
    q = painter_a[1]
    q.model.train(False)
    n_graphs = len(q.model._graphs)
    with pytest.raises(NotImplementedError, match="p_y_in"):
        q.model.paint_graph(2, scales={"n_scale": 1, "step_size": 2.0, "include_original": False})
    # ... and by the painter, for a one-level split-scale chain (whose levels ARE this model's channels)
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    split, unsplit = T.create_split_scale_transform(1, 2.0, False)
    good = (q.transform, q.inverse_transform)
    try:
        q.transform = type(good[0])(T.chain_transformations([fwd, T.as_float32, split, T.atleast_3d]), good[0].stats)
        q.inverse_transform = type(good[1])(T.chain_transformations([unsplit, inv, T.squeeze]), good[1].stats)
        assert not q.can_paint_stream()
        with pytest.raises(NotImplementedError, match="p_y_in"):
            q.paint_stream(painter_a[3][:2], painter_a[4][:2], batch_size=2)
        with pytest.raises(NotImplementedError, match="p_y_in"):
            q._device_paint_parameters(np.zeros(1))
    finally:
        q.transform, q.inverse_transform = good
    assert q.can_paint_stream() and len(q.model._graphs) == n_graphs


# ---------------------------------------------------------------- what existed before launches what it launched
class _Recorder:
    """Stands in for the loaded library: every entry point called through it is noted by name (the mechanism behind
    tests/golden/paint_sequence.json, tests/test_gpu_scales_paint.py)."""

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


def record_paint_sequence(batch=8):
    from baryon_painter_amd.models.cvae import CVAE
    torch.manual_seed(11)
    model = CVAE(A.fiducial_architecture(64), "cuda:0")
    model.train(False)
    log = []
    model._lib = _Recorder(model._lib, log)
    g = model.paint_graph(batch)
    torch.cuda.synchronize()
    return {"units": [u.name for u in g["units"]], "entry_points": log}


def record_train_sequence(L_samples, batch=2):
    """Entry points, in call order, of two training steps (forward + backward) of a fresh fiducial 64^2 model."""
    from baryon_painter_amd.models.cvae import CVAE
    torch.manual_seed(11)
    arch = A.fiducial_architecture(64)
    arch["L"] = L_samples
    model = CVAE(arch, "cuda:0")
    model.train(True)
    log = []
    model._lib = _Recorder(model._lib, log)
    x, y, aux = (torch.from_numpy(t) for t in syn.synthetic_batch(batch, 64, 64, seed=3))
    model._eps_override = syn.synthetic_eps((L_samples, batch, *arch["dim_z"]), seed=4)
    for _ in range(2):
        model.zero_grad()
        (-model(x, y, aux)).backward()
    torch.cuda.synchronize()
    return log


def test_paint_graph_of_a_fiducial_model_launches_what_it_launched_before():
    with open(os.path.join(GOLDEN, "paint_sequence.json")) as f:
        before = json.load(f)
    now = record_paint_sequence()
    assert now["units"] == before["units"]
    assert now["entry_points"] == before["entry_points"]
    assert not any("repeat" in name for name in now["entry_points"])


@pytest.mark.parametrize("L_samples", [1, 2])
def test_training_step_of_a_fiducial_model_launches_what_it_launched_before(L_samples):
    """tests/golden/train_sequence.json: ``record_train_sequence`` on the commit before p_y_in networks."""
    with open(os.path.join(GOLDEN, "train_sequence.json")) as f:
        before = json.load(f)[f"L{L_samples}"]
    now = record_train_sequence(L_samples)
    assert now == before
    assert not any("repeat" in name for name in now)


if __name__ == "__main__":
    # PYTHONPATH=. python tests/test_gpu_cond_net_paint.py   (on a GPU, on the commit whose sequences are to be pinned): rewrites
    # tests/golden/train_sequence.json, as tests/golden/paint_sequence.json was written from test_gpu_scales_paint.py
    with open(os.path.join(GOLDEN, "train_sequence.json"), "w") as f:
        json.dump({f"L{ls}": record_train_sequence(ls) for ls in (1, 2)}, f)
