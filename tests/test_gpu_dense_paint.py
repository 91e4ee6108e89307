"""GPU: every paint surface with a dense painter -- case (v) of tests/golden/make_goldens_dense.py: a vector latent, the
prior's dense tail and p_z_in's linear head inside the captured paint graph -- on the pattern of
tests/test_gpu_cond_net_paint.py: per-tile paint, paint_batch, the captured pipeline (paint_stream), device planes,
checkpoints.  Philox draws prod(dim_z) = 12 normals per tile under the same (seed, tile id) keys."""
import numpy as np
import pytest
import torch

import host_cases as HC
from baryon_painter_amd import lightcone as LC
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils import synthetic as syn
from baryon_painter_amd.utils.datasets import BAHAMASDataset
from golden import make_goldens_dense as DN
from oracle.philox import tile_normals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def painter_v(tmp_path_factory):
    """(painter with non-trivial running statistics, the same restored from its (state, meta) files, arch, tiles, zs)."""
    from baryon_painter_amd.painter import CVAEPainter
    arch = DN.architectures()["v"]
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    tr = T.chain_transformations([fwd, T.atleast_3d, T.as_float32])
    itr = T.chain_transformations([T.squeeze, inv])
    ds = BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=1,
                        n_stack=3, transform=tr, inverse_transform=itr, scale_to_SLICS=True)
    torch.manual_seed(3)
    p = CVAEPainter(training_data_set=ds, test_data_set=ds, architecture=arch, compute_device="cuda:0")
    x, y, aux = syn.synthetic_batch(4, DN.SIZE, DN.SIZE, seed=77)
    with torch.no_grad():
        p.model(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
    d = tmp_path_factory.mktemp("ckpt_dense")
    files = (str(d / "state"), str(d / "meta"))
    p.save_state_to_file(files)
    q = CVAEPainter(filename=files, compute_device="cuda:0")
    tiles = np.stack([np.asarray(ds.get_input_sample(i % len(ds), transform=False), np.float32) for i in range(6)])
    tiles *= (1.0 + 0.1 * np.arange(6, dtype=np.float32))[:, None, None]
    zs = np.array([0.0, 0.3, 2.0, 0.5, 1.1, 0.125])
    q.checkpoint_files = files
    return p, q, arch, tiles, zs


def _philox_eps(arch, seed, ids):
    per_tile = int(np.prod(arch["dim_z"]))
    return tile_normals(seed, list(ids), per_tile).reshape(1, len(ids), *arch["dim_z"])


def test_dense_painter_surfaces_agree(painter_v):
    """paint_stream, paint_batch(use_graph=True) and per-tile paint with the same noise: 3e-7 of the tile's maximum, the
    tolerance of tests/test_gpu_paint_pipeline.py."""
    p, q, arch, tiles, zs = painter_v
    assert q.can_paint_stream() and q.model.dim_z == (12,)
    assert type(q.model.prior_network[10]).__name__ == "ParamLinear" and type(q.model.p_z_in[0]).__name__ == "ParamLinear"
    seed, ids = 99, np.arange(6, dtype=np.int64) + 1000
    out = q.paint_stream(tiles, zs, batch_size=4, tile_ids=ids, seed=seed)
    assert out.shape == tiles.shape and np.isfinite(out).all()
    for i in range(len(tiles)):
        q.model._eps_override = _philox_eps(arch, seed, [ids[i]])
        ref = np.asarray(q.paint(tiles[i], z=float(zs[i])), np.float64)
        assert np.abs(out[i] - ref).max() <= 3e-7 * np.abs(ref).max(), i
    # the noise matters: another seed paints other tiles
    assert not np.array_equal(q.paint_stream(tiles, zs, batch_size=4, tile_ids=ids, seed=seed + 1), out)
    # paint_batch without the graph, the same Philox noise
    q.model._eps_override = _philox_eps(arch, seed, ids[:4])
    eager = q.paint_batch(tiles[:4], zs[:4], batch_size=4, use_graph=False).reshape(4, *tiles.shape[1:]).astype(np.float64)
    q.model._eps_override = None
    assert np.abs(out[:4] - eager).max() <= 3e-7 * np.abs(eager).max()
    # paint_batch through the captured graph draws its noise in the graph, from torch's generator: an eager draw of the
    # same shape from the same generator state is that noise (see tests/test_gpu_cond_net_paint.py on this property)
    q.paint_batch(tiles[:4], zs[:4], batch_size=4, use_graph=True)                  # (captures)
    torch.manual_seed(21)
    graphed = q.paint_batch(tiles[:4], zs[:4], batch_size=4, use_graph=True).reshape(4, *tiles.shape[1:])
    torch.manual_seed(21)
    q.model._eps_override = torch.randn(size=(1, 4, *arch["dim_z"]), device="cuda").cpu().numpy()
    ref = q.paint_batch(tiles[:4], zs[:4], batch_size=4, use_graph=False).reshape(4, *tiles.shape[1:]).astype(np.float64)
    q.model._eps_override = None
    assert np.isfinite(graphed).all()
    assert np.abs(graphed - ref).max() <= 3e-7 * np.abs(ref).max()
    # sample_P_graphed with a given z of shape (n, 12)
    q.model.train(False)
    y = np.stack([np.asarray(q.transform(t, field=q.input_field, z=float(z))) for t, z in zip(tiles[:4], zs[:4])])
    yt, at = torch.from_numpy(y.reshape(4, *q.model.dim_y)), torch.from_numpy(zs[:4].astype(np.float32))
    zfix = torch.from_numpy(syn.synthetic_eps((4, 12), seed=8))
    a = q.model.sample_P_graphed(yt, aux_label=at, z=zfix)
    b = q.model.sample_P(yt, aux_label=at, z=zfix)
    assert torch.equal(a, b)


def test_device_plane_equals_host_plane(painter_v):
    """As tests/test_gpu_paint_plane_device.py::test_device_plane_equals_host_plane, on a 100^2 plane."""
    q = painter_v[1]
    rng = np.random.Generator(np.random.PCG64(41))
    delta = (np.exp(rng.standard_normal((100, 100)) * 0.5) * 0.05).astype(np.float32)
    host = LC.paint_plane(q, delta, 64 / 100, 64, 0.42, seed=5, batch_size=4)
    dev = LC.paint_plane(q, delta, 64 / 100, 64, 0.42, seed=5, batch_size=4, on_device=True)
    assert dev.shape == host.shape == (100, 100) and dev.dtype == np.float64
    ok = np.isfinite(host)
    assert np.array_equal(np.isfinite(dev), ok) and ok.mean() > 0.9
    assert np.abs(dev[ok] - host[ok]).max() <= 1e-6 * np.abs(host[ok]).max()


def test_checkpoint_reloads_and_paints_the_same_tiles(painter_v):
    p, q, arch, tiles, zs = painter_v
    assert list(q.model.state_dict()) == list(p.model.state_dict())
    assert {"q_out.1.weight", "q_out.1.bias", "q_out.3.weight", "p_z_in.0.weight", "p_z_in.0.bias",
            "prior_network.10.weight"} <= set(q.model.state_dict())
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
