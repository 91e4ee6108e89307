"""GPU: the CGAN painter with ``paint_dtype="bf16"`` (models/cgan.py _GanPaintPlan: the 128-channel trunk on the bf16
matrix-core kernels) -- accuracy against the float64 generator, and the properties the fp32 paint path has.

Yardstick (the rule tests/test_gpu_parity_r3.py applies to the CVAE's bf16 mode): truth is the float64 generator on the
same weights; the comparison is the float64 ROUNDING TWIN of tests/cgan_bf16_ref.py, rounded to bf16 where the plan
stores or stages bf16.  Relative L2 over the network-domain (tanh) output:

    device error against truth  <=  max(2 x twin error against truth, 5e-3).

The twin's own error is printed, not fixed in advance.  Tile 64 runs with two residual blocks; tile 512 with one block
at batch 2, once: only there the trunk is 128 pixels wide and the plan reaches the column-strip kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

import cgan_bf16_ref as R
from baryon_painter_amd import _lib as L
from baryon_painter_amd import lightcone as LC
from baryon_painter_amd.utils import datasets as D

pytestmark = pytest.mark.gpu

TILE = 64
REDSHIFTS = np.array([-0.2, 0.0, 0.06, 0.125, 0.3, 0.77, 1.0, 1.6, 2.0, 2.5, 3.1])


def _painter(ds, tile, n_res, seed, **kw):
    from baryon_painter_amd.painter import CGANPainter
    torch.manual_seed(seed)
    return CGANPainter(training_data_set=ds, tile_size=tile, compute_device="cuda:0", n_res=n_res, **kw)


@pytest.fixture(scope="module")
def painters(tmp_path_factory):
    """Two 64^2, two-block painters from the same seed, bf16 and fp32 paint, each trained for two iterations (batch-norm
    running statistics off their initial values) with the training logs; the bf16 one restored from its checkpoint."""
    from baryon_painter_amd.painter import CGANPainter
    ds = D.SyntheticTileDataset(n_sample=16, tile_size=TILE, seed=3)
    pb = _painter(ds, TILE, 2, 4, paint_dtype="bf16")
    log_b = pb.train(n_iter=2, batch_size=2)
    pf = _painter(ds, TILE, 2, 4)
    log_f = pf.train(n_iter=2, batch_size=2)
    d = tmp_path_factory.mktemp("cgan_bf16_ckpt")
    files = (str(d / "state"), str(d / "meta"))
    pb.save_state_to_file(files)
    q = CGANPainter(filename=files, compute_device="cuda:0")
    tiles = np.stack([ds.raw_fields(i)[0] for i in range(len(REDSHIFTS))])
    return {"bf16": pb, "fp32": pf, "restored": q, "logs": (log_b, log_f), "tiles": tiles, "zs": REDSHIFTS, "ds": ds}


def _accuracy(p, tiles, zs):
    """(device error, twin error) against the float64 generator, relative L2 over the tanh-domain output."""
    m = p.model
    m.train(False)
    y = np.stack([p.transform(t, "dm", float(z)) for t, z in zip(tiles, zs)])[:, None]
    dev = m.generate(torch.from_numpy(y), torch.tensor(zs, dtype=torch.float32)).cpu()
    P = R.parameters(m.g_arch, m.d_arch, {k: v.detach().cpu() for k, v in m.state_dict().items()})
    truth = R.truth(m.g_arch, P, y, zs)
    twin = R.twin(m.g_arch, P, y, zs)
    assert np.isfinite(dev.numpy()).all()
    return R.rel_l2(dev, truth), R.rel_l2(twin, truth)


def test_bf16_plan_runs_the_trunk_in_bf16(painters):
    p = painters["bf16"]
    p.model.train(False)
    plan = p.model._paint_plan(3)
    bf = [u.name for u in plan.units if u.bf16]
    assert bf == ["generator.6", "generator.9.res_block.0", "generator.9.res_block.3", "generator.10.res_block.0",
                  "generator.10.res_block.3", "generator.11"]
    by = {u.name: u for u in plan.units}
    assert by["generator.6"].inp.dt == L.F32 and by["generator.6"].out.dt == L.BF16
    assert by["generator.11"].inp.dt == L.BF16 and by["generator.11"].out.dt == L.F32
    assert all(u.out.dt == L.F32 for u in plan.units if not u.bf16)
    # the training plan ignores the keyword
    assert not any(u.bf16 for g in p.model._plan(2).g_units for u in (g.body if hasattr(g, "body") else [g]))
    assert (3, "bf16") in p.model._paint_plans and 3 not in p.model._paint_plans
    p.model._plans.clear()


def test_accuracy_at_tile_64(painters):
    p = painters["bf16"]
    e_dev, e_twin = _accuracy(p, painters["tiles"][:4], painters["zs"][3:7])
    e_f32, _ = _accuracy(painters["fp32"], painters["tiles"][:4], painters["zs"][3:7])
    print(f"tile 64, 2 blocks: device {e_dev:.3e}  twin {e_twin:.3e}  fp32 plan {e_f32:.3e}")
    assert e_dev <= max(2 * e_twin, 5e-3)
    assert e_f32 < e_dev, "the fp32 plan is closer to the truth than the bf16 plan: otherwise bf16 never ran"


def test_accuracy_at_tile_512_through_the_strip_kernel():
    ds = D.SyntheticTileDataset(n_sample=4, tile_size=512, seed=5)
    p = _painter(ds, 512, 1, 9, paint_dtype="bf16")
    p.model.train(False)
    lib = p.model._lib
    plan = p.model._paint_plan(2)
    for u in plan.units:
        if ".res_block." in u.name:
            assert u.bf16 and u.out.w == 128
            assert lib.bp_conv_ws_kind(C.byref(u.cv), L.PACK_FWD, C.byref(u.inp.view), C.byref(u.out.view)) == 3
    tiles = np.stack([ds.raw_fields(i)[0] for i in range(2)])
    e_dev, e_twin = _accuracy(p, tiles, np.array([0.1, 0.9]))
    print(f"tile 512, 1 block, batch 2: device {e_dev:.3e}  twin {e_twin:.3e}")
    assert e_dev <= max(2 * e_twin, 5e-3)
    p.release_paint_buffers()


def test_paint_stream_is_independent_of_batching_and_sharding(painters):
    p, tiles, zs = painters["bf16"], painters["tiles"], painters["zs"]
    ref = p.paint_stream(tiles, zs, batch_size=4)
    assert ref.shape == (11, TILE, TILE) and np.isfinite(ref).all()
    assert np.array_equal(p.paint_stream(tiles, zs, batch_size=11), ref)
    assert np.array_equal(p.paint_stream(tiles, zs, batch_size=3), ref)
    parts = [p.paint_stream(tiles, zs, batch_size=4, rank=r, world_size=2) for r in range(2)]       # (tiles, (first, last))
    assert parts[0][1][0] == 0 and parts[0][1][1] == parts[1][1][0] and parts[1][1][1] == len(tiles)
    assert np.array_equal(np.concatenate([a[0] for a in parts]), ref)
    # ... and it is not the fp32 painter's result
    assert not np.array_equal(painters["fp32"].paint_stream(tiles, zs, batch_size=4), ref)


def test_fp32_keyword_is_the_painter_of_before(painters):
    ds, tiles, zs = painters["ds"], painters["tiles"], painters["zs"]
    a = _painter(ds, TILE, 2, 21)
    b = _painter(ds, TILE, 2, 21, paint_dtype="fp32")
    assert a.model.paint_dtype == b.model.paint_dtype == "fp32"
    assert np.array_equal(a.paint_stream(tiles, zs, batch_size=4), b.paint_stream(tiles, zs, batch_size=4))
    with pytest.raises(ValueError):
        _painter(ds, TILE, 2, 21, paint_dtype="fp16")


def test_device_plane_equals_host_plane(painters):
    p = painters["bf16"]
    rng = np.random.Generator(np.random.PCG64(41))
    delta = (np.exp(rng.standard_normal((150, 150)) * 0.5) * 0.05).astype(np.float32)
    rel, z = TILE / 150, 0.42
    host = LC.paint_plane(p, delta, rel, TILE, z, seed=5, batch_size=4)
    dev = LC.paint_plane(p, delta, rel, TILE, z, seed=5, batch_size=4, on_device=True)
    ok = np.isfinite(host)
    assert np.array_equal(np.isfinite(dev), ok) and ok.mean() > 0.9
    assert np.array_equal(dev[ok], host[ok]), np.abs(dev[ok] - host[ok]).max()       # cut == tile: the same bits


def test_checkpointed_bf16_painter_paints_the_same_bits(painters):
    p, q, tiles, zs = painters["bf16"], painters["restored"], painters["tiles"], painters["zs"]
    assert q.paint_dtype == "bf16" and q.model.paint_dtype == "bf16" and (q.tile_size, q.n_res) == (TILE, 2)
    assert np.array_equal(q.paint_stream(tiles, zs, batch_size=4), p.paint_stream(tiles, zs, batch_size=4))


def test_training_ignores_paint_dtype_and_painting_survives_it(painters):
    log_b, log_f = painters["logs"]
    assert len(log_b) == 2 and log_b == log_f, (log_b, log_f)          # the same losses bit for bit
    # the bf16 painter paints after its two training iterations (every test above), also once its buffers were dropped
    p, tiles, zs = painters["bf16"], painters["tiles"], painters["zs"]
    a = p.paint_stream(tiles[:3], zs[:3], batch_size=3)
    p.release_paint_buffers()
    assert not p.model._paint_plans and not p.model._paint_graphs
    assert np.isfinite(a).all() and np.array_equal(p.paint_stream(tiles[:3], zs[:3], batch_size=3), a)
