"""GPU: device batch assembly for multi-scale and minimum-subtracted training sets -- bp_tile_minima and
bp_gather_tiles_scales behind ``DeviceTileAssembler`` / ``CVAEPainter.use_device_assembly()``.

  1. the per-tile minimum: ``get_batch`` of a ``subtract_minimum`` set bit-equal to the host dataset, all 8 permutation
     codes, a NaN in one tile;
  2. the pyramid stage alone: bp_gather_tiles_scales == bp_split_scale(bp_gather_tiles) rewritten NCHW, bit for bit;
  3. the assembled multi-scale batch against the reference's dataset[idx] (tests/golden/assemble.npz);
  4. one training step fed by the assembler against the same step fed by the host dataset's tensors;
  5. a single-scale set without subtract_minimum: the tensors of a direct bp_gather_tiles call."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import assemble_cases as AC
import gpu_util as G
import host_cases as HC
import scales_ref as R
from baryon_painter_amd import _lib as L
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils import synthetic as syn
from baryon_painter_amd.utils.datasets import BAHAMASDataset, DeviceTileAssembler

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REDSHIFTS = [0.0, 0.5]


def stacks(grid, seed, n_stack=3):
    """``data=`` of a BAHAMASDataset: seeded positive float32 stacks (n_stack, grid, grid) per field, redshift, slab."""
    rng = np.random.Generator(np.random.PCG64([seed, grid]))
    data = {}
    for f, amp in (("dm", 5.0e3), ("pressure", 0.05)):
        data[f] = {}
        for z in REDSHIFTS:
            data[f][z] = {"100": (rng.random((n_stack, grid, grid), dtype=np.float32) * amp + 0.01 * amp),
                          "150": (rng.random((n_stack, grid, grid), dtype=np.float32) * amp + 0.02 * amp),
                          "mean_100": 0.5 * amp, "mean_150": 0.5 * amp, "var_100": amp * amp / 12,
                          "var_150": amp * amp / 12}
    return data


GRIDS = {16: (64, 4), 48: (96, 2), 64: (128, 2), 80: (160, 2)}          # tile -> (n_grid, n_tile)


def tile_dataset(tile, transform=None, sub=False, data=None, **kw):
    grid, n_tile = GRIDS[tile]
    args = dict(data=data or stacks(grid, 5), redshifts=REDSHIFTS, label_fields=["pressure"], n_tile=n_tile, n_stack=2,
                stack_offset=1, tile_permutations=True, scale_to_SLICS=True, subtract_minimum=sub, fixed_indexing=True)
    args.update(kw)
    if transform is not None:
        args["transform"] = transform
    ds = BAHAMASDataset(**args)
    assert ds.tile_size == tile
    return ds


def permutation_indices(ds):
    """16 indices in which each slab takes every one of the 8 permutation codes, on changing tiles and redshifts."""
    block = ds.n_sample // 64
    idx = [p * 8 * block + (7 * p + 3) % block for p in range(8)] + \
          [ds.n_sample + p * block + (11 * p + 5) % block for p in range(8)]
    perms = np.array([ds.sample_idx_to_tile_permutation(i) for i in idx])
    assert set(perms[:, 0]) == set(perms[:, 1]) == set(range(8))
    return idx


# ---------------------------------------------------------------------------------------------- 1. the minimum
@pytest.mark.parametrize("tile", [16, 64])
def test_subtract_minimum_batch_is_bit_equal_to_the_host_dataset(tile):
    grid, _ = GRIDS[tile]
    data = stacks(grid, 9)
    probe = tile_dataset(tile, sub=True, data=data)
    idx = permutation_indices(probe)
    # a NaN in the 100-slab tile of sample idx[5] (written before the assembler uploads the stacks)
    z = probe.sample_idx_to_redshift(idx[5])
    s100, y100, x100 = probe.sample_idx_to_tile(idx[5])[:3]
    data["dm"][z]["100"][s100, y100 * tile + 3, x100 * tile + tile - 2] = np.nan
    ds = tile_dataset(tile, sub=True, data=data)             # transform: the identity (the default)
    asm = DeviceTileAssembler(ds, "cuda:0")
    assert asm.mode is None and asm.scales is None
    x, y, zs = asm.get_batch(idx)
    assert x.shape == y.shape == (len(idx), 1, tile, tile)
    n_nan = 0
    for n, i in enumerate(idx):
        (dm, pr), _, zz = ds[i]
        assert dm.dtype == np.float32 and float(zs[n]) == np.float32(zz)
        got = y[n, 0].cpu().numpy()
        if np.isnan(dm).any():                               # np.min propagates the NaN: the whole tile is NaN
            assert np.isnan(dm).all() and np.isnan(got).all()
            n_nan += 1
        else:
            assert dm.min() == 0 and np.array_equal(got, dm), i
        assert np.array_equal(x[n, 0].cpu().numpy(), pr), i    # the label field keeps its minimum
    assert n_nan >= 1
    # the minima themselves, through the C ABI
    lib = L.load()
    d100, d150, xf = (torch.from_numpy(a.view(np.uint8)).cuda() for a in asm._descriptors("dm", idx))
    mn = torch.full((len(idx),), -1.0, device="cuda")
    assert lib.bp_tile_minima(L.ptr(d100), L.ptr(d150), L.ptr(xf), len(idx), tile, L.ptr(mn), G.stream()) == L.BP_OK
    raw = tile_dataset(tile, sub=False, data=data)
    ref = np.array([np.min(raw.get_input_sample(i, transform=False)) for i in idx], np.float32)
    assert np.array_equal(mn.cpu().numpy(), ref, equal_nan=True) and np.isnan(ref).sum() == n_nan
    assert lib.bp_tile_minima(None, L.ptr(d150), L.ptr(xf), len(idx), tile, L.ptr(mn), G.stream()) == L.BP_EINVAL


# ---------------------------------------------------------------------------------------------- 2. the pyramid stage
def _tables(n_scale, step=4):
    radii, w = T.split_scale_tables(n_scale, step, 3.0)
    return (G.dev(w, torch.float64) if len(w) else None), (C.c_int32 * len(radii))(*radii), radii


def _gather_scales(desc, minima, n, tile, n_scale, inc, step=4, ws_bytes=None):
    lib = L.load()
    wd, radii, _ = _tables(n_scale, step)
    ws = int(lib.bp_gather_tiles_scales_workspace(n, tile, n_scale))
    scratch = torch.empty(max(ws // 4, 1), device="cuda")
    out = torch.full((n, n_scale + inc, tile, tile), float("nan"), device="cuda")
    rc = lib.bp_gather_tiles_scales(L.ptr(desc[0]), L.ptr(desc[1]), L.ptr(desc[2]), L.ptr(minima), n, tile, n_scale, inc,
                                    L.ptr(wd), radii, L.ptr(scratch), ws if ws_bytes is None else ws_bytes, L.ptr(out),
                                    G.stream())
    torch.cuda.synchronize()
    return rc, out


def _split_nchw(tiles, n_scale, inc, step=4):
    """bp_split_scale on device tiles (n, t, t), its NHWC output rewritten NCHW."""
    lib = L.load()
    n, t, _ = tiles.shape
    wd, radii, _ = _tables(n_scale, step)
    buf, view = G.empty_nhwc(n, t, t, n_scale + inc)
    ws = int(lib.bp_split_scale_workspace(n, t, t))
    scratch = torch.empty(max(ws // 4, 1), device="cuda")
    assert lib.bp_split_scale(L.ptr(tiles), n, t, t, n_scale, inc, L.ptr(wd), radii, L.ptr(scratch), ws, C.byref(view),
                              G.stream()) == L.BP_OK
    torch.cuda.synchronize()
    return buf.permute(0, 3, 1, 2).contiguous()


@pytest.fixture(scope="module")
def gathered():
    """Per tile size: (descriptors on the device, bp_gather_tiles' output) of the shift-log dm field of 16 indices."""
    cache = {}

    def get(tile):
        if tile not in cache:
            fwd, _ = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
            ds = tile_dataset(tile, transform=T.chain_transformations([fwd, T.atleast_3d]))
            asm = DeviceTileAssembler(ds, "cuda:0")
            idx = permutation_indices(ds)
            rec = asm._descriptors("dm", idx)
            assert {1, 4} <= set(ds.sample_idx_to_tile_permutation(i)[0] for i in idx)      # a flip and a 90 degree turn
            assert any(r["rc"] != 0 for r in rec[0]) and any(r["cc"] == -1 for r in rec[0])
            desc = [torch.from_numpy(a.view(np.uint8)).cuda() for a in rec]
            out = torch.empty((len(idx), 1, tile, tile), device="cuda")
            assert L.load().bp_gather_tiles(L.ptr(desc[0]), L.ptr(desc[1]), L.ptr(desc[2]), len(idx), tile, L.ptr(out),
                                            G.stream()) == L.BP_OK
            torch.cuda.synchronize()
            cache[tile] = (desc, out, asm)
        return cache[tile]
    return get


@pytest.mark.parametrize("tile", [16, 48, 64, 80])
@pytest.mark.parametrize("n_scale,inc", [(2, 0), (2, 1), (3, 0), (3, 1)])
def test_gather_into_scales_equals_split_scale_of_the_gathered_tiles(tile, n_scale, inc, gathered):
    desc, tiles, _ = gathered(tile)
    n = tiles.shape[0]
    if tile == 16 and n_scale == 3:
        assert _tables(3)[2][2] == 24                         # r = 24 > 16: the reflection folds
    rc, got = _gather_scales(desc, None, n, tile, n_scale, inc)
    assert rc == L.BP_OK
    ref = _split_nchw(tiles[:, 0].contiguous(), n_scale, inc)
    assert got.shape == ref.shape == (n, n_scale + inc, tile, tile)
    assert torch.equal(got, ref)
    assert torch.equal(_gather_scales(desc, None, n, tile, n_scale, inc)[1], got)          # the same bits again


@pytest.mark.parametrize("tile", [16, 48])
def test_gather_into_scales_with_minima_and_single_scale(tile, gathered):
    desc, tiles, _ = gathered(tile)
    n = tiles.shape[0]
    # n_scale = 1 without minima: bp_gather_tiles' tile, once or twice
    for inc in (0, 1):
        rc, got = _gather_scales(desc, None, n, tile, 1, inc)
        assert rc == L.BP_OK and all(torch.equal(got[:, c], tiles[:, 0]) for c in range(1 + inc))
    # with minima: the single-scale form is the tile the pyramid is taken from
    mn = torch.empty(n, device="cuda")
    assert L.load().bp_tile_minima(L.ptr(desc[0]), L.ptr(desc[1]), L.ptr(desc[2]), n, tile, L.ptr(mn), G.stream()) == L.BP_OK
    rc, sub = _gather_scales(desc, mn, n, tile, 1, 0)
    assert rc == L.BP_OK and float(sub.amin()) == 0.0 and not torch.equal(sub, tiles)      # log(0 / sigma + 1) = 0
    rc, got = _gather_scales(desc, mn, n, tile, 3, 1)
    assert rc == L.BP_OK and torch.equal(got, _split_nchw(sub[:, 0].contiguous(), 3, 1))


def test_gather_into_scales_refuses_before_it_writes(gathered):
    desc, tiles, _ = gathered(16)
    n = tiles.shape[0]

    def untouched(res, code):
        rc, out = res
        return rc == code and bool(torch.isnan(out).all())
    assert untouched(_gather_scales([None, desc[1], desc[2]], None, n, 16, 3, 1), L.BP_EINVAL)
    assert untouched(_gather_scales(desc, None, n, 16, 0, 0), L.BP_EINVAL)
    assert untouched(_gather_scales(desc, None, n, 16, 3, 1, ws_bytes=4 * 3 * n * 256 - 1), L.BP_EWORKSPACE)
    assert untouched(_gather_scales(desc, None, n, 16, 17, 0, step=1), L.BP_EUNSUPPORTED)      # > 16 scales
    assert untouched(_gather_scales(desc, None, n, 16, 2, 0, step=65), L.BP_EUNSUPPORTED)      # r = 98 > 96
    assert _gather_scales(desc, None, n, 16, 2, 0, step=64)[0] == L.BP_OK                      # r = 96


# ---------------------------------------------------------------------------------------------- 3. the reference
@pytest.mark.parametrize("tag,sub", [("plain", False), ("submin", True)])
def test_assembled_batch_against_the_reference_fixture(tag, sub):
    """Per level: within 2 x the host chain's own sensitivity to one float32 rounding of the shift-log tile, plus one
    float32 ulp of the level's maximum.  The sensitivity and the worst ratio are printed."""
    gold = np.load(os.path.join(HERE, "golden", "assemble.npz"))
    tr, itr = AC.chain(T)
    ds = BAHAMASDataset(data=HC.data_dict("random"), transform=tr, inverse_transform=itr, subtract_minimum=sub,
                        **AC.DATASET)
    asm = DeviceTileAssembler(ds, "cuda:0")
    assert asm.levels == AC.LEVELS
    idx = gold[f"{tag}/idx"]
    x, y, zs = asm.get_batch([int(i) for i in idx])
    t = ds.tile_size
    assert x.shape == y.shape == (len(idx), AC.LEVELS, t, t)
    assert np.array_equal(zs.cpu().numpy().astype(np.float64), gold[f"{tag}/z"].astype(np.float32).astype(np.float64))
    split = T.create_split_scale_transform(AC.N_SCALE, AC.STEP)[0]
    worst = np.zeros((2, AC.LEVELS))                         # err / tolerance, per field and level
    sens_max = np.zeros((2, AC.LEVELS))
    for n, i in enumerate(idx):
        host = ds[int(i)][0]
        for k, dev in ((0, y), (1, x)):                      # golden order: [input, label]
            got = dev[n].cpu().numpy().astype(np.float64)
            # the float64 shift-log tile the pyramid is taken from: the reference's own where the fixture holds it
            x64 = gold[f"{tag}/full"][n, k, 0] if n < AC.N_FULL else np.asarray(host[k][0], np.float64)
            assert x64.dtype == np.float64
            # the host chain's own sensitivity to one float32 rounding of that tile
            sens = np.abs(np.asarray(split(x64.astype(np.float32), None, None, None), np.float64)
                          - split(x64, None, None, None)).max(axis=(1, 2))
            ref_pix = gold[f"{tag}/pixel"][n, k]
            level_max = np.abs(split(x64, None, None, None)).max(axis=(1, 2))
            tol = 2 * sens + np.spacing(level_max.astype(np.float32)).astype(np.float64)
            sens_max[k] = np.maximum(sens_max[k], sens)
            got_pix = np.stack([got[:, r, c] for r, c in AC.PIXELS], axis=1)
            err = np.abs(got_pix - ref_pix).max(axis=1)
            if n < AC.N_FULL:
                err = np.maximum(err, np.abs(got - gold[f"{tag}/full"][n, k]).max(axis=(1, 2)))
            err = np.maximum(err, np.abs(got.sum(axis=(1, 2)) - gold[f"{tag}/sum"][n, k]) / (t * t))
            worst[k] = np.maximum(worst[k], err / tol)
    print(tag, "host sensitivity per level, input / label:", sens_max.tolist())
    print(tag, "worst err / tolerance per level, input / label:", worst.tolist())
    assert (worst <= 1.0).all(), worst


# ---------------------------------------------------------------------------------------------- 4. a training step
def test_training_step_from_the_assembler_equals_the_step_from_host_tensors():
    """ELBO and every parameter gradient at the device / host limit of tests/test_gpu_scales_paint.py; the figures
    are printed."""
    from baryon_painter_amd.painter import CVAEPainter, _DeviceLoader
    size, n_scale, batch = 64, 2, 4
    limit = 3e-7 * R.rounding_count(n_scale)                 # tests/test_gpu_scales_paint.py: STREAM_LIMIT
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    split, unsplit = T.create_split_scale_transform(n_scale, 4, False)
    ds = BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=1,
                        n_stack=3, transform=T.chain_transformations([fwd, T.as_float32, split, T.atleast_3d]),
                        inverse_transform=T.chain_transformations([unsplit, inv, T.squeeze]),
                        n_feature_per_field=n_scale, scale_to_SLICS=True)
    arch = A.fiducial_architecture(size, n_scale=n_scale)
    torch.manual_seed(3)
    p = CVAEPainter(training_data_set=ds, test_data_set=ds, architecture=arch, compute_device="cuda:0")
    p.use_device_assembly()
    assert p.device_assembler.levels == n_scale and isinstance(p._loader(batch), _DeviceLoader)
    model = p.model
    model.train(True)
    idx = [0, 5, 13, 26]
    state = {k: v.clone() for k, v in model.state_dict().items()}
    eps = syn.synthetic_eps((1, batch, *arch["dim_z"]), seed=21)

    def step(x, y, aux):
        model.load_state_dict(state)
        model._bump_param_versions()
        model._eps_override = eps
        for q in model.parameters():
            q.grad = None
        elbo = model(x, y, aux)
        (-elbo).backward()
        return float(elbo), [q.grad.detach().cpu().numpy().astype(np.float64) for q in model.parameters()]

    x, y, z = p.device_assembler.get_batch(idx)
    assert x.shape == y.shape == (batch, n_scale, size, size) and x.is_cuda
    elbo_d, grads_d = step(x, y, z)
    samples = [ds[i] for i in idx]
    assert all(s[0][0].dtype == np.float32 for s in samples)
    hy = torch.from_numpy(np.stack([s[0][0] for s in samples])).cuda()
    hx = torch.from_numpy(np.stack([s[0][1] for s in samples])).cuda()
    hz = torch.tensor([s[2] for s in samples], dtype=torch.float32).cuda()
    elbo_h, grads_h = step(hx, hy, hz)
    model._eps_override = None
    print("ELBO device / host", elbo_d, elbo_h, "rel", abs(elbo_d - elbo_h) / abs(elbo_h), "limit", limit)
    rel = [np.abs(a - b).max() / max(np.abs(b).max(), 1e-300) for a, b in zip(grads_d, grads_h)]
    print("worst gradient err / max|grad|", max(rel), "limit", limit)
    assert np.isfinite(elbo_h) and abs(elbo_d - elbo_h) <= limit * abs(elbo_h)
    assert len(rel) > 10 and all(np.abs(g).max() > 0 for g in grads_h)
    assert max(rel) <= limit, (max(rel), limit)


def test_train_runs_on_the_assembled_multi_scale_batches():
    """``train()`` itself, eager and with ``graph_step``, fed by ``use_device_assembly()``."""
    from baryon_painter_amd.painter import CVAEPainter
    size, n_scale = 64, 2
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    split, unsplit = T.create_split_scale_transform(n_scale, 4, False)
    ds = BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=1,
                        n_stack=3, transform=T.chain_transformations([fwd, T.as_float32, split, T.atleast_3d]),
                        inverse_transform=T.chain_transformations([unsplit, inv, T.squeeze]),
                        n_feature_per_field=n_scale, scale_to_SLICS=True, subtract_minimum=True)
    torch.manual_seed(5)
    p = CVAEPainter(training_data_set=ds, test_data_set=ds, architecture=A.fiducial_architecture(size, n_scale=n_scale),
                    compute_device="cuda:0")
    p.use_device_assembly()
    for graph_step in (False, True):
        ts, vs = p.train(n_epoch=1, n_pepoch=1, learning_rate=1e-3, batch_size=4, pepoch_size=12, validation_pepochs=[],
                         validation_loss_frequency=10 ** 9, statistics_report_frequency=0, verbose=False,
                         graph_step=graph_step)
        elbo = np.asarray(ts.loss_terms["ELBO"]["all"])
        assert len(elbo) >= 3 and np.isfinite(elbo).all()


# ---------------------------------------------------------------------------------------------- 5. unchanged
def test_single_scale_batch_is_the_direct_gather(gathered):
    desc, tiles, asm = gathered(16)
    ds = asm.ds
    idx = permutation_indices(ds)
    assert asm.scales is None and asm.levels == 1 and asm.k_values == {"dm": 4.0, "pressure": 4.0}
    x, y, z = asm.get_batch(idx)
    assert torch.equal(y, tiles) and x.shape == y.shape
    explicit = DeviceTileAssembler(ds, "cuda:0", k_values=HC.K_VALUES)       # the form from before chains were read
    xe, ye, ze = explicit.get_batch(idx)
    assert torch.equal(x, xe) and torch.equal(y, ye) and torch.equal(z, ze)
    lib = L.load()
    rec = [torch.from_numpy(a.view(np.uint8)).cuda() for a in asm._descriptors("pressure", idx)]
    out = torch.empty_like(x)
    assert lib.bp_gather_tiles(L.ptr(rec[0]), L.ptr(rec[1]), L.ptr(rec[2]), len(idx), 16, L.ptr(out), G.stream()) == L.BP_OK
    torch.cuda.synchronize()
    assert torch.equal(x, out)
    # the new entry point's single-scale form stores the same bits
    rc, same = _gather_scales(rec, None, len(idx), 16, 1, 0)
    assert rc == L.BP_OK and torch.equal(same, out)
