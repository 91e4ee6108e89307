"""GPU: one CGAN training iteration under ``train_dtype="bf16"`` against the float64 restatement.

Truth: ``oracle.cgan_torch.TorchCGAN(dtype=torch.float64)``.  Yardstick: its rounding twin, tests/cgan_bf16_train_ref.py
-- the same float64 iteration with a tensor rounded to bf16 wherever the training plan stores or stages bf16.  Criterion
(the project's bf16 criterion, tests/test_gpu_parity_r3.py and the floor of tests/test_gpu_cgan_bf16_paint.py), per
parameter tensor of both networks, the distance measured as tests/test_gpu_cgan.py measures it (largest difference over
the larger of the tensor's scale and 1e-4 of its network's):

    distance(HIP, truth) <= max(4 x distance(twin, truth), 5e-3)
    |loss - truth| <= max(2 x |twin - truth|, 5e-3 max(1, |truth|))          for each of the three losses

Cases: tile 64 / two blocks / batch 4 (trunk 16 wide: the tiled weight gradient), tile 256 / one block / batch 2 (trunk 64
wide: the output-stationary kernel), tile 512 / one block / batch 2 (trunk 128 wide: column strips in all three passes).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from baryon_painter_amd import _lib as L
from baryon_painter_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu

CASES = [(64, 2, 4, "bf16_tiled"), (256, 1, 2, "ws_bf16"), (512, 1, 2, "ws_bf16")]


def _batch(size, n):
    x, y, z = syn.synthetic_batch(n, size, size, seed=5)
    return np.tanh(3 * x - 0.5).astype(np.float32), y, z             # real field in the tanh domain


def _model(size, n_res, seed=0, **kw):
    from baryon_painter_amd.models.cgan import CGAN
    torch.manual_seed(seed)
    m = CGAN(tile_size=size, device="cuda:0", n_res=n_res, **kw)
    m.train(True)
    return m


def _step(m, batch):
    x, y, z = batch
    opt_g = torch.optim.Adam(m.g_parameters(), lr=5e-5, betas=(0.5, 0.999))
    opt_d = torch.optim.Adam(m.d_parameters(), lr=5e-5, betas=(0.5, 0.999))
    cap = {}
    losses = m.train_step(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(z), opt_g, opt_d, capture=cap)
    torch.cuda.synchronize()
    return {k: float(v) for k, v in losses.items()}, cap


def _flat(cap):
    return {net + "." + k: v for net in ("d", "g") for k, v in cap[net].items()}


@pytest.mark.parametrize("size,n_res,n,family", CASES, ids=["tile%d" % c[0] for c in CASES])
def test_bf16_iteration_against_the_rounding_twin(size, n_res, n, family):
    from baryon_painter_amd.models.graph import CastUnit
    from cgan_bf16_train_ref import TwinCGAN
    from oracle.cgan_torch import TorchCGAN
    m = _model(size, n_res, train_dtype="bf16")
    state = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    batch = _batch(size, n)
    losses, cap = _step(m, batch)

    # ---- the plan: exactly the residual convolutions in bf16, a cast at either end, the weight gradient's family
    plan = m._plan(n)
    units = plan.flat_units(plan.g_units)
    convs = [u for u in units if not isinstance(u, CastUnit)]
    casts = [u for u in units if isinstance(u, CastUnit)]
    assert [u.name for u in convs if u.bf16] == [u.name for u in convs if ".res_block." in u.name] and \
        sum(u.bf16 for u in convs) == 2 * n_res
    assert all(u.inp.dt == L.BF16 and u.out.dt == L.BF16 and u.out.w == size // 4 for u in convs if u.bf16)
    assert all(u.inp.dt == L.F32 and u.out.dt == L.F32 for u in convs if not u.bf16)
    assert [(u.inp.dt, u.out.dt) for u in casts] == [(L.F32, L.BF16), (L.BF16, L.F32)]
    assert not any(u.bf16 for u in plan.flat_units(plan.d_units) + plan.flat_units(plan.d_units_fake))
    for u in convs:
        if u.bf16:
            out = (C.c_int32 * 4)()
            assert m._lib.bp_conv_backward_weight_plan(C.byref(u.cv), C.byref(u.inp.view), C.byref(u.out.grad), L.IMPL_BF16,
                                                       out) == L.BP_OK
            assert L.WGRAD_FAMILIES[out[0]] == family, u.name
            if size == 512:
                for d, (a, b) in ((L.PACK_FWD, (u.inp.view, u.out.view)), (L.PACK_BWD, (u.out.grad, u.dx))):
                    assert m._lib.bp_conv_ws_kind(C.byref(u.cv), d, C.byref(a), C.byref(b)) == 3, (u.name, d)

    # ---- truth and twin
    runs = {}
    for name, cls in (("truth", TorchCGAN), ("twin", TwinCGAN)):
        r = cls(m.g_arch, m.d_arch, state, m.lambda_perceptual, dtype=torch.float64)
        rl, gd, gg, _ = r.iteration(*batch)
        runs[name] = (rl, {**{"d." + k[len("discriminator."):]: v for k, v in gd.items()},
                           **{"g." + k[len("generator."):]: v for k, v in gg.items()}}, r.P)
    t_loss, t_grad, t_state = runs["truth"]
    w_loss, w_grad, w_state = runs["twin"]
    for k in ("D", "G_adv", "G_perceptual"):
        print("loss %-12s HIP %.9f  twin %.9f  truth %.9f" % (k, losses[k], w_loss[k], t_loss[k]))
        assert abs(losses[k] - t_loss[k]) <= max(2 * abs(w_loss[k] - t_loss[k]), 5e-3 * max(1.0, abs(t_loss[k]))), k

    scale0 = {net: 1e-4 * max(float(v.abs().max()) for k, v in t_grad.items() if k[0] == net and v.numel() > 1)
              for net in "dg"}

    def dist(a, w, s0=0.0):
        return float((a.detach().cpu().double() - w).abs().max() / max(float(w.abs().max()), s0, 1e-300))

    rows = []
    got = _flat(cap)
    assert set(got) == set(t_grad)
    for k, g in got.items():
        assert torch.isfinite(g).all(), k
        w = t_grad[k].double()
        d_hip, d_twin = dist(g, w, scale0[k[0]]), dist(w_grad[k], w, scale0[k[0]])
        rows.append((d_hip / max(4 * d_twin, 5e-3), d_hip, d_twin, k))
    rows.sort(reverse=True)
    print("tile %d: parameter gradients, distance from float64 / limit, HIP, twin (worst first)" % size)
    for r in rows[:8]:
        print("  %.3f  %.2e  %.2e  %s" % r)
    print("  worst HIP / twin %.2f" % max((r[1] / r[2] for r in rows if r[2] > 1e-4), default=0.0))
    assert rows[0][0] <= 1.0, rows[:6]

    # ---- batch-norm running statistics and the power iteration's u, v after the iteration: the same criterion
    after = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    for k, v in after.items():
        if k.endswith(("running_mean", "running_var", "weight_u", "weight_v")):
            d_hip, d_twin = dist(v, t_state[k].double()), dist(w_state[k], t_state[k].double())
            assert d_hip <= max(4 * d_twin, 5e-3), (k, d_hip, d_twin)


def test_fp32_keyword_is_the_training_of_before_and_bf16_repeats_its_bits():
    batch = _batch(64, 4)
    a = _step(_model(64, 2), batch)
    b = _step(_model(64, 2, train_dtype="fp32"), batch)
    assert a[0] == b[0]
    fa, fb = _flat(a[1]), _flat(b[1])
    assert all(torch.equal(fa[k], fb[k]) for k in fa), "train_dtype='fp32' changed a gradient"
    # two bf16 iterations from one seed: the same bits -- through the strip kernels too
    for size, n_res, n in ((64, 2, 4), (512, 1, 2)):
        batch = _batch(size, n)
        c = _step(_model(size, n_res, train_dtype="bf16"), batch)
        d = _step(_model(size, n_res, train_dtype="bf16"), batch)
        assert c[0] == d[0]
        fc, fd = _flat(c[1]), _flat(d[1])
        assert all(torch.equal(fc[k], fd[k]) for k in fc), "two bf16 iterations differ"
        if size == 64:
            assert c[0] != a[0] and any(not torch.equal(fa[k], fc[k]) for k in fa), "bf16 never ran"


def test_painter_trains_in_bf16_and_its_checkpoint_paints(tmp_path):
    from baryon_painter_amd.painter import CGANPainter
    from baryon_painter_amd.utils import datasets as D
    tile = 64
    ds = D.SyntheticTileDataset(n_sample=16, tile_size=tile, seed=3)
    torch.manual_seed(4)
    p = CGANPainter(training_data_set=ds, tile_size=tile, compute_device="cuda:0", n_res=2, train_dtype="bf16")
    assert p.model.train_dtype == "bf16" and p.model.paint_dtype == "fp32"
    log = p.train(n_iter=2, batch_size=2)
    assert len(log) == 2 and all(np.isfinite(v) for row in log for v in row.values())
    assert any(u.bf16 for u in p.model._plan(2).flat_units(p.model._plan(2).g_units))
    files = (str(tmp_path / "state"), str(tmp_path / "meta"))
    p.save_state_to_file(files)
    dm, _, z = ds.raw_fields(1)
    want = p.paint(dm, z=z)
    q = CGANPainter(filename=files, compute_device="cuda:0")
    assert q.train_dtype == "bf16" and q.model.train_dtype == "bf16" and q.paint_dtype == "fp32"
    out32 = q.paint(dm, z=z)
    assert out32.shape == (tile, tile) and np.array_equal(out32, want)
    q.paint_dtype = q.model.paint_dtype = "bf16"
    out16 = q.paint(dm, z=z)
    assert out16.shape == (tile, tile) and np.isfinite(out16).all() and not np.array_equal(out16, out32)
