"""Round-3 parity cases (fixtures: tests/golden/model_r3.npz, made from the imported reference by
tests/golden/make_goldens_r3.py):

  * WELL-CONDITIONED gradients: the fiducial net with every ReLU softened to LeakyReLU(0.9) (same layers, kernels
    and wiring; a tenth of the activation kink).  The reference's own fp32 gradients of these cases lie within
    1e-6..5e-5 of the float64 truth (the ReLU net: 1e-3..1e-2), so every HIP gradient is held to 2e-4 of its scale:
    a percent-level error in any kernel of the backward chain cannot hide.
  * the backward chain layer by layer on that softened network (every convolution's d(loss)/d(raw) against the
    float64 evaluation of the same graph, next to what stock fp32 torch achieves).
  * the training script's two-head network at its real geometry (512^2), fp32 and bf16.
  * fid128_n16: sixteen tiles, the standard noise-floor criterion.
"""
import os

import numpy as np
import pytest
import torch

from baryon_painter_amd.models import arch as A
from baryon_painter_amd.utils import synthetic as syn
from golden_util import check, crop_rel_l2, distance, summary_distance

import gpu_util as G
from plan_units import conv_units as _conv_units

pytestmark = pytest.mark.gpu
SLOPE = 0.9


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_r3.npz"))


def _model(arch, soft=False, dtype="f32"):
    from baryon_painter_amd.models.cvae import CVAE
    m = CVAE(arch, "cuda:0", dtype=dtype)
    P = syn.fill_params({k: tuple(p.shape) for k, p in m.named_parameters()}, 7)
    if soft:
        P = syn.soften_params(P, SLOPE)
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(torch.from_numpy(P[k]))
    return m, P


def _floor(tag, k, gold):
    """max(reference executions' distance from the float64 truth, conditioning draws) -- as tests/test_gpu_model.py."""
    errs = [summary_distance(f"{tag}/grad/{k}", f"{tag}/grad64/{k}", gold)]
    names = str(gold[f"{tag}/grad_variant_params"]).split(",")
    errs += list(gold[f"{tag}/grad_variant_dist"][:, names.index(k)])
    names = str(gold[f"{tag}/grad_cond_params"]).split(",")
    errs += list(gold[f"{tag}/grad_cond_dist"][:, names.index(k)])
    return float(max(errs))


def _step(m, arch, n, size):
    x, y, aux = syn.synthetic_batch(n, size, size, seed=1234)
    m._eps_override = syn.synthetic_eps((1, n, *arch["dim_z"]), seed=99)
    m.train(True)
    elbo = m(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
    (-elbo).backward()
    torch.cuda.synchronize()
    return x, y, aux


@pytest.mark.parametrize("tag,size,n", [("soft128_n4", 128, 4), ("soft512_n2", 512, 2)])
def test_well_conditioned_gradients_match_reference(tag, size, n, gold):
    """Every parameter gradient within 2e-4 of its scale of the float64 truth (10x tighter than the 2e-3 floor of
    the ReLU cases); forward quantities at the usual fp32 tolerances against the REFERENCE's run."""
    fid = A.fiducial_architecture(512)
    arch = syn.softened_architecture(fid if size == 512 else syn.scaled_architecture(fid, size), SLOPE)
    m, P = _model(arch, soft=True)
    assert ",".join(m.state_dict().keys()) == str(gold[f"{tag}/state_keys"])
    x, y, aux = _step(m, arch, n, size)
    check(f"{tag}/stats", np.array(m.get_stats()), gold, 2e-5)
    check(f"{tag}/x_mu", m.x_mu.cpu().numpy(), gold, 1e-4)
    check(f"{tag}/z_mu", m.z_mu.cpu().numpy(), gold, 1e-4)
    check(f"{tag}/z_log_var", m.z_log_var.cpu().numpy(), gold, 1e-4)
    if f"{tag}/x_mu/crop_tl" in gold:
        assert crop_rel_l2(f"{tag}/x_mu", m.x_mu.cpu().numpy(), gold) <= 1e-4
    rows = []
    for k, p in m.named_parameters():
        ours = distance(f"{tag}/grad64/{k}", p.grad.cpu().numpy(), gold)
        rows.append((ours / max(4 * _floor(tag, k, gold), 2e-4), ours, _floor(tag, k, gold), k))
    rows.sort(reverse=True)
    print("worst gradients (distance from float64 truth / limit, distance, fp32 noise floor):", rows[:6])
    assert rows[0][0] < 1.0, rows[:6]
    # no tensor anywhere near the percent level; nine in ten within 2e-4 (the rest are zero-true-gradient biases in
    # front of a batch-norm and the one-channel latent path, whose floors the fixtures hold)
    assert max(r[1] for r in rows) < 3e-3 and np.mean([r[1] < 2e-4 for r in rows]) >= 0.9, rows[:10]
    for k, b in m.named_buffers():
        check(f"{tag}/buf/{k}", b.cpu().numpy(), gold, 2e-5)
    m.train(False)
    zfix = syn.synthetic_eps((n, *arch["dim_z"]), seed=101)
    s = m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux), z=zfix)
    check(f"{tag}/sample_P_eval_zfix", s.cpu().numpy(), gold, 1e-4)


def test_sixteen_tile_case_matches_reference(gold):
    tag, size, n = "fid128_n16", 128, 16
    arch = A.fiducial_architecture(size)
    m, P = _model(arch)
    _step(m, arch, n, size)
    check(f"{tag}/stats", np.array(m.get_stats()), gold, 2e-5)
    check(f"{tag}/x_mu", m.x_mu.cpu().numpy(), gold, 1e-4)
    rows = []
    for k, p in m.named_parameters():
        ours = distance(f"{tag}/grad64/{k}", p.grad.cpu().numpy(), gold)
        rows.append((ours / max(4 * _floor(tag, k, gold), 2e-3), ours, k))
    rows.sort(reverse=True)
    assert rows[0][0] < 1.0, rows[:6]
    for k, b in m.named_buffers():
        check(f"{tag}/buf/{k}", b.cpu().numpy(), gold, 2e-5)


# ---------------------------------------------------------------------------------------------- two heads at 512^2
@pytest.mark.parametrize("tag,alpha", [("twohead512_n2", 0.3), ("twohead512_n2_a1", 1.0)])
def test_training_script_network_at_512(tag, alpha, gold):
    """The two-head net scripts/CVAE_single_scale.py builds (p_var_out, free-variance likelihood, alpha blend;
    /root/reference/baryon_painter/models/cvae.py:33-41,115-118,135-144) at its real geometry."""
    arch = A.fiducial_architecture(512, predict_var=True)
    m, P = _model(arch)
    assert ",".join(m.state_dict().keys()) == str(gold[f"{tag}/state_keys"])
    assert ",".join(m.get_stats_labels()) == str(gold[f"{tag}/stats_labels"])
    m.alpha_var = alpha
    x, y, aux = _step(m, arch, 2, 512)
    check(f"{tag}/stats", np.array(m.get_stats()), gold, 2e-5)
    assert crop_rel_l2(f"{tag}/x_mu", m.x_mu.cpu().numpy(), gold) <= 1e-4
    check(f"{tag}/z_mu", m.z_mu.cpu().numpy(), gold, 1e-4)
    # gradients: float64 truth in the fixture; noise floor = the reference's own distance from it, and never below
    # 5e-3 (two-tile ReLU case without stored execution variants: see fid512_n2 for those)
    rows = []
    for k, p in m.named_parameters():
        ref = summary_distance(f"{tag}/grad/{k}", f"{tag}/grad64/{k}", gold)
        ours = distance(f"{tag}/grad64/{k}", p.grad.cpu().numpy(), gold)
        rows.append((ours / max(4 * ref, 5e-3), ours, ref, k))
    rows.sort(reverse=True)
    assert rows[0][0] < 1.0, rows[:6]
    for k, b in m.named_buffers():
        check(f"{tag}/buf/{k}", b.cpu().numpy(), gold, 2e-5)
    m.train(False)
    zfix = syn.synthetic_eps((2, *arch["dim_z"]), seed=101)
    mu, var = m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux), z=zfix, return_var=True)
    assert crop_rel_l2(f"{tag}/sample_P_eval_zfix", mu.cpu().numpy(), gold) <= 1e-4
    check(f"{tag}/sample_P_eval_var", var.cpu().numpy(), gold, 1e-4)


def test_training_script_network_at_512_bf16(gold):
    """The same in throughput mode (bf16 trunk): stated bf16 tolerances against the reference's fp32 run."""
    tag = "twohead512_n2"
    arch = A.fiducial_architecture(512, predict_var=True)
    m, P = _model(arch, dtype="bf16")
    m.alpha_var = 0.3
    x, y, aux = _step(m, arch, 2, 512)
    got = np.array(m.get_stats())
    ref = gold[f"{tag}/stats/full"].astype(np.float64)
    assert np.abs(got - ref).max() <= 1e-3 * np.abs(ref).max(), (got, ref)
    assert crop_rel_l2(f"{tag}/x_mu", m.x_mu.cpu().numpy(), gold) <= 1e-2
    flat, flat_ref = [], []
    for k, p in m.named_parameters():
        g = p.grad.cpu().numpy().reshape(-1).astype(np.float64)
        assert np.isfinite(g).all(), k
        if f"{tag}/grad/{k}/full" in gold:            # the small tensors are stored whole
            flat.append(g)
            flat_ref.append(gold[f"{tag}/grad/{k}/full"].astype(np.float64).reshape(-1))
    a, b = np.concatenate(flat), np.concatenate(flat_ref)
    cos = float(a @ b / np.sqrt((a @ a) * (b @ b)))
    assert cos >= 0.99, cos
    m.train(False)
    zfix = syn.synthetic_eps((2, *arch["dim_z"]), seed=101)
    mu, var = m.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux), z=zfix, return_var=True)
    assert crop_rel_l2(f"{tag}/sample_P_eval_zfix", mu.cpu().numpy(), gold) <= 1e-2


# ---------------------------------------------------------------------------------------------- the chain, layer by layer
@pytest.mark.parametrize("size,n", [(128, 2), (512, 2)])
def test_backward_chain_layer_by_layer(size, n):
    """tools/chain_bisect.py as a test, on the WELL-CONDITIONED (softened) network: every convolution's raw output and
    d(loss)/d(raw) of the HIP path against the float64 evaluation of the same graph (stock torch.nn.functional on the
    CPU, oracle/torch_ref.py), next to the distance of the fp32 evaluation of that graph on the CPU -- what the
    reference computes.  On the ReLU network this comparison is dominated by mask flips that are individual to each
    fp32 execution (measured here at 128^2: stock torch 4e-6 from the truth in an execution without a flip, the HIP path
    5e-3 with one -- a ratio of 500 that says nothing about any kernel); with the kinks softened tenfold every layer
    of both executions lies within 1e-6..1e-4 of the truth, and a kernel that deviates at the percent level stands
    out by two orders of magnitude.  Limit per layer: max(4 x stock fp32, 3e-4) relative L2 for d_raw, 2e-6 for raw."""
    from oracle.torch_ref import TorchRefCVAE
    fid = A.fiducial_architecture(512)
    arch = syn.softened_architecture(fid if size == 512 else syn.scaled_architecture(fid, size), SLOPE)
    m, P = _model(arch, soft=True)
    x, y, aux = syn.synthetic_batch(n, size, size, seed=1234)
    eps = syn.synthetic_eps((1, n, *arch["dim_z"]), seed=99)
    m._eps_override = eps
    elbo = m(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
    (-elbo).backward()
    torch.cuda.synchronize()
    taps = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        tap = {}
        r = TorchRefCVAE(arch, P, dtype=dt, tap=tap)
        (-r.forward(x, y, aux, eps)).backward()
        taps[name] = tap

    def rel(a, b):
        a, b = a.double(), b.double()
        return float((a - b).norm() / b.norm().clamp_min(1e-300))

    rows = []
    for u in _conv_units(m._last):
        t64, t32 = taps["f64"][u.name + "."], taps["f32"][u.name + "."]
        s = u.out
        raw = s.buf[..., s.coff:s.coff + s.c].permute(0, 3, 1, 2).float().cpu()
        assert rel(raw, t64.detach()) <= max(2e-6, 3 * rel(t32.detach(), t64.detach())), u.name
        if t64.grad is None:
            continue
        g = s.grad_buf[..., s.coff:s.coff + s.c].permute(0, 3, 1, 2).float().cpu()
        ours, stock = rel(g, t64.grad), rel(t32.grad, t64.grad)
        rows.append((ours / max(4 * stock, 3e-4), ours, stock, u.name))
    rows.sort(reverse=True)
    print("d_raw: (distance / limit, ours, stock fp32 torch) worst first:")
    for r in rows:
        print("  %.3f  %.2e  %.2e  %s" % r)
    assert len(rows) >= 30
    assert rows[0][0] <= 1.0, rows[:5]


TWIN_SEEDS = (1234, 1235, 1236, 1237)


@pytest.mark.parametrize("size,n", [(128, 4), (512, 2)])
def test_bf16_gradients_per_tensor_and_chain_against_rounding_twin(size, n):
    """Throughput mode (CVAE(dtype="bf16"), BASELINE.json configs[3]) held PER TENSOR, on the well-conditioned softened
    network: every parameter gradient, and every convolution's raw output and d(loss)/d(raw), against the float64
    evaluation of the graph (oracle/torch_ref.py, pinned to the reference's fixtures).

    What a correct bf16 execution's distance from that truth should be depends on the tensor: bf16 rounds every trunk
    activation and gradient to 8 bits, and how much of that noise survives in a gradient is the tensor's conditioning
    (the 1-channel latent up-sampler's batch-norm parameters are 1000 : 1 cancelling sums: their bf16 gradients are
    30 % - 100 % noise in any execution; a 128-channel trunk weight sits at 1e-2).  So the yardstick is measured, per
    tensor, in the test: the ROUNDING TWIN -- the same float64 graph with a bf16 round-trip wherever the HIP path
    stores or stages bf16 (TorchRefCVAE(bf16=True)): same noise, same places, no kernels.  Measured on MI355X the two
    agree to a few percent layer by layer (d_raw 2.72e-2 vs 2.63e-2, ...), median ratio over the parameters 1.0.
    Criterion, over four batches (a tensor's distance is ONE draw of its noise; for the one- and two-element batch-norm
    tensors of the latent path the ratio of two single draws is heavy-tailed, the ratio of two four-draw RMS values is not):
        rms distance(HIP, truth) <= max(m x rms distance(twin, truth), 5e-3),   m = 2 (>= 64 elements) or 4 (tiny tensors)
    and for the chain tensors of the first batch  distance(HIP) <= max(3 x distance(twin), 2e-3).  The twin must BE a
    noise model of this path: the median ratio over all tensors within [1/2, 2].  (measured: HIP / twin <= 1.16 on every tensor.)  A kernel that is 3 % off in one trunk
    tensor (twin distance 1e-2) fails; the whole-vector cosine this replaces could not see it.
    The step is /root/reference/baryon_painter/painter.py:224-228."""
    from oracle.torch_ref import TorchRefCVAE
    fid = A.fiducial_architecture(512)
    arch = syn.softened_architecture(fid if size == 512 else syn.scaled_architecture(fid, size), SLOPE)
    m, P = _model(arch, soft=True, dtype="bf16")
    m.train(True)

    def rel(a, b):
        a, b = a.double(), b.double()
        return float((a - b).norm() / b.norm().clamp_min(1e-300))

    d_hip = {k: [] for k, _ in m.named_parameters()}
    d_twin = {k: [] for k in d_hip}
    for it, seed in enumerate(TWIN_SEEDS):
        x, y, aux = syn.synthetic_batch(n, size, size, seed=seed)
        eps = syn.synthetic_eps((1, n, *arch["dim_z"]), seed=seed + 99)
        for p_ in m.parameters():
            p_.grad = None
        m._eps_override = eps
        elbo = m(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
        (-elbo).backward()
        torch.cuda.synchronize()
        runs = {}
        for name, twin in (("truth", False), ("twin", True)):
            tap = {}
            r = TorchRefCVAE(arch, P, dtype=torch.float64, tap=tap, bf16=twin)
            (-r.forward(x, y, aux, eps)).backward()
            runs[name] = (r, tap)
        e64 = float(runs["truth"][0].ELBO.detach())
        assert abs(float(elbo) - e64) <= 2e-3 * abs(e64)
        for k, p_ in m.named_parameters():
            g = p_.grad.detach().cpu()
            assert torch.isfinite(g).all(), k
            t, w = runs["truth"][0].P[k].grad, runs["twin"][0].P[k].grad
            d_hip[k].append(rel(g, t))
            d_twin[k].append(rel(w, t))
        if it:
            continue
        # ---- the chain, layer by layer (first batch)
        crow, nb16 = [], 0
        for u in _conv_units(m._last):
            t64, tw = runs["truth"][1][u.name + "."], runs["twin"][1][u.name + "."]
            s = u.out
            nb16 += s.buf.dtype == torch.bfloat16
            raw = s.buf[..., s.coff:s.coff + s.c].permute(0, 3, 1, 2).float().cpu()
            r_hip, r_twin = rel(raw, t64.detach()), rel(tw.detach(), t64.detach())
            assert r_hip <= max(3 * r_twin, 2e-5), (u.name, r_hip, r_twin)
            if t64.grad is None:
                continue
            g = s.grad_buf[..., s.coff:s.coff + s.c].permute(0, 3, 1, 2).float().cpu()
            g_hip, g_twin = rel(g, t64.grad), rel(tw.grad, t64.grad)
            crow.append((g_hip / max(3 * g_twin, 2e-3), g_hip, g_twin, r_hip, r_twin, u.name))
        crow.sort(reverse=True)
        print("bf16 chain: d_raw distance / limit, HIP, twin | raw HIP, twin")
        for r_ in crow:
            print("  %.3f  %.2e  %.2e | %.2e  %.2e  %s" % r_)
        assert nb16 >= 15, "the trunk's slots should be bf16"
        assert len(crow) >= 30 and crow[0][0] <= 1.0, crow[:5]

    # ---- parameter gradients: rms over the batches
    numel = {k: p_.numel() for k, p_ in m.named_parameters()}
    rows = []
    for k in d_hip:
        h, t = float(np.sqrt(np.mean(np.square(d_hip[k])))), float(np.sqrt(np.mean(np.square(d_twin[k]))))
        mult = 2.0 if numel[k] >= 64 else 4.0
        rows.append((h / max(mult * t, 5e-3), h, t, numel[k], k))
    rows.sort(reverse=True)
    print("bf16 parameter gradients: rms distance from float64 / limit, HIP, twin, elements (worst first)")
    for r_ in rows[:14]:
        print("  %.3f  %.2e  %.2e  %7d  %s" % r_)
    ratios = [r_[1] / r_[2] for r_ in rows if r_[2] > 1e-4]
    print("  median HIP / twin %.2f over %d tensors; median HIP distance %.2e" % (np.median(ratios), len(ratios), np.median([r_[1] for r_ in rows])))
    assert rows[0][0] <= 1.0, rows[:6]
    assert 0.5 <= np.median(ratios) <= 2, np.median(ratios)
