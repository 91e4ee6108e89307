"""GPU: ``CVAE.score`` and ``CVAE.reconstruct`` on 64^2 tiles against ``oracle.torch_ref.TorchRefCVAE`` in float64, in
eval mode, for the two-head painter of tests/test_gpu_pixel_noise_paint.py (its running statistics settled by thirty
training-mode forwards, as tests/test_gpu_ensemble_paint.py does) and two more painters restored from (state, meta)
files: one without a variance head, one without a prior network.

The yardstick of a log-weight is the deviation of the float32 CPU twin (the same oracle in float32, same inputs) from
float64; the device may deviate four times as much -- the margin the project's parity tests give the HIP path over oneDNN
for its different summation order -- with a floor of 2e-5 of the sum of the magnitudes of the entry's terms, the
project's operator tolerance.  bound, elbo, log_likelihood and kl inherit the largest limit of their tile (logsumexp and
the mean are 1-Lipschitz in the sup norm); the effective sample size is checked against the device's own log-weights."""
import math

import numpy as np
import pytest
import torch

import score_ref as S
import test_gpu_pixel_noise_paint as PN
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu
SIZE = PN.SIZE
N, K = 3, 4


def settle(q):
    """Thirty training-mode forwards without gradients: the running statistics move away from their initial values, so
    that in eval mode the latent matters (tests/test_gpu_ensemble_paint.py)."""
    cx, cy = q.model.dim_x[0], q.model.dim_y[0]
    x, y, aux = syn.synthetic_batch(4, SIZE, SIZE, seed=77)
    q.model.train(True)
    with torch.no_grad():
        for _ in range(30):
            q.model(torch.from_numpy(np.repeat(x, cx, axis=1)), torch.from_numpy(np.repeat(y, cy, axis=1)),
                    torch.from_numpy(aux))
    q.model.train(False)
    return q


def build_plain(tmp, arch, ds):
    """``PN.build`` for a painter without a variance head: one training-mode forward, saved and reloaded."""
    from baryon_painter_amd.painter import CVAEPainter
    torch.manual_seed(3)
    p = CVAEPainter(training_data_set=ds, test_data_set=ds, architecture=arch, compute_device="cuda:0")
    x, y, aux = syn.synthetic_batch(4, SIZE, SIZE, seed=77)
    with torch.no_grad():
        p.model(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
    files = (str(tmp / "state"), str(tmp / "meta"))
    p.save_state_to_file(files)
    q = CVAEPainter(filename=files, compute_device="cuda:0")
    q.checkpoint_files = files
    return q


def make_painter(kind, tmp):
    ds = PN.single_field_dataset()
    if kind == "two heads":
        return settle(PN.build(tmp, PN.two_head_architecture(), ds))
    if kind == "no variance head":
        return settle(build_plain(tmp, A.fiducial_architecture(SIZE), ds))
    assert kind == "no prior network"
    return settle(PN.build(tmp, PN.two_head_architecture(prior=False), ds))


KINDS = ["two heads", "no variance head", "no prior network"]


@pytest.fixture(scope="module", params=KINDS)
def painter(request, tmp_path_factory):
    q = make_painter(request.param, tmp_path_factory.mktemp("ckpt"))
    assert q.model.predict_var == (request.param != "no variance head")
    assert (q.model.prior_network is None) == (request.param == "no prior network")
    return q


def inputs(model, n=N, k=K):
    x, y, aux = syn.synthetic_batch(n, SIZE, SIZE, seed=5)
    return x, y, aux, syn.synthetic_eps((k, n, *model.dim_z), seed=11)


def state_of(model):
    return {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


def log_weight_limits(model, x, y, aux, eps):
    """(float64 log w, ll_sum, r, per-entry limit, the oracle's samples) -- the yardstick of the module docstring."""
    arch, state = model.architecture, state_of(model)
    lw64, ll64, r64, mag, s64 = S.oracle_log_weights(arch, state, x, y, aux, eps, torch.float64)
    lw32 = S.oracle_log_weights(arch, state, x, y, aux, eps, torch.float32)[0]
    yard = np.abs(lw32 - lw64)
    return lw64, ll64, r64, np.maximum(4.0 * yard, 2e-5 * mag), yard, mag, s64


def test_score_equals_the_float64_oracle_under_the_same_normals(painter):
    m = painter.model
    x, y, aux, eps = inputs(m)
    out, lw = m.score(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux), draws=K, eps=eps,
                      return_log_w=True)
    assert out.dtype == lw.dtype == torch.float64 and tuple(out.shape) == (N, 5) and tuple(lw.shape) == (K, N)
    out, lw = out.cpu().numpy(), lw.cpu().numpy()
    lw64, ll64, r64, limit, yard, mag, _ = log_weight_limits(m, x, y, aux, eps)
    err = np.abs(lw - lw64)
    print("log w: |dev - f64| / |f32 twin - f64| per entry\n", err / np.maximum(yard, 1e-300))
    print("log w: |dev - f64| / sum|term|\n", err / mag, "\n|f32 twin - f64| / sum|term|\n", yard / mag)
    print("log w: |dev - f64| / limit, largest:", (err / limit).max())
    assert (err <= limit).all(), (err / limit).max()
    ref = S.score(lw64, ll64, r64)
    tile = limit.max(axis=0)
    print("columns 0-3: |dev - f64| / limit of the tile\n", np.abs(out[:, :4] - ref[:, :4]) / tile[:, None])
    assert (np.abs(out[:, :4] - ref[:, :4]) <= tile[:, None]).all()
    ess = S.ess_of(lw)
    assert (np.abs(out[:, 4] - ess) <= 1e-9 * ess).all() and (out[:, 4] >= 1 - 1e-9).all() and (out[:, 4] <= K).all()
    assert (out[:, 0] >= out[:, 1] - tile).all()
    # without the log-weights: the same bits; the same call twice too
    again = m.score(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux), draws=K, eps=eps).cpu().numpy()
    assert np.array_equal(again, out)
    # one draw: bound == elbo, ess == 1
    one = m.score(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux), draws=1, eps=eps[:1]).cpu().numpy()
    assert np.array_equal(one[:, 0], one[:, 1]) and (one[:, 4] == 1.0).all()
    assert (np.abs(one[:, 1] - lw64[0]) <= limit[0]).all()             # draw 0 of the four, from a plan of its own


def test_log_likelihood_is_the_pinned_loss_with_log_2pi_per_pixel(painter):
    """Eval mode, K = L = 1, the same normals: mean_m ll[m] = (log_likelihood_free_var - c0) + H W c0 with
    c0 = -log(2 pi)/2 (``log_likelihood_fixed_var`` for the painter without a variance head), the statistics of
    ``model(x, y, aux)``, within 2e-5 of the sum of the magnitudes of the terms."""
    m = painter.model
    assert m.L == 1 and m.dim_x[0] == 1 and not m.training
    x, y, aux, eps = inputs(m, k=1)
    m._eps_override = eps
    try:
        with torch.no_grad():
            m(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
        stat = float((m.log_likelihood_free_var if m.predict_var else m.log_likelihood)[0])
        out = m.score(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux), draws=1).cpu().numpy()
    finally:
        m._eps_override = None
    s = S.oracle_samples(m.architecture, state_of(m), x, y, aux, eps, torch.float64)
    mag = S.loglik_samples(x, s["x_mu"], s["x_lv"])[1][:, 0].mean()
    ref = (stat - S.C0) + SIZE * SIZE * S.C0
    got = out[:, 2].mean()
    print("mean ll", got, "from the loss", ref, "difference / sum|term|", abs(got - ref) / mag)
    assert abs(got - ref) <= 2e-5 * mag


def test_reconstruct_is_the_oracles_mean_at_the_posterior_mean(painter):
    m = painter.model
    x, y, aux, _ = inputs(m)
    zero = np.zeros((1, N, *m.dim_z), np.float32)
    s = S.oracle_samples(m.architecture, state_of(m), x, y, aux, zero, torch.float64)
    got = m.reconstruct(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, 1, SIZE, SIZE)
    got = got.cpu().numpy().astype(np.float64)
    for i in range(N):
        scale = np.abs(s["x_mu"][i]).max()
        err = np.abs(got[i] - s["x_mu"][i]).max()
        print("reconstruct tile", i, "err / max|ref|", err / scale)
        assert err <= 3e-7 * scale, (i, err / scale)
    # eps given, in either shape: the sample of ``score``'s plan at K = 1
    e = syn.synthetic_eps((1, N, *m.dim_z), seed=12)
    a = m.reconstruct(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux), eps=e).cpu().numpy()
    b = m.reconstruct(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux), eps=e[0]).cpu().numpy()
    assert np.array_equal(a, b) and not np.array_equal(a, got.astype(np.float32))


def test_training_mode_and_bad_arguments_are_refused(painter):
    m = painter.model
    x, y, aux, eps = inputs(m)
    args = (torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))
    m.train(True)
    try:
        with pytest.raises(RuntimeError):
            m.score(*args)
        with pytest.raises(RuntimeError):
            m.reconstruct(*args)
    finally:
        m.train(False)
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError):
            m.score(*args, draws=bad)
    with pytest.raises(ValueError):
        m.score(*args, draws=2, eps=eps)                               # (K, n, *dim_z) with K = 4
    with pytest.raises(ValueError):
        m.score(torch.from_numpy(x[:2]), args[1], args[2])
    with pytest.raises(ValueError):
        m.reconstruct(*args, eps=eps)
    assert math.isfinite(float(m.score(*args).sum()))
