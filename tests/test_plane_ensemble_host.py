"""Host side of the plane and light-cone ensembles (lightcone.paint_plane_ensemble and its kin, csrc/plane_moments.hip):
the float64 loop the kernel is held to is the population variance, ``lightcone.ensemble_moments`` is that loop bit for
bit, the entry point is declared and bound, and the refusals that need no GPU are raised before any random number is
drawn."""
import os

import numpy as np
import pytest
import torch

import plane_ensemble_ref as R
from baryon_painter_amd import lightcone as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ulps64(a, b):
    ia, ib = (np.ascontiguousarray(v, np.float64).view(np.int64) for v in (a, b))
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFFFFFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFFFFFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("draws", [1, 2, 5, 16, 17, 64])
def test_reference_loop_is_mean_and_population_variance(draws):
    """Positive planes of one scale: a sequential sum of K <= 64 terms and NumPy's pairwise one differ by at most
    K - 1 roundings of the sum, and the variance inherits the mean's error only in second order."""
    rng = np.random.Generator(np.random.PCG64(draws))
    planes = rng.random((draws, 37, 41)) + 0.5
    mean, var = R.moments(planes)
    assert mean.dtype == var.dtype == np.float64 and mean.shape == (37, 41)
    assert _ulps64(mean, planes.mean(axis=0)).max() <= draws
    ref = planes.var(axis=0, ddof=0)
    assert np.abs(var - ref).max() <= 4 * draws * np.finfo(np.float64).eps * max(ref.max(), 1e-300)
    if draws == 1:
        assert np.array_equal(var, np.zeros_like(var)) and not np.signbit(var).any()
    else:
        assert (var > 0).all()
    # with weights: the planes are the quotients
    w = rng.random(planes.shape) + 0.25
    P = R.quotients(planes * w, w)
    assert R.same_bits(P, (planes * w) / w)
    assert all(R.same_bits(a, b) for a, b in zip(R.moments(P), R.moments((planes * w) / w)))


def _wild(draws, shape, seed):
    """Mixed signs over thirty decades, a band of NaN (0 / 0), one +inf and one -inf element."""
    rng = np.random.Generator(np.random.PCG64([seed, draws]))
    p = rng.standard_normal((draws, *shape)) * 10.0 ** rng.integers(-15, 15, (draws, *shape))
    flat = p.reshape(draws, -1)
    flat[:, 3:9] = np.nan
    flat[0, 11] = np.inf
    flat[draws - 1, 12] = -np.inf
    return p


@pytest.mark.parametrize("draws", [1, 2, 5, 16, 17, 64])
def test_ensemble_moments_is_the_reference_loop(draws):
    p = _wild(draws, (23, 19), 7)
    mean, var = LC.ensemble_moments(p)
    m, v = R.moments(p)
    assert R.same_bits(mean, m) and R.same_bits(var, v)
    flat_m, flat_v = mean.reshape(-1), var.reshape(-1)
    assert np.isnan(flat_m[3:9]).all() and np.isnan(flat_v[3:9]).all()
    assert np.isinf(flat_m[11]) and np.isnan(flat_v[11])            # inf - inf
    # what NumPy's own mean / var give at the non-finite elements
    with np.errstate(invalid="ignore", over="ignore"):
        assert np.array_equal(np.isnan(mean), np.isnan(p.mean(axis=0)))
        assert np.array_equal(np.isnan(var), np.isnan(p.var(axis=0)))
    # a list of planes and a float32 stack are taken as float64
    assert R.same_bits(LC.ensemble_moments(list(p))[1], v)
    p32 = np.abs(p[:, :4, :4]).astype(np.float32).clip(0, 1e30)
    p32[np.isnan(p32)] = 1.0
    assert R.same_bits(LC.ensemble_moments(p32)[0], R.moments(p32.astype(np.float64))[0])
    with pytest.raises(ValueError):
        LC.ensemble_moments(np.zeros((0, 3, 3)))


def test_entry_point_is_declared_and_bound():
    import ctypes as C

    from baryon_painter_amd import _lib as L
    with open(os.path.join(ROOT, "include", "bp_hip.h")) as f:
        header = f.read()
    assert "int bp_plane_moments(const double* acc, const double* wsum, int32_t draws, int64_t count, double* mean, " \
           "double* var," in header
    res, args = L.SIGNATURES["bp_plane_moments"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]
    assert hasattr(L.load(), "bp_plane_moments")
    assert os.path.exists(os.path.join(ROOT, "baryon_painter_amd", "csrc", "plane_moments.hip"))


class _NoLatent:
    """What a CGAN painter looks like to the ensembles: device pipelines, no ``paint_ensemble``."""
    label_fields = ["pressure"]

    def _device_paint_parameters(self, zs):
        raise AssertionError("not reached")

    def _paint_plane_device(self, *a, **k):
        raise AssertionError("not reached")

    _paint_small_plane_device = _paint_plane_device


class _Ensemble(_NoLatent):
    """A painter whose transforms have no ensemble pipeline."""

    def paint_ensemble(self, *a, **k):
        raise AssertionError("not reached")

    def _device_paint_parameters(self, zs, ensemble=False):
        assert ensemble
        raise NotImplementedError("no device form")


def _surfaces(painter, **kw):
    delta = np.ones((100, 100), np.float32)
    small = (np.ones((64, 64), np.float32), (0.1, 0.2), 128.0)
    yield lambda: LC.paint_plane_ensemble(painter, delta, 0.64, 64, 0.3, **kw)
    kw_small = {k: v for k, v in kw.items() if k != "batch_size"}
    yield lambda: LC.paint_small_plane_ensemble(painter, *small[:2], 32.0, 64.0, small[2], 64, 0.1, **kw_small)
    yield lambda: LC.paint_light_cone_ensemble(painter, [small, delta], [0.1, 0.3], [32.0, 100.0], 64.0, 64, 48,
                                               [1.0, 1.0], **kw)


@pytest.mark.parametrize("on_device", [False, True])
def test_refusals_need_no_gpu_and_draw_no_random_number(on_device):
    state = torch.get_rng_state()
    for draws in (0, 65, 2.5, -1):                               # PG.check_draws
        for call in _surfaces(_Ensemble(), draws=draws, on_device=on_device):
            with pytest.raises(ValueError, match="1 ... 64 draws"):
                call()
    for call in list(_surfaces(_Ensemble(), draws=3, batch_size=64, on_device=on_device))[::2]:
        with pytest.raises(ValueError, match="must divide"):    # 3 does not divide 64
            call()
    for call in list(_surfaces(_Ensemble(), draws=8, batch_size=4, on_device=on_device))[::2]:
        with pytest.raises(ValueError, match="must divide"):    # fewer samples than one tile's draws
            call()
    for call in _surfaces(_NoLatent(), draws=4, on_device=on_device):
        with pytest.raises(NotImplementedError, match="no latent"):
            call()
    for call in _surfaces(_Ensemble(), draws=4, on_device=on_device):
        with pytest.raises(NotImplementedError, match="no device form"):
            call()
    for call in list(_surfaces(_Ensemble(), draws=4, pixel_noise=True, on_device=on_device))[1:]:
        with pytest.raises(NotImplementedError, match="noise_org"):
            call()
    with pytest.raises(TypeError):                               # paint_plane_ensemble does not offer the argument
        LC.paint_plane_ensemble(_Ensemble(), np.ones((100, 100), np.float32), 0.64, 64, 0.3, 4, pixel_noise=True)
    assert torch.equal(torch.get_rng_state(), state)


def test_check_draws_is_the_tile_ensembles():
    from baryon_painter_amd.models import paint_graph as PG
    assert PG.check_draws(1) == 1 and PG.check_draws(64) == 64 and PG.DRAWS_MAX == 64
    for bad in (0, 65, 1.5):
        with pytest.raises(ValueError):
            PG.check_draws(bad)
