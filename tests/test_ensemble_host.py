"""Host: the restatement of an ensemble's moments against NumPy's own, the new entry point's declaration, the block
layouts with and without ``draws``, the lattice ids of an ensemble's pixel noise, and the argument checks of
``paint_ensemble``, which come before any device work.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from baryon_painter_amd import _lib as L
from baryon_painter_amd.models import paint_graph as PG
from baryon_painter_amd.models.cvae import CVAE
from baryon_painter_amd.painter import CVAEPainter, _fill_block

import ensemble_ref as E

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("K", [1, 2, 5, 17, 64])
def test_the_restatement_agrees_with_numpy_to_a_few_ulp(K):
    """Positive data, u = eps / 2.  A sequential sum of K positive terms is within (K - 1) u of the exact one,
    relatively, NumPy's pairwise sum within log2(K) u, each division within u: the two means differ by less than
    K eps |mean|.  A mean that is off by d changes the sum of squared differences by 3 K d^2 at most (the differences
    from the exact mean sum to zero), and the K squares, K - 1 additions and the division round within (K + 3) u on
    either side: the variances differ by less than (K + 3) eps var + 3 (K eps mean)^2."""
    rng = np.random.Generator(np.random.PCG64([11, K]))
    p = np.exp(rng.standard_normal((7, K, 3, 5)) * 2.0).astype(np.float32)
    M, V = E.moments64(p)
    m_np, v_np = p.astype(np.float64).mean(axis=1), p.astype(np.float64).var(axis=1, ddof=0)
    eps = np.finfo(np.float64).eps
    err_m, err_v = np.abs(M - m_np) / (eps * m_np), np.abs(V - v_np)
    print("K", K, "mean: worst error in ulp", err_m.max(), "var: worst error over its bound",
          (err_v / ((K + 3) * eps * v_np + 3 * (K * eps * m_np) ** 2 + 1e-300)).max())
    assert (err_m <= K).all()
    assert (err_v <= (K + 3) * eps * v_np + 3 * (K * eps * m_np) ** 2).all()
    mean, var = E.moments(p)
    assert mean.dtype == var.dtype == np.float32 and mean.shape == (7, 3, 5)
    assert E.same_bits(mean, M.astype(np.float32)) and E.same_bits(var, V.astype(np.float32))
    if K == 1:
        assert (var == 0).all() and not np.signbit(var).any() and np.array_equal(mean, p[:, 0])


def test_non_finite_draws_propagate_as_numpy_does():
    p = np.ones((2, 3, 4), np.float32)
    p[0, 1, 0], p[1, 2, 1] = np.inf, np.nan
    mean, var = E.moments(p)
    with np.errstate(invalid="ignore"):
        m_np, v_np = p.astype(np.float64).mean(axis=1), p.astype(np.float64).var(axis=1)
    assert mean[0, 0] == np.inf and np.isnan(var[0, 0]) and np.isnan(mean[1, 1]) and np.isnan(var[1, 1])
    assert np.array_equal(mean, m_np.astype(np.float32), equal_nan=True)
    assert np.array_equal(var, v_np.astype(np.float32), equal_nan=True)
    assert E.same_bits(mean, mean.copy()) and not E.same_bits(mean, var)


def test_the_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(HERE), "include", "bp_hip.h")).read()
    declared = set(re.findall(r"\b(bp_[a-z0-9_]+)\s*\(", header))
    name = "bp_paint_store_moments"
    assert name in declared, f"{name} is not declared in bp_hip.h"
    assert name in L.SIGNATURES, f"{name} has no ctypes signature"
    assert hasattr(L.load(), name), f"{name} is not exported"
    args = re.search(rf"^int {name}\(([^;]*)\);", header, re.M).group(1)
    assert len(args.split(",")) == len(L.SIGNATURES[name][1]) == 13


def test_layouts_without_draws_are_unchanged_and_an_ensemble_block_holds_ids_per_sub_batch():
    n, w = 6, 4
    plain = PG.ParamBlock(PG.paint_fields(n, w, 1, xf_out_width=8))
    assert plain.layout == {"xf_in": (0, torch.float64, (n, w)), "xf_out": (192, torch.float64, (n, 8)),
                            "tile_ids": (576, torch.int64, (n,)), "seed": (624, torch.int64, (1,)),
                            "aux": (632, torch.float32, (n, 1))}
    assert plain.nbytes == 656
    noisy = PG.ParamBlock(PG.paint_fields(n, w, 1, xf_out_width=8, noise=True))
    assert noisy.layout["noise_ids"] == (656, torch.int64, (n,)) and noisy.layout["noise_org"] == (704, torch.int32, (n, 2))
    assert noisy.nbytes == 752
    for kw in ({"draws": None}, {"draws": None, "parts": 1}):
        assert PG.ParamBlock(PG.paint_fields(n, w, 1, xf_out_width=8, **kw)).layout == plain.layout
        assert PG.ParamBlock(PG.paint_fields(n, w, 1, xf_out_width=8, noise=True, **kw)).layout == noisy.layout
    # an ensemble: the five fields are per tile; without noise that is all
    assert PG.ParamBlock(PG.paint_fields(n, w, 1, xf_out_width=8, draws=5, parts=2)).layout == plain.layout
    ens = PG.ParamBlock(PG.paint_fields(n, w, 1, xf_out_width=8, noise=True, draws=5, parts=2))
    assert list(ens.layout) == list(plain.layout) + ["noise_ids"]
    assert ens.layout["noise_ids"] == (656, torch.int64, (2, 5, 3)) and ens.nbytes == 656 + 8 * 30
    # _fill_block: a short batch of 4 tiles in a block of 6, two sub-batches of 3 tiles, 5 draws
    hv = ens.views(torch.zeros(ens.nbytes, dtype=torch.uint8))
    N = 10
    params = {"xf_in": np.ones((N, w)), "xf_out": np.ones((N, 8)), "aux": np.zeros(N),
              "noise_ids": np.arange(N, dtype=np.int64) + 100}
    _fill_block(hv, params, np.arange(N, dtype=np.int64), 6, 10, n)
    tiles = np.array([106, 107, 108, 109, 109, 109])
    want = tiles.reshape(2, 1, 3) + (np.arange(5, dtype=np.int64) << 40).reshape(1, 5, 1)
    assert np.array_equal(hv["noise_ids"], want) and hv["tile_ids"].tolist() == [6, 7, 8, 9, 9, 9]


def test_ensemble_noise_ids_number_the_draws_above_bit_40():
    ids = PG.ensemble_noise_ids(np.array([0, 7, 2 ** 40 - 1]), 3)
    assert ids.dtype == np.int64 and ids.shape == (3, 3)
    assert ids.tolist() == [[0, 7, 2 ** 40 - 1], [2 ** 40, 2 ** 40 + 7, 2 ** 41 - 1], [2 ** 41, 2 ** 41 + 7, 3 * 2 ** 40 - 1]]
    assert PG.ensemble_noise_ids(np.array([5], np.uint64), 64)[63, 0] == 5 + (63 << 40)
    for bad in ([2 ** 40], [-1], [0.5], [[1, 2]]):
        with pytest.raises(ValueError):
            PG.ensemble_noise_ids(np.array(bad), 2)
    assert [PG.check_draws(k) for k in (1, 64, np.int64(5))] == [1, 64, 5]
    for bad in (0, 65, -1, 2.5):
        with pytest.raises(ValueError):
            PG.check_draws(bad)


class _StubModel:
    """What ``paint_ensemble`` may touch before it raises: nothing but the question whether there is a variance head.
    Everything else is an AttributeError, which would fail the test."""
    _need_var_head = CVAE._need_var_head

    def __init__(self, predict_var):
        self.predict_var = predict_var


def _stub_painter(predict_var):
    p = object.__new__(CVAEPainter)
    p.model = _StubModel(predict_var)
    return p


def test_paint_ensemble_checks_its_arguments_before_any_device_work():
    tiles, state = np.ones((4, 8, 8), np.float32), torch.get_rng_state()
    for p in (_stub_painter(True), _stub_painter(False)):
        for kw in ({"draws": 0}, {"draws": 65}, {"draws": -3}, {"draws": 3, "batch_size": 64},
                   {"draws": 16, "batch_size": 8}, {"draws": 5, "batch_size": 64}):
            with pytest.raises(ValueError):
                p.paint_ensemble(tiles, 0.3, **kw)
    # a noise id >= 2^40, explicit or taken from the tile ids; a negative one
    p = _stub_painter(True)
    for kw in ({"noise_ids": [0, 1, 2, 2 ** 40]}, {"tile_ids": [0, 1, 2, 2 ** 40]}, {"noise_ids": [0, 1, 2, -1]},
               {"noise_ids": [0, 1, 2]}):
        with pytest.raises(ValueError):
            p.paint_ensemble(tiles, 0.3, draws=4, batch_size=8, pixel_noise=True, **kw)
    # a painter without a variance head
    with pytest.raises(ValueError, match="no variance head"):
        _stub_painter(False).paint_ensemble(tiles, 0.3, draws=4, batch_size=8, pixel_noise=True)
    assert torch.equal(torch.get_rng_state(), state)
    # valid arguments reach the model (the stub has none of it): the checks above were the checks, not the stub
    with pytest.raises(AttributeError):
        p.paint_ensemble(tiles, 0.3, draws=4, batch_size=8, pixel_noise=True, noise_ids=[0, 1, 2, 2 ** 40 - 1])
