"""CPU: tests/ymap_ref_orders.py -- the float64 restatement of SciPy's mirror zoom at spline orders 2 to 5 and the
emulation of csrc/ymap.hip's chunked prefilter with the kernel's own constants -- against SciPy, the warm-up lengths
against the poles they are derived from, and the order check of the device path (which needs no device to refuse)."""
import numpy as np
import pytest

import ymap_ref as R3
import ymap_ref_orders as R
from baryon_painter_amd import lightcone as LC

NEW = (2, 4, 5)


def _lognormal(shape, seed, sigma=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.exp(sigma * rng.standard_normal(shape))


@pytest.fixture(scope="module")
def line():
    """3000 samples of exp(3 N(0, 1)), three lines."""
    return _lognormal((3000, 3), 5, sigma=3.0)


@pytest.mark.parametrize("order", NEW)
@pytest.mark.parametrize("n,n_out", [(37, 20), (37, 37), (37, 50), (300, 257), (100, 333), (20, 64), (2, 7), (3, 9)])
def test_restatement_equals_scipy_mirror_zoom(order, n, n_out):
    """Down-sampling, unit zoom and up-sampling; 2 and 3 samples have fewer samples than taps.  SciPy's own arithmetic
    sets the floor: a plain sequential recursion is 1.3e-14 (order 4) and 7.4e-15 (order 5) of the maximum from
    spline_filter1d on the 3000-sample line (SciPy 1.15.3)."""
    nd = pytest.importorskip("scipy.ndimage")
    a = _lognormal((n, n), 100 + n + n_out)
    ref = nd.zoom(a, n_out / n, order=order, mode="mirror")
    assert ref.shape == (n_out, n_out)
    for chunked in (False, True):
        err = np.abs(R.zoom(a, n_out, order, chunked=chunked) - ref).max()
        assert err <= 1e-13 * np.abs(ref).max(), (chunked, err)


@pytest.mark.parametrize("order", NEW)
def test_restatement_equals_scipy_spline_filter1d(order, line):
    nd = pytest.importorskip("scipy.ndimage")
    ref = nd.spline_filter1d(line, order=order, axis=0, mode="mirror")
    err = np.abs(R.prefilter_lines(line, order) - ref).max() / np.abs(ref).max()
    print(f"order {order}: sequential recursion vs spline_filter1d {err:.2e} of the maximum")
    assert err <= 1e-13


def test_order_3_restatement_is_the_original():
    """Same poles, taps and weights as tests/ymap_ref.py; the gain is the literal 6 there and in the kernel."""
    a = _lognormal((40, 40), 3)
    assert R.gain(3) == 6.0 and R.poles(3) == (R3.Z,)
    assert np.array_equal(R.zoom(a, 33, 3), R3.zoom(a, 33))
    assert np.array_equal(R.zoom(a, 50, 3, chunked=True), R3.zoom(a, 50, chunked=True))


def test_poles_are_scipys_and_the_warm_ups_follow_from_them():
    """|z| ** warm <= 1e-18 per pole, with the smallest whole number of sub-chunks; the gain is the B-spline's."""
    for order, exact in [(2, 8.0), (3, 6.0), (4, 384.0), (5, 120.0)]:
        zs = R.poles(order)
        assert len(zs) == len(R.WARM[order]) == (1 if order < 4 else 2)
        assert all(-1.0 < z < 0.0 for z in zs)
        assert abs(R.gain(order) - exact) <= 1e-12 * exact
        for z, w in zip(zs, R.WARM[order]):
            need = np.log(R.TINY) / np.log(abs(z))
            assert abs(z) ** w <= R.TINY and w % R.SUB == 0 and w - R.SUB < need
        a = _lognormal((21, 21), order)                           # interpolation: a unit zoom gives the samples back
        assert np.abs(R.zoom(a, 21, order) - a).max() <= 1e-13 * a.max()
    assert abs(R.poles(5)[0]) ** 32 > 1e-12 and abs(R.poles(4)[0]) ** 32 > 1e-15       # 32 samples are not enough


# lines from just above the short-line threshold to 3000 samples: one below / at / above the halo + 1 and the chunk
LENGTHS = sorted({R.SHORT, R.SHORT + 1, 65, 96, 97, 98, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 2 * R.CHUNK + 1, 1000, 3000})


@pytest.mark.parametrize("order", NEW)
def test_chunked_emulation_equals_the_full_line(order, line):
    """The kernel's steps (pieces of CHUNK samples, a thread per SUB samples, warm-ups WARM[order]) against the unchunked
    recursion with SciPy's closed-form initialisations: <= 1e-15 of the largest value (measured: 3.4e-18, 1.7e-17 and
    6.8e-18 at orders 2, 4 and 5)."""
    worst = 0.0
    for n in LENGTHS:
        x = line[:n]
        full = R.prefilter_lines(x, order)
        got = R.prefilter_lines_chunked(x, order)
        worst = max(worst, np.abs(got - full).max() / np.abs(full).max())
    print(f"order {order}: chunked vs full line {worst:.2e} of the maximum")
    assert worst <= 1e-15


@pytest.mark.parametrize("order", (4, 5))
def test_a_16_sample_first_warm_up_is_not_enough(order, line):
    """Measured: off by 1.7e-9 (order 4) and 3.6e-8 (order 5) of the maximum."""
    full = R.prefilter_lines(line, order)
    top = np.abs(full).max()
    cut = np.abs(R.prefilter_lines_chunked(line, order, (16, R.WARM[order][1])) - full).max() / top
    print(f"order {order}: first warm-up 16 samples: {cut:.2e} of the maximum")
    assert cut > 1e-12
    assert np.abs(R.prefilter_lines_chunked(line, order, R.WARM[order]) - full).max() <= 1e-15 * top


@pytest.mark.parametrize("order", NEW)
def test_even_and_odd_orders_place_their_taps_as_scipy(order):
    """order + 1 taps from floor(c) - order // 2 (odd) or floor(c + 0.5) - order // 2 (even), weights sum to one."""
    ti, w = R.axis_weights(50, 37, order)
    assert ti.shape == w.shape == (37, order + 1)
    assert np.abs(w.sum(axis=1) - 1.0).max() <= 4e-16 and (w > -1e-16).all()
    cc = np.arange(37.0) * (49 / 36)
    first = np.floor(cc) - order // 2 if order & 1 else np.floor(cc + 0.5) - order // 2
    assert np.array_equal(ti[:, 0], R.mirror(first.astype(np.int64), 50))


def test_device_order_check():
    """Orders 2 to 5 pass the order check of the device path; 0, 1 and 6 are refused before anything else happens
    (no device is needed to be refused, and no random number is drawn)."""
    import torch
    planes, scales = [np.ones((8, 8))], [1.0]
    state = torch.get_rng_state()
    for order in (0, 1, 6):
        with pytest.raises(NotImplementedError):
            LC.project_planes(planes, scales, 8, order=order, on_device=True)
        with pytest.raises(NotImplementedError):
            LC.create_y_map(planes, [0.1], 8, 10.0, np.array([500.0]), lambda c: 1.0, 0.7, order=order, on_device=True)
        with pytest.raises(NotImplementedError):
            LC.paint_light_cone(object(), planes, [0.1], [100.0], 50.0, 8, 8, scales, order=order, on_device=True)
    assert torch.equal(torch.get_rng_state(), state)
    for order in (2, 3, 4, 5):
        assert order in LC._DEVICE_ORDERS
        # past the order check: a plane of the wrong shape is what is refused now
        with pytest.raises(TypeError):
            LC.project_planes([np.ones((8, 7))], scales, 8, order=order, on_device=True)
        # a painter without a device pipeline is refused for that, not for the order
        with pytest.raises(NotImplementedError, match="device paint pipeline"):
            LC.paint_light_cone(object(), planes, [0.1], [100.0], 50.0, 8, 8, scales, order=order, on_device=True)
    assert LC.project_planes([], [], 8, order=5, on_device=True).shape == (8, 8)      # no planes: nothing to launch
