"""GPU: ``bp_plane_moments`` (csrc/plane_moments.hip) through the C ABI against the float64 loop of
tests/plane_ensemble_ref.py, bit for bit: the register forms (K <= 4, K <= 16), their boundary and the two-pass form,
with and without weights, with and without the planes, on 16-byte and on 8-byte accesses over the same data, NaN where
no tile reaches and an infinite draw; and the guards, which write nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import plane_ensemble_ref as R
from baryon_painter_amd import _lib as L

import gpu_util as G

pytestmark = pytest.mark.gpu

COUNTS = [1, 7, 4096, 150 * 150 + 1]
DRAWS = [1, 2, 5, 16, 17, 64]
SENTINEL = -7.25


def _inputs(count, draws, special="both"):
    """acc of mixed sign over twenty-four decades, wsum positive over six; a band with acc == wsum == 0 (no tile
    reaches: NaN) and one infinite element, where ``count`` has room for them (``special`` places one of them in a
    single element)."""
    rng = np.random.Generator(np.random.PCG64([count, draws]))
    acc = rng.standard_normal((draws, count)) * 10.0 ** rng.integers(-12, 12, (draws, count))
    wsum = (rng.random((draws, count)) + 1e-3) * 10.0 ** rng.integers(-3, 3, (draws, count))
    if count >= 7:
        lo, hi = (1, 3) if count == 7 else (count // 3, count // 3 + 37)
        acc[:, lo:hi] = 0.0
        wsum[:, lo:hi] = 0.0
        acc[draws // 2, count - 2] = np.inf
    elif special == "nan":
        acc[:], wsum[:] = 0.0, 0.0
    elif special == "inf":
        acc[draws - 1, 0] = -np.inf
    return acc, wsum


class _Buffer:
    """A float64 device buffer of ``n`` elements that starts ``offset`` bytes (0 or 8) behind a 16-byte boundary, with
    a sentinel element on either side."""

    def __init__(self, n, offset, fill=None):
        self.store = torch.full((n + 4,), SENTINEL, dtype=torch.float64, device="cuda")
        assert self.store.data_ptr() % 16 == 0 and offset in (0, 8)
        first = 2 + offset // 8
        self.view = self.store[first:first + n]
        assert self.view.data_ptr() % 16 == offset
        if fill is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(fill).reshape(-1)))

    @property
    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def numpy(self, shape):
        return self.view.cpu().numpy().reshape(shape)

    def margins_untouched(self):
        s = self.store.cpu().numpy()
        inside = self.view.numel()
        first = (self.view.data_ptr() - self.store.data_ptr()) // 8
        return bool((s[:first] == SENTINEL).all() and (s[first + inside:] == SENTINEL).all())


def _run(acc, wsum, with_planes, offsets):
    """One launch; ``offsets`` = byte offsets of (acc, wsum, mean, var, planes).  Returns (mean, var, planes or None)
    as NumPy and the raw result tensors' bits."""
    draws, count = acc.shape
    a = _Buffer(draws * count, offsets[0], acc)
    w = _Buffer(draws * count, offsets[1], wsum) if wsum is not None else None
    mean, var = _Buffer(count, offsets[2]), _Buffer(count, offsets[3])
    planes = _Buffer(draws * count, offsets[4]) if with_planes else None
    rc = L.load().bp_plane_moments(a.ptr, w.ptr if w else None, draws, count, mean.ptr, var.ptr,
                                   planes.ptr if planes else None, G.stream())
    assert rc == L.BP_OK, rc
    torch.cuda.synchronize()
    for b in (a, w, mean, var, planes):
        assert b is None or b.margins_untouched()
    assert np.array_equal(a.numpy(acc.shape), acc, equal_nan=True)                 # the inputs are left as they were
    return mean.numpy((count,)), var.numpy((count,)), planes.numpy(acc.shape) if planes else None


ALIGNED, SHIFTED, MIXED = (0, 0, 0, 0, 0), (8, 8, 8, 8, 8), (0, 0, 8, 0, 0)


@pytest.mark.parametrize("draws", DRAWS)
@pytest.mark.parametrize("count", COUNTS)
def test_moments_equal_the_float64_loop(count, draws):
    for special in (("both",) if count > 1 else ("none", "nan", "inf")):
        acc, wsum = _inputs(count, draws, special)
        for weights in (wsum, None):
            P = R.quotients(acc, weights)
            m_ref, v_ref = R.moments(P)                          # one reference for every launch over these inputs
            if count >= 7 and weights is not None:
                assert np.isnan(m_ref).any() and np.isnan(P).any()
            if count >= 7:
                assert np.isinf(m_ref[count - 2]) and np.isnan(v_ref[count - 2])
            first = None
            for offsets in (ALIGNED, SHIFTED, MIXED):
                for with_planes in (True, False):
                    mean, var, planes = _run(acc, weights, with_planes, offsets)
                    what = (count, draws, special, weights is not None, offsets, with_planes)
                    assert R.same_bits(mean, m_ref) and R.same_bits(var, v_ref), what
                    if with_planes:
                        assert R.same_bits(planes, P), what
                    if draws == 1:
                        ok = np.isfinite(P[0])
                        assert (var[ok] == 0).all() and not np.signbit(var[ok]).any(), what
                        assert R.same_bits(mean, P[0]), what
                    # every launch over the same inputs gives the same bits, NaNs included
                    bits = (mean.view(np.uint64).copy(), var.view(np.uint64).copy())
                    if first is None:
                        first = bits
                        again = _run(acc, weights, with_planes, offsets)
                        assert np.array_equal(again[0].view(np.uint64), bits[0])
                        assert np.array_equal(again[1].view(np.uint64), bits[1])
                        assert np.array_equal(again[2].view(np.uint64), planes.view(np.uint64))
                    assert np.array_equal(bits[0], first[0]) and np.array_equal(bits[1], first[1]), what


def test_guards_write_nothing():
    lib = L.load()
    draws, count = 3, 64
    acc = torch.ones(draws * count, dtype=torch.float64, device="cuda")
    wsum = torch.ones_like(acc)
    mean = torch.full((count,), SENTINEL, dtype=torch.float64, device="cuda")
    var, planes = torch.full_like(mean, SENTINEL), torch.full_like(acc, SENTINEL)
    a, w, m, v, p = (L.ptr(t) for t in (acc, wsum, mean, var, planes))
    cases = [((None, w, draws, count, m, v, p), L.BP_EINVAL), ((a, w, draws, count, None, v, p), L.BP_EINVAL),
             ((a, w, draws, count, m, None, p), L.BP_EINVAL), ((a, w, 0, count, m, v, p), L.BP_EINVAL),
             ((a, w, -1, count, m, v, p), L.BP_EINVAL), ((a, w, draws, 0, m, v, p), L.BP_EINVAL),
             ((a, w, draws, -count, m, v, p), L.BP_EINVAL), ((a, None, 65, count, m, v, None), L.BP_EUNSUPPORTED),
             ((a, w, 65, count, m, v, p), L.BP_EUNSUPPORTED), ((a, w, 2 ** 31 - 1, count, m, v, p), L.BP_EUNSUPPORTED)]
    for args, code in cases:
        assert lib.bp_plane_moments(*args, G.stream()) == code, args
    torch.cuda.synchronize()
    for t in (mean, var, planes):
        assert bool((t == SENTINEL).all())
    # the limit itself is taken
    big = torch.ones(64 * count, dtype=torch.float64, device="cuda")
    assert lib.bp_plane_moments(L.ptr(big), None, 64, count, m, v, None, G.stream()) == L.BP_OK
    torch.cuda.synchronize()
    assert bool((mean == 1.0).all()) and bool((var == 0.0).all())
