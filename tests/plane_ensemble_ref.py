"""NumPy restatement of ``bp_plane_moments`` (include/bp_hip.h): an explicit float64 loop over the draws, ascending,
every operation rounded once (NumPy never contracts a product into a sum):

    P_k = acc_k / wsum_k  (acc_k without weights),
    S = ((P_0 + P_1) + ...) + P_{K-1},  M = S / K,  Q = ((P_0 - M)^2 + (P_1 - M)^2) + ...,  mean = M,  var = Q / K

so that the kernel's float64 results, and ``lightcone.ensemble_moments``', can be compared bit for bit.  Written on its
own: it shares no code with ``lightcone.ensemble_moments``."""
import numpy as np


def quotients(acc, wsum=None):
    """The K planes P_k, float64 (K, ...): ``acc / wsum`` element by element (0 / 0 = NaN), or ``acc``."""
    acc = np.asarray(acc)
    assert acc.dtype == np.float64
    if wsum is None:
        return acc.copy()
    wsum = np.asarray(wsum)
    assert wsum.dtype == np.float64 and wsum.shape == acc.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.stack([acc[k] / wsum[k] for k in range(acc.shape[0])])


def moments(planes):
    """(mean, var) in float64 across axis 0 of the float64 ``planes``."""
    planes = np.asarray(planes)
    assert planes.dtype == np.float64 and planes.shape[0] >= 1
    draws = planes.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        total = planes[0]
        for k in range(1, draws):
            total = total + planes[k]
        mean = total / np.float64(draws)
        squares = (planes[0] - mean) * (planes[0] - mean)
        for k in range(1, draws):
            dev = planes[k] - mean
            squares = squares + dev * dev
        return mean, squares / np.float64(draws)


def same_bits(a, b):
    """Equal float64 bits, except that any NaN equals any NaN (a NaN's payload and sign are not pinned)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.float64 or b.dtype != np.float64 or a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan]))
