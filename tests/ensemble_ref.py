"""NumPy restatement of the moments of ``bp_paint_store_moments`` (include/bp_hip.h): an explicit float64 loop over the
draws, ascending, every operation rounded once (NumPy never contracts a product into a sum):

    S = ((p_0 + p_1) + ...) + p_{K-1},  M = S / K,  Q = ((p_0 - M)^2 + (p_1 - M)^2) + ...,
    mean = float32(M),  var = float32(Q / K)

so that the kernel's float32 results can be compared bit for bit."""
import numpy as np


def moments64(draws, axis=1):
    """(M, Q / K) in float64 over ``axis`` of the float32 array ``draws``."""
    p = np.moveaxis(np.asarray(draws), axis, 0)
    assert p.dtype == np.float32
    K = np.float64(p.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        S = p[0].astype(np.float64)
        for l in range(1, p.shape[0]):
            S = S + p[l].astype(np.float64)
        M = S / K
        Q = None
        for l in range(p.shape[0]):
            d = p[l].astype(np.float64) - M
            Q = d * d if Q is None else Q + d * d
        return M, Q / K


def moments(draws, axis=1):
    """(mean, var) as float32: ``moments64`` rounded once."""
    with np.errstate(invalid="ignore", over="ignore"):
        M, V = moments64(draws, axis)
        return M.astype(np.float32), V.astype(np.float32)


def same_bits(a, b):
    """Equal float32 bits, except that any NaN equals any NaN (a NaN's payload and sign are not pinned)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))
