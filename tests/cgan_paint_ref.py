"""The CGAN painter's field transform ("shift-log-cam") and its inverse, restated in float64 NumPy, and the two device
kernels built on them (bp_paint_load_cam / bp_paint_store_cam, csrc/paint.hip) as array expressions.

    t(x) = log(x / sigma + 1) / k0 - k1          t^-1(y) = (exp((y + k1) * k0) - 1) * sigma          K = (4, 1)
"""
import numpy as np

K = (4.0, 1.0)


def transform(x, sigma, k=K):
    return np.log(np.asarray(x, np.float64) / sigma + 1.0) / k[0] - k[1]


def inverse(y, sigma, k=K):
    return (np.exp((np.asarray(y, np.float64) + k[1]) * k[0]) - 1.0) * sigma


def load(raw_nchw, xf, aux=None):
    """bp_paint_load_cam before its rounding to float32: raw (n, c, h, w), xf (n, 3) {sigma, k0, k1}, aux (n, caux) or
    None -> (n, h, w, c + caux) float64, the aux values as constant planes behind the transformed channels."""
    raw = np.asarray(raw_nchw, np.float64)
    n, c, h, w = raw.shape
    xf = np.asarray(xf, np.float64)
    sig, k0, k1 = (xf[:, i, None, None, None] for i in range(3))
    out = (np.log(raw / sig + 1.0) / k0 - k1).transpose(0, 2, 3, 1)
    if aux is not None:
        planes = np.broadcast_to(np.asarray(aux, np.float64)[:, None, None, :], (n, h, w, np.shape(aux)[1]))
        out = np.concatenate([out, planes], axis=-1)
    return out


def store(y_nhwc, xf):
    """bp_paint_store_cam after its tanh and before its rounding to float32: y (n, h, w, c) network-domain values
    (the tanh already applied), xf (n, 3) {k0, k1, sigma} -> (n, c, h, w) float64."""
    y = np.asarray(y_nhwc, np.float64)
    xf = np.asarray(xf, np.float64)
    k0, k1, sig = (xf[:, i, None, None, None] for i in range(3))
    return ((np.exp((y + k1) * k0) - 1.0) * sig).transpose(0, 3, 1, 2)


def ulp32(x):
    """Spacing of float32 at |x| (of the smallest normal below it)."""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def ulps32(a, b):
    """Distance of two float32 arrays in units in the last place."""
    ia, ib = (np.asarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)
