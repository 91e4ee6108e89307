"""The six range-compression modes as the device kernels evaluate them (csrc/range_compress.hpp), restated in NumPy:
record table in (``data_transforms.DeviceRangeCompress.records``), per-mode expression out, with the promotions of the
table in DESIGN.md -- forward entirely float64 and rounded to float32 once; inverse float32 until the np.float64
statistic enters.  Also the cases shared by tests/golden/make_goldens_range_modes.py (which feeds them to the
reference) and the tests (which feed them to this repository's code)."""
import collections

import numpy as np

MODES = ("shift-log", "log", "shift-log-2p", "log-tanh", "x/(1+x)", "1/x")
# two k settings per mode (Python floats / ints, as the training scripts write them)
K_SETS = {"shift-log": (4.0, 3), "log": (2.0, 5), "shift-log-2p": ((0.5, 3.0), (0.01, 4.0)), "log-tanh": (6.0, 9.5),
          "x/(1+x)": ((2.0, 1.0), (2, 1)), "1/x": (2.0, 0.75)}
EPS = 1e-3
FIELD = "dm"
REDSHIFTS = (0.0, 0.5, 2.0)
Z_CASES = (0.3, -0.2, 2.5)           # between two table entries, below the first, beyond the last
F32 = np.float32


def stats():
    """stats[field][z] with field- and redshift-dependent means and variances (Python floats)."""
    out = collections.OrderedDict()
    for fi, f in enumerate(("dm", "pressure")):
        out[f] = collections.OrderedDict(
            (z, {"mean": 0.4 + 0.3 * fi + 0.11 * zi, "var": 0.07 * (1 + fi) / (1 + zi)}) for zi, z in enumerate(REDSHIFTS))
    return out


def raw_tile(seed=5, n=32):
    """Positive float32 tile over four decades with 0, a negative value and NaN in it."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = np.exp(rng.random((n, n)) * 9.0 - 6.0)
    x[0, 0], x[0, 1], x[0, 2], x[1, 0], x[1, 1] = 0.0, -0.25, np.nan, -3.0, -1e-30
    return x.astype(F32)


def activation_tile(mode, k, seed=6, n=32, margin=0.05):
    """A float32 tile inside the domain of ``mode``'s inverse -- |y| <= 0.99 for log-tanh, y kept ``margin`` away from
    the pole k0 - k1 of x/(1+x) (where k0 / (y + k1) - 1 = 0) and from -k1 -- with the edge values y = -1, y < -1 and
    NaN in the first pixels (their branch results are compared exactly)."""
    rng = np.random.Generator(np.random.PCG64([seed, MODES.index(mode)]))
    u = rng.random((n, n))
    if mode == "log-tanh":
        y = u * 1.98 - 0.99
    elif mode == "x/(1+x)":
        y = -k[1] + margin + u * (k[0] - 2 * margin)          # (-k1, k0 - k1), the image of x > 0
    elif mode == "1/x":
        y = u * 1.9 - 0.95
    else:
        y = u * 3.0 - 1.5
    y[0, 0], y[0, 1], y[0, 2] = -1.0, -1.5, np.nan
    return y.astype(F32)


EDGE = (slice(0, 1), slice(0, 3))       # where activation_tile's edge values sit


def _f32(v):
    return F32(v)


def forward(mode, rec, x):
    """rec: one record {s, k, c, b}; x float32 -> float32."""
    s, k, c, b = (np.float64(v) for v in rec)
    x = np.asarray(x, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        if mode == "shift-log":
            v = np.log(x / s + 1.0) / k
        elif mode == "log":
            v = np.where(x > 0, np.log(x / s + c) / k, b)
        elif mode == "shift-log-2p":
            v = np.log(x / s + c) / k
        elif mode == "log-tanh":
            v = np.where(x > 0, np.tanh(np.log(x / s + c) / k), -1.0)
        elif mode == "x/(1+x)":
            v = x / (x + s) * k - c
        elif mode == "1/x":
            t = x / s
            v = np.where(t > -1, 2.0 / (t + 1.0) - 1.001, -1.0)
        else:
            raise ValueError(mode)
        return v.astype(F32)


def inverse(mode, rec, y):
    """rec: one record; y float32 -> float64 (what the host holds; the kernels store it rounded to float32).  NumPy's
    float32 exp / arctanh, as on the host: the kernels use the correctly rounded ones."""
    s, k, c, b = (np.float64(v) for v in rec)
    y = np.asarray(y, F32)
    kf, cf = _f32(k), _f32(c)
    with np.errstate(all="ignore"):
        if mode == "shift-log":
            return (np.exp(y * kf) - F32(1)).astype(np.float64) * s
        if mode == "log":
            return np.where(y.astype(np.float64) > b, (np.exp(y * kf) - cf).astype(np.float64) * s, 0.0)
        if mode == "shift-log-2p":
            return (np.exp(y * kf) - cf).astype(np.float64) * s
        if mode == "log-tanh":
            return np.where(y > F32(-1), (np.exp(np.arctanh(y) * kf) - cf).astype(np.float64) * s, 0.0)
        if mode == "x/(1+x)":
            return s / (kf / (y + cf) - F32(1)).astype(np.float64)
        if mode == "1/x":
            q = (F32(2) / (y + F32(1.001)) - F32(1)).astype(np.float64)
            return np.where(y >= F32(-1), q * b * c * k, 0.0)
    raise ValueError(mode)


def inverse_f64(mode, k, std, mean, eps, y):
    """The host formula with every operation in float64 on the float32 input: what the inverse's errors are measured
    against."""
    y = np.asarray(y, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        if mode == "shift-log":
            return (np.exp(y * k) - 1) * std
        if mode == "log":
            return np.where(y > np.log(eps) / k, (np.exp(y * k) - eps) * std, 0)
        if mode == "shift-log-2p":
            return (np.exp(y * k[1]) - k[0]) * std
        if mode == "log-tanh":
            return np.where(y > -1, (np.exp(np.arctanh(y) * k) - eps) * std, 0)
        if mode == "x/(1+x)":
            return std / (k[0] / (y + k[1]) - 1)
        if mode == "1/x":
            return np.where(y >= -1, (2 / (y + 1.001) - 1) * std * mean * k, 0)
    raise ValueError(mode)


def forward_tolerance(host):
    """One float32 spacing of the host value: the float64 evaluation is rounded once, so only a rounding boundary can
    move a value (plus 1e-14 for values at 0)."""
    return np.spacing(np.abs(np.asarray(host)).astype(F32)).astype(np.float64) + 1e-14


def cases(mode):
    """(sqrt_of_mean, index into Z_CASES) pairs of the fixture: every redshift without ``sqrt_of_mean``; with it every
    redshift for "1/x", the one mode that reads the mean, and the first for the others."""
    return [(False, zi) for zi in range(len(Z_CASES))] + \
        [(True, zi) for zi in range(len(Z_CASES) if mode == "1/x" else 1)]


def key(mode, ki, sqrt_of_mean, zi, direction):
    return f"{MODES.index(mode)}_k{ki}_s{int(sqrt_of_mean)}_z{zi}_{direction}"
