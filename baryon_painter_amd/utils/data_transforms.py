"""Field transforms applied before / after the network (NumPy, host side).

Same call signature ``f(x, field, z, stats)`` and the same mode names as the reference
(/root/reference/baryon_painter/utils/data_transforms.py:14-119), the split-scale (Gaussian
pyramid) transform of data_transforms.py:14-42 included (its device form: csrc/scales.hip).
``stats[field][z] -> {"mean", "var"}`` is tabulated per training redshift and linearly
interpolated in z (clamped at both ends), data_transforms.py:52-64.
"""
import numpy as np


class _Chain:
    def __init__(self, steps):
        self.steps = list(steps)

    def __call__(self, x, field, z, stats):
        for t in self.steps:
            x = t(x, field, z, stats)
        return x


def chain_transformations(transformations):
    """Apply the given transforms one after the other (data_transforms.py:44-49)."""
    return _Chain(transformations)


def interpolate_z(stats_of_field, z):
    """Statistics at redshift z: linear between the bracketing tabulated redshifts,
    the last entry at/after the last tabulated z, the first entry below the first."""
    zs = list(stats_of_field.keys())
    idx = int(np.searchsorted(zs, z, side="right"))
    if idx >= len(zs):
        return stats_of_field[zs[-1]]
    if idx <= 0:
        return stats_of_field[zs[0]]
    lo, hi = zs[idx - 1], zs[idx]
    w = (z - lo) / (hi - lo)
    return {k: w * stats_of_field[hi][k] + (1 - w) * stats_of_field[lo][k] for k in stats_of_field[zs[0]]}


def interpolate_z_many(stats_of_field, zs, key="var"):
    """``interpolate_z(stats_of_field, z)[key]`` for an array of redshifts at once -- the same float64 arithmetic
    element by element (w * hi + (1 - w) * lo, clamped at both ends), without a Python call per tile
    (paint_stream: 100k tiles)."""
    tab = np.array(list(stats_of_field.keys()), dtype=np.float64)
    val = np.array([stats_of_field[z][key] for z in stats_of_field.keys()], dtype=np.float64)
    zs = np.asarray(zs, dtype=np.float64)
    idx = np.searchsorted(tab, zs, side="right")
    i1 = np.clip(idx, 1, len(tab) - 1) if len(tab) > 1 else np.zeros_like(idx)
    i0 = i1 - 1 if len(tab) > 1 else i1
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (zs - tab[i0]) / (tab[i1] - tab[i0]) if len(tab) > 1 else np.zeros_like(zs)
        out = w * val[i1] + (1 - w) * val[i0]
    out = np.where(idx >= len(tab), val[-1], out)
    return np.where(idx <= 0, val[0], out)


# mode -> (forward, inverse); each takes (x, k, std, mean, eps).  Formulas: data_transforms.py:72-108.
_MODES = {
    "log": (lambda x, k, std, mean, eps: np.where(x > 0, np.log(x / std + eps) / k, np.log(eps) / k),
            lambda y, k, std, mean, eps: np.where(y > np.log(eps) / k, (np.exp(y * k) - eps) * std, 0)),
    "shift-log": (lambda x, k, std, mean, eps: np.log(x / std + 1) / k,
                  lambda y, k, std, mean, eps: (np.exp(y * k) - 1) * std),
    "shift-log-2p": (lambda x, k, std, mean, eps: np.log(x / std + k[0]) / k[1],
                     lambda y, k, std, mean, eps: (np.exp(y * k[1]) - k[0]) * std),
    "log-tanh": (lambda x, k, std, mean, eps: np.where(x > 0, np.tanh(np.log(x / std + eps) / k), -1),
                 lambda y, k, std, mean, eps: np.where(y > -1, (np.exp(np.arctanh(y) * k) - eps) * std, 0)),
    "x/(1+x)": (lambda x, k, std, mean, eps: x / (x + std) * k[0] - k[1],
                lambda y, k, std, mean, eps: std / (k[0] / (y + k[1]) - 1)),
    "1/x": (lambda x, k, std, mean, eps: np.where(x / (std * mean * k) > -1, 2 / (x / (std * mean * k) + 1) - 1.001, -1),
            lambda y, k, std, mean, eps: np.where(y >= -1, (2 / (y + 1.001) - 1) * std * mean * k, 0)),
}


class _RangeCompress:
    """One direction of a range-compression transform; a picklable callable ``f(x, field, z, stats)``."""

    def __init__(self, k_values, modes, eps, sqrt_of_mean, direction):
        self.k_values, self.modes, self.eps = dict(k_values), dict(modes), eps
        self.sqrt_of_mean, self.direction = sqrt_of_mean, direction

    def __call__(self, x, field, z, stats):
        mode = self.modes[field]
        if mode.lower() not in _MODES:
            raise ValueError(f"Mode '{mode}' not supported.")
        s = interpolate_z(stats[field], z)
        mean = np.sqrt(s["mean"]) if self.sqrt_of_mean else s["mean"]
        return _MODES[mode.lower()][self.direction](x, self.k_values[field], np.sqrt(s["var"]), mean, self.eps)


def create_range_compress_transforms(k_values, modes={}, eps=1e-3, sqrt_of_mean=False):
    """(transform, inverse) pair for the reference's range-compression modes
    (data_transforms.py:51-110): "log", "shift-log", "shift-log-2p", "log-tanh", "x/(1+x)", "1/x"."""
    return (_RangeCompress(k_values, modes, eps, sqrt_of_mean, 0),
            _RangeCompress(k_values, modes, eps, sqrt_of_mean, 1))


def gaussian_radius(sigma, truncate=3.0):
    """Half width of scipy.ndimage.gaussian_filter1d's kernel."""
    return int(truncate * float(sigma) + 0.5)


def gaussian_weights(sigma, truncate=3.0):
    """The float64 weights scipy.ndimage.gaussian_filter1d(order=0) correlates with: exp(-0.5 / sigma^2 * k^2) for
    k = -r .. r, divided by their float64 sum (``csrc/scales.hip`` reads these from device memory)."""
    r = gaussian_radius(sigma, truncate)
    sigma2 = float(sigma) * float(sigma)
    k = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / sigma2 * k ** 2)
    return phi / phi.sum()


def split_scale_sigmas(n_scale, step_size):
    """sigma of level i = 1 .. n_scale-1 (index 0 is unused: level 0 is the residual)."""
    return [0.0] + [step_size ** i / 2 for i in range(1, n_scale)]


class _SplitScale:
    """One direction of the split-scale (Gaussian pyramid) transform (data_transforms.py:14-42); a picklable
    callable ``f(x, field, z, stats)``.

    Forward: d = x.copy(); for i = n_scale-1 .. 1: g = gaussian_filter(d, sigma=step_size**i / 2, truncate); scale i
    = g; d -= g.  Scale 0 is what is left of d.  ``include_original`` puts x itself in a leading extra channel.  What
    SciPy's filter does on a float32 tile is part of the result: axis 0 first, then axis 1; each axis accumulates in
    float64 over the weights of ``gaussian_weights`` and is rounded to float32 once; boundary "reflect"
    (d c b a | a b c d, folded with period 2n when the radius exceeds the line); the subtraction is the array's own
    (float32 for a float32 tile).
    Inverse: channel 0 with ``include_original``, the sum over the channels otherwise; RuntimeError on a wrong channel
    count."""

    def __init__(self, n_scale, step_size, include_original, truncate, direction):
        self.n_scale, self.step_size = int(n_scale), step_size
        self.include_original, self.truncate, self.direction = bool(include_original), truncate, direction

    @property
    def levels(self):
        return self.n_scale + int(self.include_original)

    def __call__(self, x, field, z, stats):
        return self._inverse(x) if self.direction else self._forward(x)

    def _forward(self, x):
        from scipy.ndimage import gaussian_filter
        inc = int(self.include_original)
        d_in = x.copy()
        d_out = np.zeros((self.n_scale + inc, *x.shape[-2:]), dtype=x.dtype)
        if inc:
            d_out[0] = x
        for i in range(self.n_scale - 1, 0, -1):
            d_out[i + inc] = gaussian_filter(d_in, sigma=self.step_size ** i / 2, truncate=self.truncate)
            d_in -= d_out[i + inc]
        d_out[inc] = d_in
        return d_out

    def _inverse(self, x):
        if x.shape[0] != self.levels:
            raise RuntimeError(f"Invalid shape of input. Expected x.shape[0] == {self.levels} but got {x.shape[0]}.")
        return x[0] if self.include_original else x.sum(axis=0)


def create_split_scale_transform(n_scale=3, step_size=4, include_original=True, truncate=3.0):
    """(transform, inverse) pair of the reference's split-scale transform (data_transforms.py:14-42)."""
    return (_SplitScale(n_scale, step_size, include_original, truncate, 0),
            _SplitScale(n_scale, step_size, include_original, truncate, 1))


def atleast_3d(x, field, z, stats):
    return x.reshape(1, *x.shape) if x.ndim == 2 else x


def squeeze(x, field, z, stats):
    return x.squeeze()


def as_float32(x, field, z, stats):
    """Keep tiles float32: under NumPy >= 2 promotion ``float32_array / np.float64_scalar`` yields
    float64, whereas the NumPy 1.x the reference was written for kept float32."""
    return np.asarray(x, dtype=np.float32)


# ---- which chains have a device form (painter.CVAEPainter.paint_stream, datasets.DeviceTileAssembler) --------------
def chain_steps(func):
    """The steps of a transform function: those of a chain, or the function itself."""
    return getattr(func, "steps", None) or [func]


def is_shape_only(st):
    """atleast_3d / squeeze / as_float32 (by name: a chain restored from a checkpoint holds re-imported functions)."""
    return getattr(st, "__module__", None) == __name__ and \
        getattr(st, "__name__", None) in ("atleast_3d", "squeeze", "as_float32")


def has_split_scale(func):
    return func is not None and any(isinstance(st, _SplitScale) for st in chain_steps(func))


# mode name -> mode number of the device kernels (csrc/range_compress.hpp, BP_RC_* of include/bp_hip.h)
MODE_IDS = {"shift-log": 0, "log": 1, "shift-log-2p": 2, "log-tanh": 3, "x/(1+x)": 4, "1/x": 5}


class DeviceRangeCompress:
    """A chain's range compression of one field as the device kernels take it: ``name`` / ``mode`` (the mode and its
    number) and ``records(stats_of_field, zs)``, the (n, 4) float64 table {s, k, c, b} of csrc/range_compress.hpp for an
    array of redshifts.  Every constant a kernel uses is computed here, in float64, with the host lambdas' own
    expressions (``std * mean * k``, ``np.log(eps) / k``), so both sides share them to the bit.  Compares equal to the
    shift-log ``k`` it was read from (callers of ``device_shift_log`` from before the other modes had a device form)."""

    def __init__(self, st, field):
        name = st.modes[field].lower()
        if name not in _MODES:
            raise ValueError(f"Mode '{st.modes[field]}' not supported.")
        k = st.k_values[field]
        two = name in ("shift-log-2p", "x/(1+x)")
        ks = list(k) if two else [k]
        if (two and len(ks) != 2) or (name != "shift-log" and not all(type(v) in (int, float) for v in ks + [st.eps])):
            # NumPy scalars promote differently from Python floats in the host expressions the kernels restate
            raise NotImplementedError(f"the device form of '{name}' needs Python-float k and eps, got {k!r}, {st.eps!r}")
        self.name, self.mode = name, MODE_IDS[name]
        self.k = [float(v) for v in ks]
        self.eps, self.sqrt_of_mean = float(st.eps), bool(st.sqrt_of_mean)

    def __eq__(self, other):
        return self.k[0] == other if isinstance(other, (int, float)) else NotImplemented

    __hash__ = None

    def __float__(self):
        return self.k[0]

    def records(self, stats_of_field, zs):
        zs = np.atleast_1d(np.asarray(zs, dtype=np.float64))
        rec = np.zeros((len(zs), 4), np.float64)
        std = np.sqrt(interpolate_z_many(stats_of_field, zs, "var"))
        rec[:, 0], rec[:, 1] = std, self.k[-1] if self.name == "shift-log-2p" else self.k[0]
        if self.name in ("log", "log-tanh"):
            rec[:, 2] = self.eps
            rec[:, 3] = np.log(self.eps) / self.k[0]
        elif self.name == "shift-log-2p":
            rec[:, 2] = self.k[0]
        elif self.name == "x/(1+x)":
            rec[:, 2] = self.k[1]
        elif self.name == "1/x":
            mean = interpolate_z_many(stats_of_field, zs, "mean")
            mean = np.sqrt(mean) if self.sqrt_of_mean else mean
            rec[:, 0], rec[:, 2], rec[:, 3] = std * mean * self.k[0], mean, std
        return rec


def device_shift_log(func, direction, field):
    """The ONE range compression of a single-scale chain whose other steps are shape-only, in any order, as a
    ``DeviceRangeCompress`` (any of the six modes; ValueError for an unknown mode name, as on the host);
    NotImplementedError for every other chain."""
    found = None
    for st in chain_steps(func):
        if isinstance(st, _RangeCompress) and st.direction == direction and found is None:
            found = DeviceRangeCompress(st, field)
        elif not is_shape_only(st):
            # a custom scaling step in the chain would be silently dropped on the device path
            raise NotImplementedError(f"transform step {st!r} has no device form")
    if found is None:
        raise NotImplementedError("the device path needs the chain's range compression")
    return found


def device_split_scale(func, direction, field):
    """(range compression, split-scale step) of a multi-scale chain in the strict orders the kernels implement,
         forward  [range compression, as_float32 (optional), split-scale, shape-only steps ...]
         inverse  [inverse split-scale, inverse range compression, shape-only steps ...]
    -- exactly these: the kernels filter the transformed tile and sum in front of the inverse transform.  The range
    compression is a ``DeviceRangeCompress``, as from ``device_shift_log``."""
    steps = list(chain_steps(func))
    if direction == 0:
        head = [lambda st: isinstance(st, _RangeCompress) and st.direction == 0]
        if len(steps) > 1 and getattr(steps[1], "__name__", None) == "as_float32" and is_shape_only(steps[1]):
            head.append(is_shape_only)
        head.append(lambda st: isinstance(st, _SplitScale) and st.direction == 0)
    else:
        head = [lambda st: isinstance(st, _SplitScale) and st.direction == 1,
                lambda st: isinstance(st, _RangeCompress) and st.direction == 1]
    if len(steps) < len(head) or not all(ok(st) for ok, st in zip(head, steps)) or \
            not all(is_shape_only(st) for st in steps[len(head):]):
        raise NotImplementedError(
            "a split-scale chain has a device form only as [range compression, as_float32 (optional), split-scale, "
            "shape-only steps] / [inverse split-scale, inverse range compression, shape-only steps]; got "
            f"{[getattr(st, '__name__', type(st).__name__) for st in steps]}")
    rc = next(st for st in steps if isinstance(st, _RangeCompress))
    return DeviceRangeCompress(rc, field), next(st for st in steps if isinstance(st, _SplitScale))


def split_scale_tables(n_scale, step_size, truncate):
    """(radii, weights) as bp_split_scale reads them: radii[i] of level i (entry 0 unused), and the float64 weights of
    level 1, 2, ... back to back."""
    sig = split_scale_sigmas(n_scale, step_size)
    radii = [0] + [gaussian_radius(s, truncate) for s in sig[1:]]
    weights = np.concatenate([np.zeros(0)] + [gaussian_weights(s, truncate) for s in sig[1:]])
    return radii, np.ascontiguousarray(weights, np.float64)
