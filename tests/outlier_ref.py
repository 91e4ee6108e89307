"""A float64 NumPy restatement of the outlier count of ``bp_tile_outliers`` (include/bp_hip.h) and of the report built
on it: per image the mean, the population standard deviation, the number of pixels with ``abs(p - mean) > std * r``, and
the TIE BAND of that comparison -- the pixels whose distance from the mean is within 1e-9 (relative) of the threshold,
where summing in another order could decide the other way.  A test asserts that the band is empty for its inputs and
may then ask for equal counts."""
import numpy as np

TIE = 1e-9


def outliers(images, r, tie=TIE):
    """``images`` (n, ...) of any float type -> (mean (n,), std (n,), counts (n,) int32, ties (n,) int32), float64
    arithmetic.  NaN and infinite pixels give what NumPy gives: every comparison with a NaN is false."""
    x = np.asarray(images, dtype=np.float64).reshape(len(images), -1)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = x.mean(axis=1)
        std = np.sqrt(((x - mean[:, None]) ** 2).mean(axis=1))
        dist, limit = np.abs(x - mean[:, None]), (std * r)[:, None]
        counts = np.count_nonzero(dist > limit, axis=1).astype(np.int32)
        ties = np.count_nonzero(np.abs(dist - limit) <= tie * limit, axis=1).astype(np.int32)
    return mean, std, counts, ties


def problematic(counts, fields=1):
    """Tile numbers with a non-zero count in any of their ``fields`` images (row order t * fields + f)."""
    return np.flatnonzero((np.asarray(counts).reshape(-1, fields) != 0).any(axis=1))
