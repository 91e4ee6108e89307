"""Inputs shared by tests/test_plane_kernels_host.py (CPU) and tests/test_gpu_plane_kernels.py (GPU): the tiles of
the ``regularise`` cases of bp_plane_blend / bp_plane_blend_fields, and the condition under which their masks cannot
depend on the last bit of a tile's statistics.  The CPU file asserts the condition on every case; the GPU file then
compares bits."""
import numpy as np

import plane_ref as R

TIE_BAND = 1e-9                                  # of a tile's std, on either side of the threshold std * regularise_std


def wide_tiles(shape, seed):
    """float32 tiles of both signs over many decades (exp(6 N(0, 1))): a reordered sum changes bits."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (np.exp(6.0 * rng.standard_normal(shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def narrow_tiles(shape, seed):
    """float32 tiles of N(1, 2): with a threshold of about one std a good part of every tile is masked."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.standard_normal(shape) * 2 + 1).astype(np.float32)


def integer_tile(tile, seed):
    """A tile of small integers whose sum is a multiple of tile^2: every partial sum is exact in float64 in any order,
    the mean is an integer, and several pixels equal it."""
    rng = np.random.Generator(np.random.PCG64(seed))
    tt = tile * tile
    p = rng.integers(-8, 9, tt)
    k = 0
    while p.sum() % tt:                          # walk the sum down to a multiple of tt, one unit at a time
        p[k % tt] -= 1
        k += 1
    return p.reshape(tile, tile).astype(np.float32)


def regularise_cases():
    """name -> (tiles (n, fields, tile, tile) float32, regularise_std).  tile^2 <= 289: the 4-ulp bound on the
    statistics is the tt 2^-52 summation bound at these sizes."""
    cases = {}
    for tile, seed in ((3, 20), (16, 21), (17, 22)):
        cases[f"narrow{tile}"] = (narrow_tiles((9, 1, tile, tile), seed), 1.5)
        cases[f"wide{tile}"] = (wide_tiles((9, 1, tile, tile), seed + 10), 0.75)
    cases["after_refusal"] = (narrow_tiles((4, 1, 3, 3), 12), 1.5)
    cases["fields3"] = (narrow_tiles((7, 3, 17, 17), 40), 1.25)
    t = narrow_tiles((4, 1, 17, 17), 41)
    t[1] = 1.5                                   # a constant tile: sums of 1.5 are exact, std 0, nothing masked
    cases["constant"] = (t, 1.5)
    t = narrow_tiles((4, 1, 16, 16), 42)
    for k in range(4):
        t[k, 0] = integer_tile(16, 50 + k)
    cases["zero_threshold"] = (t, 0.0)           # regularise_std = 0: all but the pixels equal to the mean are masked
    t = narrow_tiles((4, 1, 17, 17), 43)
    t[2, 0, 5, 11] = np.nan
    cases["nan"] = (t, 1.5)
    t = narrow_tiles((4, 1, 17, 17), 44)
    t[0, 0, 16, 0] = np.inf
    cases["inf"] = (t, 1.5)
    return cases


def exact_sums(p):
    """Every sum of the tile's pixels is exact in float64 whatever its order (small integers)."""
    p = np.asarray(p, np.float64)
    return bool(np.isfinite(p).all() and (p == np.round(p)).all() and np.abs(p).sum() < 2.0 ** 50)


def mask_is_safe(p, regularise_std):
    """True where a last-bit difference in the tile's mean or std cannot flip a pixel of its regularisation mask:
      * the statistics are not finite (a NaN or an inf in the tile): the mean is NaN or +-inf and the std NaN, every
        comparison |p - mean| > std * regularise_std has a NaN on one side and is false whatever the bits;
      * every sum of the tile is exact (small integers; a constant tile of 1.5 scaled likewise) and the threshold is
        exactly 0 (std 0 or regularise_std 0): the mean carries no rounding, so |p - mean| is exactly 0 or not;
      * otherwise no pixel lies within TIE_BAND * std of the threshold."""
    p = np.asarray(p, np.float64)
    m, s = R.device_tile_stats(p)
    if not (np.isfinite(m) and np.isfinite(s)):
        return bool(np.isnan(s) and not np.isfinite(m))
    if (s == 0.0 or regularise_std == 0.0) and exact_sums(p * 2.0):
        return bool(m == p.mean())
    return bool((np.abs(np.abs(p - m) - s * regularise_std) > TIE_BAND * s).all())
