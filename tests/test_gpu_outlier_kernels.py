"""GPU: the two kernels behind the problematic-tile report (csrc/plane.hip), through the C ABI.

``bp_tile_outliers`` against the float64 restatement of tests/outlier_ref.py: smooth random images, some with one to
three planted spikes (at the first, the last and a middle pixel) that the threshold must find and nothing else.  The
inputs are first shown to have an empty tie band (a condition on the fixed seeds, checked on the CPU), then the counts
must be EQUAL, and the statistics must be the bits ``bp_plane_blend(regularise=1)`` leaves for the same tiles.
``bp_tile_keep`` against its definition: two calls that share one cursor, the problematic tiles below, at and above
the cap."""
import ctypes as C

import numpy as np
import pytest
import torch

import gpu_util as G
import outlier_ref as R
from baryon_painter_amd import _lib as L

pytestmark = pytest.mark.gpu

STD = 2.0          # k <= 3 equal spikes among N >= 25 pixels stand sqrt((N - k) / k) >= 2.7 stds from the mean


def _images(n, tile, seed):
    """(n, tile, tile) float32: smooth fields around 3; image i carries i % 4 spikes of 1e3, the only pixels beyond the
    threshold in it (an image without a spike has some pixels of its own beyond 2 stds, which the restatement counts
    like the kernel).  Returns (images, spikes per image)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((n, tile + 2, tile + 2))
    x = (x[:, :-2, :-2] + x[:, 1:-1, 1:-1] + x[:, 2:, 2:] + x[:, :-2, 2:] + x[:, 2:, :-2]) / 5 + 3
    img = x.astype(np.float32).reshape(n, -1)
    spikes = np.arange(n) % 4
    where = [0, tile * tile - 1, tile * tile // 2]
    for i in range(n):
        img[i, where[:spikes[i]]] = 1e3
    return img.reshape(n, tile, tile), spikes


def _outliers(images, r, stream=None):
    lib = L.load()
    n, tile = images.shape[0], images.shape[-1]
    d = G.dev(images)
    stats = torch.full((2 * n,), -7.25, dtype=torch.float64, device="cuda")
    counts = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    L.check(lib.bp_tile_outliers(L.ptr(d), n, tile, float(r), L.ptr(stats), L.ptr(counts), G.stream()), "tile outliers")
    return stats, counts


def _blend_stats(images, r, weight=None):
    """What ``bp_plane_blend(regularise=1)`` leaves in ``stats`` for the images as n tiles stacked at the origin of a
    (tile, tile) plane; also its wsum."""
    lib = L.load()
    n, tile = images.shape[0], images.shape[-1]
    d = G.dev(images)
    dst = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    w = torch.ones((tile, tile), dtype=torch.float64, device="cuda") if weight is None else weight
    acc = torch.zeros((tile, tile), dtype=torch.float64, device="cuda")
    wsum = torch.zeros_like(acc)
    stats = torch.full((2 * n,), -7.25, dtype=torch.float64, device="cuda")
    L.check(lib.bp_plane_blend(L.ptr(d), n, tile, L.ptr(dst), 0, 0, tile, tile, L.ptr(w), 1, float(r), L.ptr(stats),
                               L.ptr(acc), L.ptr(wsum), tile, tile, G.stream()), "plane blend")
    return stats, wsum


@pytest.mark.parametrize("n", [1, 3, 70])
@pytest.mark.parametrize("tile", [5, 16, 17, 64])
def test_counts_equal_the_restatement_and_stats_equal_the_blend(tile, n):
    img, spikes = _images(n, tile, 100 * tile + n)
    mean, std, ref, ties = R.outliers(img, STD)
    assert not ties.any()                                        # (the inputs: no pixel sits on the threshold)
    has = spikes > 0
    assert np.array_equal(ref[has], spikes[has])                 # a spiked image: its spikes and nothing else
    stats, counts = _outliers(img, STD)
    got = counts.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, ref), (got, ref)
    s = stats.cpu().numpy().reshape(n, 2)
    assert np.abs(s[:, 0] - mean).max() <= 1e-12 * np.abs(mean).max()
    assert np.abs(s[:, 1] - std).max() <= 1e-12 * std.max()
    # the blend's own bits
    assert torch.equal(stats.view(torch.int64), _blend_stats(img, STD)[0].view(torch.int64))
    # the same inputs give the same bits
    again = _outliers(img, STD)
    assert torch.equal(again[0].view(torch.int64), stats.view(torch.int64)) and torch.equal(again[1], counts)


def test_nan_constant_and_infinite_images():
    tile = 17
    img = _images(4, tile, 7)[0]
    img[0, 3, 4] = np.nan
    img[1] = np.float32(0.1)                                     # (not a dyadic value: the mean must still be exact)
    img[2] = np.inf
    ref = R.outliers(img, STD)
    assert list(ref[2][:3]) == [0, 0, 0] and ref[2][3] == 3
    stats, counts = _outliers(img, STD)
    s = stats.cpu().numpy().reshape(4, 2)
    assert np.array_equal(counts.cpu().numpy(), ref[2])
    assert np.isnan(s[0]).all()
    assert s[1, 0] == np.float64(np.float32(0.1)) and s[1, 1] == 0.0
    assert s[2, 0] == np.inf and np.isnan(s[2, 1]) and np.isnan(ref[1][2])          # NumPy: inf - inf
    assert torch.equal(stats.view(torch.int64), _blend_stats(img, STD)[0].view(torch.int64))


@pytest.mark.parametrize("tile", [5, 64])
def test_the_blend_zeroes_exactly_the_counted_pixels(tile):
    img = _images(3, tile, 50 + tile)[0][2:]                     # one tile, two spikes
    _, counts = _outliers(img, STD)
    c = int(counts.cpu()[0])
    assert c == 2
    wsum = _blend_stats(img, STD)[1].cpu().numpy()
    assert set(np.unique(wsum)) == {0.0, 1.0} and wsum.sum() == tile * tile - c


def test_outlier_refusals_write_nothing():
    lib = L.load()
    tile = 16
    d = G.dev(_images(2, tile, 9)[0])
    stats = torch.full((4,), -7.25, dtype=torch.float64, device="cuda")
    counts = torch.full((2,), -5, dtype=torch.int32, device="cuda")
    t, s, c = L.ptr(d), L.ptr(stats), L.ptr(counts)
    cases = [((None, 2, tile, STD, s, c), L.BP_EINVAL), ((t, 2, tile, STD, None, c), L.BP_EINVAL),
             ((t, 2, tile, STD, s, None), L.BP_EINVAL), ((t, 0, tile, STD, s, c), L.BP_EINVAL),
             ((t, 2, 0, STD, s, c), L.BP_EINVAL), ((t, -1, tile, STD, s, c), L.BP_EINVAL),
             ((t, 2, tile, float("nan"), s, c), L.BP_EINVAL), ((t, 2, tile, float("inf"), s, c), L.BP_EINVAL),
             ((t, 2, tile, -1.0, s, c), L.BP_EINVAL),
             ((t, 2 ** 31 // 64 ** 2, 64, STD, s, c), L.BP_EUNSUPPORTED)]
    for args, code in cases:
        assert lib.bp_tile_outliers(*args, G.stream()) == code, args
    torch.cuda.synchronize()
    assert (stats == -7.25).all() and (counts == -5).all()
    assert lib.bp_tile_outliers(t, 2, tile, 0.0, s, c, G.stream()) == L.BP_OK        # (a threshold of 0 is one)


# ------------------------------------------------------------------------------------------------------- bp_tile_keep
CAP, FIRST = 3, 100
# the problematic tiles of two consecutive calls (4 and 3 tiles): below, at and above the cap -- which the first call
# fills exactly, or the second call straddles
PATTERNS = {"below": ([1], [2]), "equal": ([0, 3], [1]), "above": ([0, 2, 3], [0, 2]), "straddle": ([1, 2], [0, 1, 2])}


def _keep_case(fields, tile, pattern, seed, misalign=0):
    lib = L.load()
    rng = np.random.Generator(np.random.PCG64(seed))
    cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
    index = torch.full((CAP + 2,), -5, dtype=torch.int32, device="cuda")
    kraw = torch.full((CAP + 2, tile, tile), -7.25, device="cuda")
    kpaint = torch.full((CAP + 2, fields, tile, tile), -7.25, device="cuda")
    want, first, total = [], FIRST, 0
    for n, flagged in zip((4, 3), pattern):
        raw = rng.standard_normal((n, tile, tile)).astype(np.float32)
        painted = rng.standard_normal((n, fields, tile, tile)).astype(np.float32)
        counts = np.zeros((n, fields), dtype=np.int32)
        for i, t in enumerate(flagged):                          # the last field alone, or all fields
            counts[t, fields - 1] = 7 + t
            if i % 2:
                counts[t] = 1 + t
        rd = torch.zeros(raw.size + 1, device="cuda")             # (misalign = 1: the tiles begin 4 bytes off)
        rd[misalign:misalign + raw.size] = G.dev(raw).reshape(-1)
        pd, cd = G.dev(painted), G.dev(counts, torch.int32)
        L.check(lib.bp_tile_keep(C.c_void_p(rd.data_ptr() + 4 * misalign), L.ptr(pd), L.ptr(cd), n, fields, tile, first,
                                 CAP, L.ptr(cursor), L.ptr(index), L.ptr(kraw), L.ptr(kpaint), G.stream()), "tile keep")
        want += [(first + t, raw[t], painted[t]) for t in flagged]
        first += n
        total += len(flagged)
        assert int(cursor.cpu()[0]) == total                     # those beyond the cap are counted too
    kept = min(total, CAP)
    idx = index.cpu().numpy()
    assert list(idx[:kept]) == [w[0] for w in want[:kept]] and list(idx[:kept]) == sorted(idx[:kept])
    for s in range(kept):
        assert np.array_equal(kraw[s].cpu().numpy(), want[s][1]) and np.array_equal(kpaint[s].cpu().numpy(), want[s][2])
    assert (idx[kept:] == -5).all() and (kraw[kept:] == -7.25).all() and (kpaint[kept:] == -7.25).all()
    return index, kraw, kpaint


@pytest.mark.parametrize("name", list(PATTERNS))
@pytest.mark.parametrize("tile", [5, 16])
@pytest.mark.parametrize("fields", [1, 2])
def test_keep_fills_the_slots_in_order_and_counts_beyond_the_cap(fields, tile, name):
    _keep_case(fields, tile, PATTERNS[name], 31 * tile + fields)


def test_keep_copies_the_same_bits_from_unaligned_tiles():
    a = _keep_case(2, 16, PATTERNS["straddle"], 77)
    b = _keep_case(2, 16, PATTERNS["straddle"], 77, misalign=1)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_keep_refusals_write_nothing():
    lib = L.load()
    tile, n, fields = 16, 2, 1
    raw, painted = torch.ones((n, tile, tile), device="cuda"), torch.ones((n, fields, tile, tile), device="cuda")
    counts = torch.ones((n, fields), dtype=torch.int32, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
    index = torch.full((CAP,), -5, dtype=torch.int32, device="cuda")
    kraw = torch.full((CAP, tile, tile), -7.25, device="cuda")
    kpaint = torch.full((CAP, fields, tile, tile), -7.25, device="cuda")
    good = [L.ptr(raw), L.ptr(painted), L.ptr(counts), n, fields, tile, 0, CAP, L.ptr(cursor), L.ptr(index), L.ptr(kraw),
            L.ptr(kpaint)]
    bad = [(i, None, L.BP_EINVAL) for i in (0, 1, 2, 8, 9, 10, 11)]
    bad += [(3, 0, L.BP_EINVAL), (4, 0, L.BP_EINVAL), (5, 0, L.BP_EINVAL), (6, -1, L.BP_EINVAL), (7, -1, L.BP_EINVAL),
            (3, 65536, L.BP_EUNSUPPORTED), (6, 2 ** 31 - 2, L.BP_EUNSUPPORTED)]
    for i, v, code in bad:
        args = list(good)
        args[i] = v
        assert lib.bp_tile_keep(*args, G.stream()) == code, (i, v)
    big = list(good)
    big[3], big[5] = 2 ** 31 // 64 ** 2, 64
    assert lib.bp_tile_keep(*big, G.stream()) == L.BP_EUNSUPPORTED
    torch.cuda.synchronize()
    assert int(cursor.cpu()[0]) == 0 and (index == -5).all() and (kraw == -7.25).all() and (kpaint == -7.25).all()
