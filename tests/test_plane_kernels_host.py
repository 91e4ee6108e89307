"""Host side of tests/test_gpu_plane_kernels.py: the float64 restatements that the kernels of csrc/plane.hip are
compared with (tests/plane_ref.py) are pinned here, on the CPU, to something independent of them.

  * prefilter_line solves the cubic-spline system under half-sample symmetric boundaries exactly (dense solve);
  * zoom is scipy.ndimage.zoom(order=3, mode="reflect") for lines of 12 samples and more, and NOT below: SciPy's own
    "reflect" prefilter departs from the exact solve on short lines (its causal initialisation is truncated), by the
    amounts that test_scipy_departs_from_the_exact_spline_on_short_lines prints;
  * device_tile_stats (tile_stats_kernel's order) against the two-pass statistics;
  * blend_box (blend_kernel per pixel) against the host loop of plane_ref.blend;
  * the inputs of the GPU file's ``regularise`` cases keep every pixel out of the tie band of the threshold, so that the
    GPU file may compare bits."""
import numpy as np
import pytest

import plane_cases as PC
import plane_ref as R
from baryon_painter_amd import lightcone as LC


def _line(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal(n)


@pytest.mark.parametrize("n", list(range(2, 17)) + [33])
def test_prefilter_is_the_exact_spline_solve(n):
    s = _line(n, 100 + n)
    c = s.copy()
    R.prefilter_line(c)
    ref = R.exact_prefilter_line(s)
    err = np.abs(c - ref).max()
    print(f"n = {n}: max |prefilter_line - dense solve| = {err / np.abs(ref).max():.2e} of max |c|")
    assert err <= 1e-13 * np.abs(ref).max()
    # the coefficients reproduce the samples: (c[k-1] + 4 c[k] + c[k+1]) / 6 = s[k] with the end coefficients repeated
    e = np.concatenate([c[:1], c, c[-1:]])
    assert np.abs((e[:-2] + 4 * e[1:-1] + e[2:]) / 6 - s).max() <= 1e-13 * np.abs(s).max()


def test_prefilter_of_all_lines_at_once_is_line_by_line():
    a = np.random.Generator(np.random.PCG64(5)).standard_normal((33, 33))
    c = a.copy()
    for j in range(33):
        line = c[:, j].copy()
        R.prefilter_line(line)
        c[:, j] = line
    for i in range(33):
        line = c[i].copy()
        R.prefilter_line(line)
        c[i] = line
    assert np.array_equal(c, R.prefilter(a))


@pytest.mark.parametrize("n_in,n_out", [(12, 16), (31, 32), (33, 32), (65, 64), (129, 16), (200, 3)])
def test_zoom_restatement_is_scipy_zoom_from_12_samples(n_in, n_out):
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.Generator(np.random.PCG64(n_in))
    a = np.exp(rng.standard_normal((n_in, n_in)) * 0.5) * 0.05 - 0.04
    ref = nd.zoom(a, n_out / n_in, order=3, mode="reflect")
    got = R.zoom(a, n_out)
    assert ref.shape == got.shape == (n_out, n_out)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{n_in} -> {n_out}: max |restatement - scipy| = {err:.2e} of max |ref|")
    assert err <= 1e-12


def _exact_zoom(a, n_out):
    """plane_ref.zoom with the dense solve in place of prefilter_line."""
    c = np.stack([R.exact_prefilter_line(col) for col in a.T], axis=1)
    c = np.stack([R.exact_prefilter_line(row) for row in c], axis=0)
    ti, wi = R.axis_weights(a.shape[0], n_out)
    out = np.zeros((n_out, n_out))
    for p in range(4):
        rows = c[ti[:, p]]
        inner = np.zeros((n_out, n_out))
        for q in range(4):
            inner += wi[None, :, q] * rows[:, ti[:, q]]
        out += wi[:, p, None] * inner
    return out


def test_scipy_departs_from_the_exact_spline_on_short_lines():
    """Records (prints) how far scipy.ndimage.zoom(order=3, mode="reflect") lies from the exact cubic spline for lines
    of 2 ... 10 samples (and 12, 14, where it has converged), relative to max |ref|; asserts only that the restatement
    the kernel follows is the one that matches the dense solve.  Measured on the CPU with SciPy 1.15.3: 5.9e-4, 1.3e-4,
    6.5e-6, 3.1e-7, 5.0e-8, 2.0e-9, 2.7e-10, 1.0e-11, 4.6e-13 at 2 ... 10, 7.2e-15 at 12 (DESIGN.md section 10 has the
    table)."""
    try:
        import scipy
        import scipy.ndimage as nd
    except ImportError:
        nd = None
    for n_in in (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14):
        rng = np.random.Generator(np.random.PCG64(300 + n_in))
        a = np.exp(rng.standard_normal((n_in, n_in)) * 0.5) * 0.05 - 0.04
        n_out = 16
        got, ref = R.zoom(a, n_out), _exact_zoom(a, n_out)
        top = np.abs(ref).max()
        line = f"n_in = {n_in:2d}: restatement - exact = {np.abs(got - ref).max() / top:.1e}"
        if nd is not None:
            sp = nd.zoom(a, n_out / n_in, order=3, mode="reflect")
            line += f", scipy {scipy.__version__} - exact = {np.abs(sp - ref).max() / top:.1e}" \
                    f", scipy - restatement = {np.abs(sp - got).max() / top:.1e}"
        print(line)
        assert np.abs(got - ref).max() <= 1e-13 * top, n_in


@pytest.mark.parametrize("tile", [1, 2, 3, 16, 17])
@pytest.mark.parametrize("kind", ["narrow", "wide"])
def test_device_statistics_restate_the_two_pass_statistics(tile, kind):
    make = PC.narrow_tiles if kind == "narrow" else PC.wide_tiles
    for p in make((6, tile, tile), 60 + tile):
        tt = tile * tile
        m, s = R.device_tile_stats(p)
        m2, s2 = R.tile_stats(p)
        bound = tt * 2.0 ** -52 * np.abs(p.astype(np.float64)).mean()
        assert abs(m - m2) <= bound, (m, m2, bound)
        assert abs(s - s2) <= tt * 2.0 ** -52 * s2, (s, s2)


def test_device_statistics_of_exact_and_non_finite_tiles():
    assert R.device_tile_stats(np.full((17, 17), 1.5, np.float32)) == (1.5, 0.0)
    p = PC.integer_tile(16, 50)
    m, s = R.device_tile_stats(p)
    assert m == p.astype(np.float64).mean() == np.round(m) and (p == m).sum() >= 2 and s > 0
    p = PC.narrow_tiles((17, 17), 1)
    p[3, 4] = np.nan
    assert all(np.isnan(v) for v in R.device_tile_stats(p))
    p[3, 4] = np.inf
    m, s = R.device_tile_stats(p)
    assert m == np.inf and np.isnan(s)


def _geometry():
    n_tile, n_plane = 16, 40
    geo = LC.plane_geometry(n_plane, n_tile / n_plane, n_tile)
    return n_tile, n_plane, geo["dst"], LC.make_weight_map((n_tile, n_tile), falloff=0.3, sigma=0.5)


def test_blend_box_over_everything_is_the_host_loop():
    n_tile, n_plane, dst, w = _geometry()
    tiles = PC.wide_tiles((len(dst), n_tile, n_tile), 6)
    z = np.zeros((n_plane, n_plane))
    for reg in (None, 1.5):
        # plane_ref.blend takes the two-pass statistics: hand the same ones to blend_box
        stats = None if reg is None else [R.tile_stats(p) for p in tiles]
        acc, wsum = R.blend_box(tiles, dst, n_plane, n_plane, w, (0, 0, n_plane, n_plane), z, z, stats, reg)
        ref = R.blend(tiles, dst, n_plane, w, regularise_std=reg)
        with np.errstate(invalid="ignore"):
            got = acc / wsum
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and not np.isnan(ref).all()
        ok = ~np.isnan(ref)
        assert np.array_equal(got[ok].view(np.uint64), ref[ok].view(np.uint64))


def test_blend_box_clips_to_the_box_and_keeps_the_rest():
    rng = np.random.Generator(np.random.PCG64(7))
    rows, cols, tile = 23, 40, 5
    tiles = PC.wide_tiles((4, tile, tile), 8)
    dst = [(-2, -3), (20, 37), (9, 9), (9, 11)]
    w = rng.random((tile, tile)) + 0.1
    acc0, wsum0 = rng.standard_normal((rows, cols)), rng.random((rows, cols))
    box = (0, 1, 11, 40)
    acc, wsum = R.blend_box(tiles, dst, rows, cols, w, box, acc0, wsum0)
    ref_a, ref_w = acc0.copy(), wsum0.copy()
    for x in range(box[0], box[2]):                                 # the kernel's loop, pixel by pixel
        for y in range(box[1], box[3]):
            for p, (dx, dy) in zip(tiles, dst):
                lx, ly = x - dx, y - dy
                if 0 <= lx < tile and 0 <= ly < tile:
                    ref_a[x, y] += w[lx, ly] * np.float64(p[lx, ly])
                    ref_w[x, y] += w[lx, ly]
    assert np.array_equal(acc, ref_a) and np.array_equal(wsum, ref_w)
    outside = np.ones((rows, cols), bool)
    outside[box[0]:box[2], box[1]:box[3]] = False
    assert np.array_equal(acc[outside], acc0[outside])
    assert (acc != acc0).sum() == 3 * 1 + 2 * 7         # tile 0: rows 0-2 of column 1; tiles 2, 3: rows 9, 10 of 9-15


def test_cut_ref_wraps_any_int32_origin():
    plane = np.arange(5 * 7, dtype=np.float64).reshape(5, 7)
    for x0, y0 in [(0, 0), (-37, 250), (-8, 22), (2 ** 31 - 1, -2 ** 31)]:
        got = R.cut_ref(plane, x0, y0, 9)
        for r in range(9):
            for c in range(9):
                assert got[r, c] == plane[(x0 + r) % 5, (y0 + c) % 7]


@pytest.mark.parametrize("name", sorted(PC.regularise_cases()))
def test_regularise_inputs_stay_out_of_the_tie_band(name):
    tiles, reg = PC.regularise_cases()[name]
    assert tiles.shape[-1] ** 2 <= 289
    for t in range(tiles.shape[0]):
        for f in range(tiles.shape[1]):
            assert PC.mask_is_safe(tiles[t, f], reg), (name, t, f)


def test_regularise_special_cases_are_what_they_claim():
    cases = PC.regularise_cases()

    def masked(p, reg):
        m, s = R.device_tile_stats(p)
        with np.errstate(invalid="ignore"):
            return np.abs(p.astype(np.float64) - m) > s * reg
    t, reg = cases["constant"]
    assert not masked(t[1, 0], reg).any() and masked(t[0, 0], reg).any()
    t, reg = cases["zero_threshold"]
    for k in range(4):
        keep = ~masked(t[k, 0], reg)
        assert 2 <= keep.sum() < 64 and np.array_equal(keep, t[k, 0] == t[k, 0].astype(np.float64).mean())
    for name in ("nan", "inf"):
        t, reg = cases[name]
        k = int(np.flatnonzero(~np.isfinite(t).reshape(len(t), -1).all(axis=1))[0])
        assert not masked(t[k, 0], reg).any() and masked(t[(k + 1) % 4, 0], reg).any()
    # a pixel on the threshold is refused by the condition
    p = np.zeros((16, 16), np.float32)
    p[0, 0], p[0, 1] = 1.0, -1.0
    m, s = R.device_tile_stats(p)
    assert not PC.mask_is_safe(p, float((1.0 - m) / s))
