"""Host side of the split-scale (Gaussian pyramid) transform (utils/data_transforms.py: create_split_scale_transform,
the reference's data_transforms.py:14-42): the reference's recorded results (tests/golden/scales.npz, written by
tests/golden/make_goldens_scales.py from the reference itself) bit for bit, the known answers of the reference's own
tests/test_transforms.py, the inverse, pickling, the multi-scale architecture, and the yardstick of the GPU tests --
SciPy's float32 result against the float64 restatement tests/scales_ref.py within the limit those tests use."""
import os
import pickle

import numpy as np
import pytest

import scales_ref as R
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.utils import data_transforms as T

pytest.importorskip("scipy.ndimage")

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scales.npz"))
CASES = [(shape, params) for shape in R.SHAPES for params in R.PARAMS]


def _x(shape):
    return GOLDEN[f"x_{shape[0]}x{shape[1]}"]


def test_fixture_inputs_are_the_seeded_tiles():
    for si, shape in enumerate(R.SHAPES):
        assert np.array_equal(_x(shape), R.tile(shape, 100 + si))


@pytest.mark.parametrize("shape,params", CASES)
def test_forward_and_inverse_equal_the_reference_bit_for_bit(shape, params):
    fwd, inv = T.create_split_scale_transform(*params)
    x = _x(shape)
    keep = x.copy()
    t = fwd(x, "dm", 0.0, None)
    assert np.array_equal(x, keep), "the transform must not modify its input"
    ref = GOLDEN[R.key(shape, params)]
    assert t.dtype == ref.dtype == np.float32 and t.shape == ref.shape
    assert np.array_equal(t, ref)
    assert np.array_equal(inv(t, "dm", 0.0, None), GOLDEN["inv_" + R.key(shape, params)])


def test_known_answers_of_the_reference_tests():
    """/root/reference/tests/test_transforms.py, as it stands there: a 256^2 standard-normal (float64) map, n_scale=3,
    step_size=2, include_original=True: t[0] == m and t[1:].sum(0) ~ m under np.allclose."""
    m = np.random.Generator(np.random.PCG64(0)).standard_normal((256, 256))
    fwd, inv = T.create_split_scale_transform(n_scale=3, step_size=2, include_original=True)
    t = fwd(m, None, None, {})
    assert t.shape == (4, 256, 256) and t.dtype == np.float64
    assert np.array_equal(t[0], m) and np.allclose(m, t[0])
    assert np.allclose(m, t[1:].sum(axis=0))
    assert np.array_equal(inv(t, None, None, {}), m)
    fwd, inv = T.create_split_scale_transform(n_scale=3, step_size=2, include_original=False)
    t = fwd(m, None, None, {})
    assert t.shape == (3, 256, 256) and np.allclose(inv(t, None, None, {}), m)


@pytest.mark.parametrize("params", R.PARAMS)
def test_inverse_of_forward_and_its_error(params):
    n_scale, step, inc = params
    fwd, inv = T.create_split_scale_transform(*params)
    x = _x((24, 40))
    back = inv(fwd(x, "dm", 0.0, None), "dm", 0.0, None)
    if inc or n_scale == 1:
        assert np.array_equal(back, x)
    else:
        # the float32 sum ((s0 + s1) + s2) of values bounded by 2^(n_scale-1) max|x| (scales_ref.rounding_count)
        assert np.abs(back - x).max() <= n_scale * 2.0 ** (n_scale - 1) * 2.0 ** -24 * np.abs(x).max()
    with pytest.raises(RuntimeError, match="Invalid shape of input"):
        inv(np.zeros((n_scale + int(inc) + 1, 8, 8), np.float32), "dm", 0.0, None)
    with pytest.raises(RuntimeError):
        inv(np.zeros((n_scale + int(inc) - 1, 8, 8), np.float32), "dm", 0.0, None)


def test_callables_pickle():
    fwd, inv = T.create_split_scale_transform(n_scale=4, step_size=2, include_original=True)
    chain = T.chain_transformations([T.as_float32, fwd, T.atleast_3d])
    f2, i2, c2 = pickle.loads(pickle.dumps((fwd, inv, chain)))
    x = _x((16, 16))
    t = fwd(x, "dm", 0.0, None)
    assert np.array_equal(f2(x, "dm", 0.0, None), t)
    assert np.array_equal(c2(x, "dm", 0.0, None), t)
    assert np.array_equal(i2(t, "dm", 0.0, None), inv(t, "dm", 0.0, None))
    assert (f2.n_scale, f2.step_size, f2.include_original, f2.truncate, f2.levels) == (4, 2, True, 3.0, 5)


def test_weights_are_scipys():
    from scipy.ndimage import correlate1d, gaussian_filter1d
    for sigma in (0.5, 1.0, 2.0, 8.0, 32.0):
        w = T.gaussian_weights(sigma)
        r = T.gaussian_radius(sigma)
        assert len(w) == 2 * r + 1 and np.array_equal(w, R.weights(sigma)) and r == R.radius(sigma)
        a = np.random.Generator(np.random.PCG64(int(sigma * 10))).standard_normal(300)
        assert np.array_equal(gaussian_filter1d(a, sigma, truncate=3.0), correlate1d(a, w, mode="reflect"))


def test_default_architecture_is_unchanged(golden_model):
    assert repr(A.fiducial_architecture(512)) == str(golden_model["fiducial_arch_repr"])
    assert repr(A.fiducial_architecture(512, n_scale=1)) == repr(A.fiducial_architecture(512))


def test_multi_scale_architecture_channels():
    """scripts/CVAE_single_scale.py:92-95,104-133 with n_scale = 3 and one label field."""
    a = A.fiducial_architecture(64, n_scale=3)
    assert a["dim_y"] == (3, 64, 64) and a["dim_x"] == (3, 64, 64) and a["n_x_features"] == 3
    assert a["dim_z"] == (1, 2, 2)
    first = lambda layers: layers[0][1]["in_channels"]
    assert first(a["prior_z_y"]) == 4 and first(a["q_y_in"]) == 4 and first(a["q_x_in"]) == 3
    assert first(a["p_y_z_in"]) == 5                            # n_aux_label + n_scale + 1 (h_z)
    for head in a["p_y_z_out"]:
        convs = [cfg for kind, *cfg in head if kind == "conv"]
        assert [c[0]["out_channels"] for c in convs] == [8, 3, 3] and convs[2][0]["in_channels"] == 3
    two = A.fiducial_architecture(64, predict_var=True, n_scale=4)
    assert len(two["p_y_z_out"]) == 2 and two["dim_x"][0] == 4


@pytest.mark.parametrize("shape,params", CASES)
def test_scipy_float32_lies_within_the_gpu_limit_of_the_float64_restatement(shape, params):
    """The yardstick of tests/test_gpu_scales.py: |float32 pipeline - scales_ref| <= T * 2^-24 * max|x| with T counted
    in scales_ref.rounding_count.  SciPy's own float32 result must satisfy it."""
    x = _x(shape)
    got = GOLDEN[R.key(shape, params)].astype(np.float64)
    ref = R.split_scale(x, *params)
    limit = R.rounding_count(params[0]) * 2.0 ** -24 * np.abs(x).max()
    err = np.abs(got - ref).max()
    print(R.key(shape, params), "err", err, "limit", limit)
    assert err <= limit


def test_datasets_deliver_multi_scale_tiles():
    """BAHAMASDataset(..., n_feature_per_field=n_scale) with the split-scale transform in its chain: (levels, H, W)
    float32 tiles for every field, and the painter's statistics labels per feature."""
    import host_cases as HC
    from baryon_painter_amd.utils.datasets import BAHAMASDataset
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    split, unsplit = T.create_split_scale_transform(n_scale=3, step_size=4, include_original=False)
    tr = T.chain_transformations([fwd, T.as_float32, split, T.atleast_3d])
    itr = T.chain_transformations([unsplit, inv, T.squeeze])
    ds = BAHAMASDataset(data=HC.data_dict("random"), redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=1,
                        n_stack=3, transform=tr, inverse_transform=itr, n_feature_per_field=3, scale_to_SLICS=True)
    fields, idx, z = ds[1]
    assert [f.shape for f in fields] == [(3, ds.tile_size, ds.tile_size)] * 2
    assert all(f.dtype == np.float32 for f in fields)
    raw = ds.get_label_sample(1, transform=False)[0]
    back = ds.inverse_transform(fields[1], field="pressure", z=z)
    assert np.abs(back - raw).max() <= 1e-5 * np.abs(raw).max()
    batch, _, zs = ds.get_batch(size=2)
    assert batch.shape == (2, 2, 3, ds.tile_size, ds.tile_size)
