"""CPU: painters with several label fields -- the architecture's sizes, the device-transform parameters per field, the
host plane blend per field, the per-field slicing against the reference fixture (tests/golden/multi_field.npz), the
light cone's ``field=`` argument, and the declarations of the two entry points the device paths add."""
import os
import re

import numpy as np
import pytest
import torch

import host_cases as HC
import multi_field_cases as MF
from baryon_painter_amd import _lib as L
from baryon_painter_amd import lightcone as LC
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.painter import CVAEPainter
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils.datasets import compile_transform

HERE = os.path.dirname(os.path.abspath(__file__))
ZS = np.array([0.3, -0.2, 2.5, 0.5])


@pytest.mark.parametrize("s", [1, 3])
def test_fiducial_architecture_sizes_follow_the_reference_script(s):
    """scripts/CVAE_single_scale.py:92-133: n_x_feature = len(label_fields) * n_scale, dim_y = (n_scale, ...)."""
    arch = A.fiducial_architecture(64, n_fields=2, n_scale=s, predict_var=True)
    assert arch["dim_x"] == (2 * s, 64, 64) and arch["dim_y"] == (s, 64, 64) and arch["n_x_features"] == 2 * s
    assert arch["q_x_in"][0][1]["in_channels"] == 2 * s
    assert arch["q_y_in"][0][1]["in_channels"] == s + 1 and arch["prior_z_y"][0][1]["in_channels"] == s + 1
    assert arch["p_y_z_in"][0][1]["in_channels"] == s + 2
    for head in arch["p_y_z_out"]:
        convs = [cfg for name, cfg in (l for l in head if len(l) == 2) if name == "conv"]
        assert [(c["in_channels"], c["out_channels"]) for c in convs] == [(16, 8), (8, 2 * s), (2 * s, 2 * s)]
    one = A.fiducial_architecture(64, n_scale=s)
    assert one == A.fiducial_architecture(64, n_scale=s, n_fields=1) and one["dim_x"] == (s, 64, 64)


def _painter(labels, modes=MF.MODES, k_values=MF.K_VALUES, scales=None):
    """A painter as ``load_state_from_file`` leaves it, without a model: what ``_transform_parameters`` reads."""
    p = CVAEPainter.__new__(CVAEPainter)
    fwd, inv = MF.chains(T, modes, k_values, scales)
    p.transform, p.inverse_transform = compile_transform(fwd, MF.stats()), compile_transform(inv, MF.stats())
    p.input_field, p.label_fields = MF.INPUT, list(labels)
    return p


@pytest.mark.parametrize("scales", [None, (2, 4, False)])
def test_transform_parameters_hold_every_fields_records_and_modes(scales):
    st = MF.stats()
    params, sc, modes = _painter(MF.LABELS, scales=scales)._transform_parameters(ZS)
    assert (sc is None) if scales is None else (sc["n_scale"], sc["include_original"]) == (2, False)
    fwd, inv = T.create_range_compress_transforms(MF.K_VALUES, MF.MODES, eps=MF.EPS, sqrt_of_mean=True)
    want_in = T.DeviceRangeCompress(fwd, "dm")
    want_out = [T.DeviceRangeCompress(inv, f) for f in MF.LABELS]
    assert params["xf_out"].shape == (4, 2, 4) and params["xf_out"].dtype == np.float64
    for j, f in enumerate(MF.LABELS):
        assert np.array_equal(params["xf_out"][:, j], want_out[j].records(st[f], ZS))
    assert np.array_equal(params["xf_in"], want_in.records(st["dm"], ZS)) and params["xf_in"].shape == (4, 4)
    assert modes == (T.MODE_IDS["log"], (T.MODE_IDS["shift-log-2p"], T.MODE_IDS["log"]))
    assert np.array_equal(params["aux"], ZS)
    # the four-double form on both sides even when every field is shift-log
    params, _, modes = _painter(MF.LABELS, *MF.ALL_SHIFT_LOG)._transform_parameters(ZS)
    assert modes == (0, (0, 0)) and params["xf_in"].shape == (4, 4) and params["xf_out"].shape == (4, 2, 4)
    assert np.array_equal(params["xf_out"][:, 1, 0], np.sqrt(T.interpolate_z_many(st["gas"], ZS, "var")))
    assert (params["xf_out"][:, 0, 1] == 4.0).all() and (params["xf_out"][:, 1, 1] == 3.0).all()


def test_transform_parameters_of_one_label_field_are_what_they_were():
    st = MF.stats()
    # both shift-log: rows {sigma, k} / {k, sigma}, no modes
    params, sc, modes = _painter(["pressure"], *MF.ALL_SHIFT_LOG)._transform_parameters(ZS)
    s_in = np.sqrt(T.interpolate_z_many(st["dm"], ZS, "var"))
    s_out = np.sqrt(T.interpolate_z_many(st["pressure"], ZS, "var"))
    assert modes is None and sc is None
    assert np.array_equal(params["xf_in"], np.stack([s_in, np.full(4, 4.0)], axis=1))
    assert np.array_equal(params["xf_out"], np.stack([np.full(4, 4.0), s_out], axis=1))
    # another pair: the (n, 4) records and the two mode numbers
    params, sc, modes = _painter(["gas"])._transform_parameters(ZS)
    fwd, inv = T.create_range_compress_transforms(MF.K_VALUES, MF.MODES, eps=MF.EPS, sqrt_of_mean=True)
    assert modes == (T.MODE_IDS["log"], T.MODE_IDS["log"]) and all(type(m) is int for m in modes)
    assert np.array_equal(params["xf_in"], T.DeviceRangeCompress(fwd, "dm").records(st["dm"], ZS))
    assert np.array_equal(params["xf_out"], T.DeviceRangeCompress(inv, "gas").records(st["gas"], ZS))
    assert params["xf_out"].shape == (4, 4)


class _StubPainter:
    """``paint_batch`` returns seeded tiles of ``fields`` fields (no ``paint_stream``: the host path's fall-back)."""

    def __init__(self, fields, pick=None):
        self.fields, self.pick = fields, pick
        self.label_fields = ["pressure", "gas"][:fields]

    def paint_batch(self, inputs, z, batch_size=64):
        n, h, w = inputs.shape
        rng = np.random.Generator(np.random.PCG64(31))
        out = np.exp(rng.standard_normal((n, 2, h, w))).astype(np.float32)
        out[:, 1] *= np.float32(7.0)
        return out if self.pick is None else out[:, self.pick]


@pytest.mark.parametrize("regularise_std", [None, 1.5])
def test_host_plane_of_two_fields_equals_two_single_field_blends(regularise_std):
    delta = HC.plane(40)
    kw = dict(tile_relative_size=0.4, n_pixel_tile=16, z=0.3, regularise_std=regularise_std)
    both = LC.paint_plane(_StubPainter(2), delta, **kw)
    assert both.shape == (2, 40, 40) and both.dtype == np.float64
    for f in range(2):
        single = LC.paint_plane(_StubPainter(1, pick=f), delta, **kw)
        assert single.shape == (40, 40) and np.array_equal(both[f], single, equal_nan=True)
    assert not np.array_equal(both[0], both[1], equal_nan=True)
    if regularise_std is not None:                               # the masks are the fields' own: they differ
        plain = LC.paint_plane(_StubPainter(2), delta, **dict(kw, regularise_std=None))
        assert (plain != both).any()


def test_per_field_slicing_reproduces_the_reference_fixture():
    """The reference's head through this repository's host inverses, field by field: the same NumPy expressions on the
    same inputs, so the same bits (the limit of tests/test_range_modes_host.py against its fixture) -- through
    ``CVAEPainter._inverse_fields``, the slicing ``paint`` / ``paint_batch`` use."""
    gold = np.load(os.path.join(HERE, "golden", "multi_field.npz"))
    head, want = gold["head"], gold["physical"]
    assert head.shape == (MF.BATCH, 2, MF.SIZE, MF.SIZE) and want.shape == head.shape and want.dtype == np.float64
    p = _painter(MF.LABELS)
    _, inv = T.create_range_compress_transforms(MF.K_VALUES, MF.MODES, eps=MF.EPS, sqrt_of_mean=True)
    for n in range(MF.BATCH):
        z = float(MF.FIXTURE_Z[n])
        got = p._inverse_fields(head[n], z)
        assert got.shape == (2, MF.SIZE, MF.SIZE) and got.dtype == np.float64
        assert np.array_equal(got, want[n])
        assert np.array_equal(MF.inverse_fields(inv, head[n], z, MF.stats()), want[n])
    assert not np.array_equal(want[:, 0], want[:, 1])


def test_light_cone_needs_a_field_before_any_random_number_is_drawn():
    planes = [HC.plane(40)]
    args = dict(z=[0.3], delta_size=[100.0], tile_size=40.0, n_pixel_tile=16, resolution=24, scales=[1.0])
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="field"):
        LC.paint_light_cone(_StubPainter(2), planes, **args)
    with pytest.raises(ValueError, match="field"):
        LC.paint_light_cone(_StubPainter(2), planes, field="dm", **args)
    with pytest.raises(ValueError, match="field"):
        LC.paint_light_cone(_StubPainter(1), planes, field="gas", **args)
    with pytest.raises(ValueError, match="field"):
        LC.paint_small_plane(_StubPainter(2), HC.plane(40), (0.1, 0.2), 30.0, 40.0, 100.0, 16, 0.05)
    assert torch.equal(torch.get_rng_state(), state)
    # with the name: that field's plane is the one projected and kept
    y_map, kept = LC.paint_light_cone(_StubPainter(2), planes, field="gas", return_planes=True, **args)
    want = LC.paint_plane(_StubPainter(1, pick=1), planes[0], 0.4, 16, 0.3)
    assert np.array_equal(kept[0], want, equal_nan=True)
    ref_map, _ = LC.paint_light_cone(_StubPainter(1, pick=1), planes, return_planes=True, **args)
    assert np.array_equal(y_map, ref_map)
    named, _ = LC.paint_light_cone(_StubPainter(1, pick=1), planes, field="pressure", return_planes=True, **args)
    assert np.array_equal(named, ref_map)                        # (a single-field painter's own field may be named)


def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(HERE), "include", "bp_hip.h")).read()
    declared = set(re.findall(r"\b(bp_[a-z0-9_]+)\s*\(", header))
    lib = L.load()
    for name in ("bp_paint_store_fields", "bp_plane_blend_fields"):
        assert name in declared, f"{name} is not declared in bp_hip.h"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} is not exported"
        args = re.search(rf"^int {name}\(([^;]*)\);", header, re.M).group(1)
        assert len(args.split(",")) == len(L.SIGNATURES[name][1]), name
