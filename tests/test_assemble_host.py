"""Host side of the device batch assembly for multi-scale / minimum-subtracted training sets: the host dataset against
the reference fixture (tests/golden/assemble.npz), which chains the assembler accepts, and the new entry points'
declarations."""
import os
import re

import numpy as np
import pytest

import assemble_cases as AC
import host_cases as HC
from baryon_painter_amd import _lib as L
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils.datasets import BAHAMASDataset, DeviceTileAssembler

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_ENTRY_POINTS = ("bp_tile_minima", "bp_gather_tiles_scales_workspace", "bp_gather_tiles_scales")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "assemble.npz"))


def dataset(sub, transform=None, inverse=None):
    tr, itr = AC.chain(T)
    return BAHAMASDataset(data=HC.data_dict("random"), transform=transform or tr, inverse_transform=inverse or itr,
                          subtract_minimum=sub, **AC.DATASET)


@pytest.mark.parametrize("tag,sub", [("plain", False), ("submin", True)])
def test_host_dataset_reproduces_the_reference_fixture(tag, sub, gold):
    """The same NumPy / SciPy expressions in float64 on the same stacks: equal up to the last bits of float64."""
    ds = dataset(sub)
    idx = gold[f"{tag}/idx"]
    assert len(ds) == int(gold[f"{tag}/len"]) and np.array_equal(idx, AC.indices(len(ds))) and len(idx) == 64
    perms = np.array([ds.sample_idx_to_tile_permutation(int(i)) for i in idx])
    assert set(perms[:, 0]) == set(perms[:, 1]) == set(range(8))          # every permutation code, both slabs
    got = AC.record(ds, idx)
    for k in ("z", "sum", "pixel", "full"):
        ref = gold[f"{tag}/{k}"]
        assert got[k].shape == ref.shape
        assert (np.abs(got[k] - ref) <= 1e-13 * np.abs(ref).max()).all(), k
    if sub:                                                # the minimum really is subtracted: the input's original ...
        assert (got["full"][:, 0, 0].min(axis=(1, 2)) == 0).all()            # ... channel touches log(0 + 1) = 0
        assert (got["full"][:, 1, 0].min(axis=(1, 2)) > 0).all()             # the label field is left alone


def _steps(order):
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    split, unsplit = T.create_split_scale_transform(2, 4, False)
    log_fwd, _ = T.create_range_compress_transforms(HC.K_VALUES, {"dm": "log", "pressure": "log"})
    return {
        "single": [fwd, T.atleast_3d, T.as_float32],
        "single, shape first": [T.as_float32, fwd, T.atleast_3d],
        "bare": fwd,
        "scales": [fwd, split, T.atleast_3d],
        "scales, float32": [fwd, T.as_float32, split, T.atleast_3d, T.as_float32],
        "split first": [T.as_float32, split, fwd],
        "shape in front": [T.atleast_3d, fwd, split],
        "two shape steps inside": [fwd, T.as_float32, T.as_float32, split],
        "split twice": [fwd, split, split],
        "inverse split": [fwd, unsplit],
        "other mode": [log_fwd, split, T.atleast_3d],
        "other mode, single": [log_fwd, T.atleast_3d],
        "two range compressions": [fwd, fwd, T.atleast_3d],
        "custom step": [fwd, lambda x, field, z, stats: 2 * x, T.atleast_3d],
        "no range compression": [T.atleast_3d, T.as_float32],
    }[order]


def _chain(order):
    st = _steps(order)
    return T.chain_transformations(st) if isinstance(st, list) else st


@pytest.mark.parametrize("order,levels", [("single", 1), ("single, shape first", 1), ("bare", 1), ("scales", 2),
                                          ("scales, float32", 2)])
def test_chains_with_a_device_form(order, levels):
    ds = dataset(False, transform=_chain(order))
    mode, k, scales = DeviceTileAssembler._read_chain(ds, T)
    assert mode == "shift-log" and k == {"dm": 4.0, "pressure": 4.0}
    if levels == 1:
        assert scales is None
    else:
        assert scales == {"n_scale": 2, "step_size": 4, "include_original": False, "truncate": 3.0}


def test_identity_chain_is_the_untransformed_batch():
    ds = BAHAMASDataset(data=HC.data_dict("random"), **AC.DATASET)
    assert DeviceTileAssembler._read_chain(ds, T) == (None, {}, None)


@pytest.mark.parametrize("order", ["split first", "shape in front", "two shape steps inside", "split twice",
                                   "inverse split", "other mode", "other mode, single", "two range compressions",
                                   "custom step", "no range compression"])
def test_other_chains_are_refused_in_the_constructor(order, monkeypatch):
    """NotImplementedError before any stack is uploaded: nothing may touch the device on the way."""
    import torch
    ds = dataset(False, transform=_chain(order))

    def no_upload(*a, **k):
        raise AssertionError("a stack was uploaded before the chain was refused")
    monkeypatch.setattr(torch.Tensor, "to", no_upload)
    with pytest.raises(NotImplementedError):
        DeviceTileAssembler(ds, "cuda:0")
    from baryon_painter_amd.painter import CVAEPainter
    p = CVAEPainter.__new__(CVAEPainter)
    p.training_data, p.compute_device = ds, "cuda:0"
    with pytest.raises(NotImplementedError):
        p.use_device_assembly()
    assert getattr(p, "device_assembler", None) is None


def test_painter_and_assembler_share_the_chain_reader():
    """The paint path reads the same chains through the same functions."""
    for order in ("scales", "scales, float32"):
        k, split = T.device_split_scale(_chain(order), 0, "dm")
        assert k == 4.0 and isinstance(split, T._SplitScale) and split.n_scale == 2
    with pytest.raises(NotImplementedError):
        T.device_split_scale(_chain("split first"), 0, "dm")
    assert T.device_shift_log(_chain("single"), 0, "pressure") == 4.0
    radii, weights = T.split_scale_tables(3, 4, 3.0)
    assert radii == [0, 6, 24] and weights.dtype == np.float64 and len(weights) == 13 + 49
    assert np.array_equal(weights[:13], T.gaussian_weights(2.0)) and np.array_equal(weights[13:], T.gaussian_weights(8.0))


def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(HERE), "include", "bp_hip.h")).read()
    declared = set(re.findall(r"\b(bp_[a-z0-9_]+)\s*\(", header))
    lib = L.load()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, f"{name} is not declared in bp_hip.h"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} is not exported"
    # argument counts of the declarations and of the ctypes table agree
    for name in NEW_ENTRY_POINTS:
        args = re.search(rf"^(?:int|size_t) {name}\(([^;]*)\);", header, re.M).group(1)
        assert len(args.split(",")) == len(L.SIGNATURES[name][1]), name
    # the workspace query and the error order, without a launch
    assert lib.bp_gather_tiles_scales_workspace(4, 16, 1) == 0
    assert lib.bp_gather_tiles_scales_workspace(4, 16, 3) == lib.bp_split_scale_workspace(4, 16, 16) == 3 * 4 * 256 * 4
