"""Host side of the CGAN's device batch assembly (bp_gather_tiles_gan, DeviceTileAssembler.gather_gan,
CGANPainter.use_device_assembly): the entry point's declarations, the refusal of a training set without slab stacks before
anything is uploaded, and the memoised permutation table."""
import os
import re

import numpy as np
import pytest

from baryon_painter_amd import _lib as L
from baryon_painter_amd.utils.datasets import BAHAMASDataset, DeviceTileAssembler, SyntheticTileDataset

HERE = os.path.dirname(os.path.abspath(__file__))


def test_new_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(HERE), "include", "bp_hip.h")).read()
    declared = set(re.findall(r"\b(bp_[a-z0-9_]+)\s*\(", header))
    lib = L.load()
    name = "bp_gather_tiles_gan"
    assert name in declared, f"{name} is not declared in bp_hip.h"
    assert name in L.SIGNATURES, f"{name} has no ctypes signature"
    assert hasattr(lib, name), f"{name} is not exported"
    args = re.search(rf"^int {name}\(([^;]*)\);", header, re.M).group(1)
    assert len(args.split(",")) == len(L.SIGNATURES[name][1]) == 16
    # the refusals that need no device: every argument is checked before a launch
    assert lib.bp_gather_tiles_gan(*([None] * 9), 1, 16, None, None, None, None, None) == L.BP_EINVAL


def test_a_training_set_without_stacks_is_refused_before_an_upload(monkeypatch):
    import torch
    from baryon_painter_amd.painter import CGANPainter

    def no_upload(*a, **k):
        raise AssertionError("something was uploaded before the training set was refused")
    monkeypatch.setattr(torch.Tensor, "to", no_upload)
    p = CGANPainter.__new__(CGANPainter)
    p.training_data, p.compute_device = SyntheticTileDataset(n_sample=4, tile_size=16), "cuda:0"
    with pytest.raises(NotImplementedError):
        p.use_device_assembly()
    assert getattr(p, "device_assembler", None) is None


def test_memoised_perm_affine_equals_the_computation():
    rng = np.random.default_rng(3)
    data = {f: {0.0: {"100": rng.random((1, 64, 64), dtype=np.float32), "150": rng.random((1, 64, 64), dtype=np.float32),
                      "mean_100": 0.5, "mean_150": 0.5, "var_100": 1 / 12, "var_150": 1 / 12}}
            for f in ("dm", "pressure")}
    ds = BAHAMASDataset(data=data, redshifts=[0.0], label_fields=["pressure"], n_tile=4, tile_permutations=True,
                        fixed_indexing=True)
    assert ds.tile_size == 16
    asm = DeviceTileAssembler.__new__(DeviceTileAssembler)
    asm.ds = ds
    calls = []
    apply = ds.apply_tile_permutation
    ds.apply_tile_permutation = lambda tile, p: (calls.append(p), apply(tile, p))[1]
    fresh = [asm._perm_affine_compute(p) for p in range(8)]
    assert len(set(fresh)) == 8                                   # fixed_indexing: eight different maps
    n_fresh = len(calls)
    for _ in range(3):
        assert [asm._perm_affine(p) for p in range(8)] == fresh
    assert len(calls) == 2 * n_fresh                              # the grids were built once more per code, then never
    # the table is that of the data: a tile permuted by the affine map is apply_tile_permutation's
    tile = rng.random((16, 16))
    r, c = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    for p, (r0, rr, rc, c0, cr, cc) in enumerate(fresh):
        assert np.array_equal(tile[r0 + rr * r + rc * c, c0 + cr * r + cc * c], apply(tile, p))
