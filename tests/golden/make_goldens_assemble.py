#!/usr/bin/env python3
"""Generate tests/golden/assemble.npz by IMPORTING THE REAL REFERENCE (build container only):

    python tests/golden/make_goldens_assemble.py

The reference's BAHAMASDataset (utils/datasets.py:15-508) on the synthetic stacks of tests/host_cases.py with the chain
[range_compress(shift-log), split_scale(n_scale=3), atleast_3d] (tests/assemble_cases.py), once with
``subtract_minimum=False`` and once with ``subtract_minimum=True``: for 64 indices the redshifts, the per-channel sums
and a few pixels per level of both fields of ``dataset[idx]``, and the whole output of four of them.  Data only.

Harness shims, as in make_goldens_host.py: empty stub modules for the absent packages the reference imports at module
level, and ``np.unravel_index`` given back the ``dims=`` keyword NumPy removed."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")

for name in ("cosmotools", "cosmotools.utils", "cosmotools.power_spectrum_tools", "cosmotools.plotting", "pyccl",
             "astropy", "astropy.io", "astropy.io.fits"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["cosmotools.utils"].rebin_2d = None
sys.modules["astropy.io"].fits = sys.modules["astropy.io.fits"]
_unravel = np.unravel_index
np.unravel_index = lambda indices, shape=None, order="C", dims=None: _unravel(indices, shape if dims is None else dims, order)

from baryon_painter.utils import datasets as ref_ds                  # noqa: E402  (the reference)
from baryon_painter.utils import data_transforms as ref_T            # noqa: E402
import assemble_cases as AC                                          # noqa: E402
import host_cases as HC                                              # noqa: E402


def main():
    out = {}
    tr, itr = AC.chain(ref_T)
    for tag, sub in (("plain", False), ("submin", True)):
        ds = ref_ds.BAHAMASDataset(data=HC.data_dict("random"), transform=tr, inverse_transform=itr,
                                   subtract_minimum=sub, **AC.DATASET)
        idx = AC.indices(len(ds))
        out[f"{tag}/idx"] = idx
        out[f"{tag}/len"] = np.array(len(ds))
        for k, v in AC.record(ds, idx).items():
            out[f"{tag}/{k}"] = v
        print(tag, "len", len(ds), "indices", len(idx))
    path = os.path.join(HERE, "assemble.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
