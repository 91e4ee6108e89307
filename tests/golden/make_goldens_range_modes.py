#!/usr/bin/env python3
"""Generate tests/golden/range_modes.npz by IMPORTING THE REAL REFERENCE (build container only):

    python tests/golden/make_goldens_range_modes.py

``create_range_compress_transforms`` of the reference (utils/data_transforms.py:51-110), forward and inverse, for all
six modes on the 32x32 float32 tiles of tests/range_modes_ref.py (0, negative values and NaN among the forward inputs;
-1, a value below it and NaN among the inverse inputs), at the three redshifts of ``Z_CASES`` (between two table
entries, beyond each end), two ``k`` settings per mode and ``sqrt_of_mean`` both ways (``range_modes_ref.cases``: with
``sqrt_of_mean`` every redshift for "1/x", the one mode that reads the mean, and the first redshift for the others --
the file stays under the size limit for a committed file).  Outputs only; data only.

Harness shim: an empty stub for the absent ``cosmotools`` package the reference's module imports at its top."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")

for name in ("cosmotools", "cosmotools.utils"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["cosmotools.utils"].rebin_2d = None

from baryon_painter.utils import data_transforms as ref_T            # noqa: E402  (the reference)
import range_modes_ref as R                                          # noqa: E402


def main():
    out, stats, x = {}, R.stats(), R.raw_tile()
    with np.errstate(all="ignore"):
        for mode in R.MODES:
            for ki, k in enumerate(R.K_SETS[mode]):
                y = R.activation_tile(mode, k)
                for sq, zi in R.cases(mode):
                    fwd, inv = ref_T.create_range_compress_transforms({R.FIELD: k}, {R.FIELD: mode}, eps=R.EPS,
                                                                      sqrt_of_mean=sq)
                    out[R.key(mode, ki, sq, zi, "fwd")] = np.asarray(fwd(x, R.FIELD, R.Z_CASES[zi], stats))
                    out[R.key(mode, ki, sq, zi, "inv")] = np.asarray(inv(y, R.FIELD, R.Z_CASES[zi], stats))
    assert all(v.dtype == np.float64 and v.shape == (32, 32) for v in out.values())      # NumPy 2 promotion
    path = os.path.join(HERE, "range_modes.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
