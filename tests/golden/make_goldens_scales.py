#!/usr/bin/env python3
"""Generate tests/golden/scales.npz by IMPORTING THE REAL REFERENCE (build container only):

    python tests/golden/make_goldens_scales.py

``create_split_scale_transform`` of the reference (utils/data_transforms.py:14-42, SciPy's gaussian_filter on float32
tiles) on the tiles of tests/scales_ref.py: 16^2, 24x40 and 64^2, for (n_scale, step_size, include_original) in
scales_ref.PARAMS.  Inputs and outputs are stored; data only.

Harness shim: an empty stub for the absent ``cosmotools`` package the reference's module imports at its top (its
``rebin_2d`` is only named in a comment)."""
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
import scales_ref as R                                               # noqa: E402


def main():
    out = {}
    for si, shape in enumerate(R.SHAPES):
        x = R.tile(shape, 100 + si)
        out[f"x_{shape[0]}x{shape[1]}"] = x
        for params in R.PARAMS:
            fwd, inv = ref_T.create_split_scale_transform(*params)
            t = fwd(x.copy(), "dm", 0.0, None)
            assert t.dtype == np.float32 and t.shape == (params[0] + int(params[2]), *shape)
            out[R.key(shape, params)] = t
            out["inv_" + R.key(shape, params)] = np.asarray(inv(t, "dm", 0.0, None))
    path = os.path.join(HERE, "scales.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
