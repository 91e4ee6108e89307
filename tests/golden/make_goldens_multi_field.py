#!/usr/bin/env python3
"""Generate tests/golden/multi_field.npz by IMPORTING THE REAL REFERENCE (build container only).

    python tests/golden/make_goldens_multi_field.py

The 64^2 architecture with ``n_x_features = 2`` (two label fields of one channel each, scripts/CVAE_single_scale.py:
92-133), seeded weights, ``sample_P(y, aux_label, z=given)`` of the reference for 2 tiles, and the reference's own
``create_range_compress_transforms`` inverses applied per field with the slicing of validation_plotting.py:109-110 --
field j from head channel j, the two fields in two different modes (tests/multi_field_cases.py).  Stored: the inputs,
the latent, the raw head and the per-field physical tiles (about 100 kB).  Nothing from the reference is copied, only
what it computes."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from baryon_painter_amd.models import arch as our_arch      # noqa: E402
from baryon_painter_amd.utils import synthetic as syn       # noqa: E402
import multi_field_cases as MF                              # noqa: E402


def main():
    from make_goldens import ref_cvae                                    # (imports the reference)
    from make_goldens_range_modes import ref_T
    torch.manual_seed(0)
    torch.set_num_threads(8)
    arch = MF.architecture(our_arch)
    assert arch["n_x_features"] == arch["dim_x"][0] == 2
    model = ref_cvae.CVAE(arch, "cpu")
    vals = syn.fill_params({k: tuple(v.shape) for k, v in model.named_parameters()}, MF.SEED_W)
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(torch.from_numpy(vals[k]))
    y, aux, z = MF.fixture_inputs(arch, syn)
    model.train(False)
    head = model.sample_P(torch.from_numpy(y), aux_label=torch.from_numpy(aux), z=z).numpy()
    assert head.shape == (MF.BATCH, 2, MF.SIZE, MF.SIZE) and head.dtype == np.float32
    _, inv = ref_T.create_range_compress_transforms(MF.K_VALUES, MF.MODES, eps=MF.EPS, sqrt_of_mean=True)
    st = MF.stats()
    phys = np.stack([MF.inverse_fields(inv, head[n], float(MF.FIXTURE_Z[n]), st) for n in range(MF.BATCH)])
    assert phys.shape == (MF.BATCH, 2, MF.SIZE, MF.SIZE) and phys.dtype == np.float64 and np.isfinite(phys).all()
    out = {"y": y, "aux": aux, "z": z, "head": head, "physical": phys,
           "params": np.array(",".join(k for k, _ in model.named_parameters()))}
    path = os.path.join(HERE, "multi_field.npz")
    np.savez_compressed(path, **out)
    print("multi_field.npz", os.path.getsize(path) // 1024, "KiB; head range", head.min(), head.max(),
          "physical range per field", phys.min(axis=(0, 2, 3)), phys.max(axis=(0, 2, 3)))


if __name__ == "__main__":
    main()
