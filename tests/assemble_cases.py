"""Case definitions shared by tests/golden/make_goldens_assemble.py (which feeds them to the real reference in the build
container) and tests/test_assemble_host.py / tests/test_gpu_assemble.py: a multi-scale, optionally minimum-subtracted
training set on the synthetic stacks of tests/host_cases.py (tile 16, permutations on).  Inputs are regenerated from
seeds; tests/golden/assemble.npz holds only what the reference's ``dataset[idx]`` returned."""
import numpy as np

import host_cases as HC

N_SCALE, STEP = 3, 4                       # create_split_scale_transform's defaults: include_original=True, truncate=3
LEVELS = N_SCALE + 1
DATASET = dict(redshifts=list(HC.REDSHIFTS), label_fields=["pressure"], n_tile=HC.N_TILE, n_stack=2, stack_offset=1,
               tile_permutations=True, scale_to_SLICS=True)
PIXELS = ((0, 0), (0, -1), (-1, 0), (5, 3), (8, 8))     # recorded per level
N_FULL = 4                                               # indices whose whole output is recorded


def indices(n_total):
    """64 indices: the first 8 permutation pairs of every redshift block's start, and seeded ones over the whole set
    (every one of the 8 x 8 permutation code pairs is 1/64 of a redshift block)."""
    rng = np.random.Generator(np.random.PCG64(31))
    per = n_total // len(HC.REDSHIFTS)
    fixed = [0, 1, per - 1, per, 2 * per + 63, n_total - 1]
    block = per // 64                                    # samples per permutation pair
    fixed += [p * 8 * block + 3 for p in range(8)] + [p * block + 5 + per for p in range(8)]
    rnd = (rng.random(64) * n_total).astype(np.int64).tolist()
    out = []
    for i in fixed + rnd:
        if 0 <= i < n_total and i not in out:
            out.append(int(i))
    return np.array(out[:64], dtype=np.int64)


def chain(T):
    """[range_compress(shift-log), split_scale(n_scale=3), atleast_3d] from the transforms module ``T`` (the
    reference's or this project's)."""
    fwd, inv = T.create_range_compress_transforms(HC.K_VALUES, HC.MODES)
    split, unsplit = T.create_split_scale_transform(N_SCALE, STEP)
    return T.chain_transformations([fwd, split, T.atleast_3d]), T.chain_transformations([unsplit, inv])


def record(ds, idx):
    """What the fixture holds of ``ds[i]`` for i in idx: redshifts, per-channel float64 sums, PIXELS per level, and the
    whole output of the first N_FULL indices."""
    zs = np.zeros(len(idx))
    sums = np.zeros((len(idx), 2, LEVELS))
    pix = np.zeros((len(idx), 2, LEVELS, len(PIXELS)))
    full = np.zeros((N_FULL, 2, LEVELS, ds.tile_size, ds.tile_size))
    for n, i in enumerate(idx):
        sample, ri, z = ds[int(i)]
        assert ri == int(i) and len(sample) == 2
        zs[n] = z
        for k, s in enumerate(sample):
            s = np.asarray(s, np.float64)
            assert s.shape == (LEVELS, ds.tile_size, ds.tile_size), s.shape
            sums[n, k] = s.sum(axis=(1, 2))
            pix[n, k] = np.stack([s[:, r, c] for r, c in PIXELS], axis=1)
            if n < N_FULL:
                full[n, k] = s
    return {"z": zs, "sum": sums, "pixel": pix, "full": full}
