"""Cases shared by tests/golden/make_goldens_multi_field.py (which feeds them to the reference) and the tests of
painters with several label fields (which feed them to this repository's code): a three-field ``data_dict`` beside
tests/host_cases.py's, the transforms of a (dm -> pressure, gas) painter whose two label fields use two different
range-compression modes, and the inputs of the reference fixture tests/golden/multi_field.npz."""
import collections

import numpy as np

import host_cases as HC

INPUT, LABELS = "dm", ("pressure", "gas")
# label modes: both with a positive image of the softplus head's positive activations, neither of them shift-log
MODES = {"dm": "log", "pressure": "shift-log-2p", "gas": "log"}
K_VALUES = {"dm": 2.0, "pressure": (0.5, 3.0), "gas": 2.5}
ALL_SHIFT_LOG = ({"dm": "shift-log", "pressure": "shift-log", "gas": "shift-log"}, {"dm": 4.0, "pressure": 4, "gas": 3.0})
EPS = 1e-3
SIZE, BATCH = 64, 2
SEED_W, SEED_D, SEED_Z = 7, 4321, 103
FIXTURE_Z = (0.3, 2.5)                   # the redshifts of the fixture's two tiles: between two table entries, beyond the last


def gas_stack(zi, slab):
    """Seeded positive float32 stack (14, 64, 64) of the third field, as ``host_cases.random_stack``."""
    rng = np.random.Generator(np.random.PCG64([13, zi, int(slab)]))
    return (rng.random((HC.N_STACK_FILE, HC.N_GRID, HC.N_GRID)) * 2.0 + 0.02).astype(np.float32)


def data_dict3():
    """``host_cases.data_dict("random")`` with a third field "gas" of its own stacks, means and variances."""
    data = HC.data_dict("random")
    data["gas"] = {}
    for zi, z in enumerate(HC.REDSHIFTS):
        e = {"mean_100": 0.9 + 0.03 * zi, "mean_150": 1.1 + 0.01 * zi, "var_100": 0.21 / (1 + zi), "var_150": 0.3 / (2 + zi)}
        for slab in ("100", "150"):
            e[slab] = gas_stack(zi, slab)
        data["gas"][z] = e
    return data


def stats():
    """stats[field][z] of the fixture: field- and redshift-dependent means and variances (Python floats)."""
    out = collections.OrderedDict()
    for fi, f in enumerate((INPUT,) + LABELS):
        out[f] = collections.OrderedDict(
            (z, {"mean": 0.4 + 0.3 * fi + 0.11 * zi, "var": 0.07 * (1 + fi) / (1 + zi)}) for zi, z in enumerate(HC.REDSHIFTS))
    return out


def chains(T, modes=MODES, k_values=K_VALUES, scales=None):
    """(transform, inverse transform) chains of a painter of LABELS with this repository's ``data_transforms`` module
    ``T``; ``scales = (n_scale, step_size, include_original)``: the split-scale orders the device path takes."""
    fwd, inv = T.create_range_compress_transforms(k_values, modes, eps=EPS, sqrt_of_mean=True)
    if scales is None:
        return T.chain_transformations([fwd, T.atleast_3d, T.as_float32]), T.chain_transformations([T.squeeze, inv])
    split, merge = T.create_split_scale_transform(*scales)
    return (T.chain_transformations([fwd, T.as_float32, split, T.atleast_3d]),
            T.chain_transformations([merge, inv, T.squeeze]))


def architecture(A, n_scale=1):
    return A.fiducial_architecture(SIZE, n_fields=len(LABELS), n_scale=n_scale)


def fixture_inputs(arch, syn):
    """(y, aux, z) of the fixture: a transformed 2-tile batch at FIXTURE_Z and the latent that is handed to sample_P."""
    _, y, _ = syn.synthetic_batch(BATCH, SIZE, SIZE, seed=SEED_D)
    return y, np.asarray(FIXTURE_Z, np.float32), syn.synthetic_eps((BATCH, *arch["dim_z"]), seed=SEED_Z)


def inverse_fields(inverse, head, z, st):
    """The reference's slicing (validation_plotting.py:109-110) of one tile's head (F * nf, H, W) with ``inverse`` --
    a range-compression inverse ``f(x, field, z, stats)`` of either code base -- per label field."""
    nf = head.shape[0] // len(LABELS)
    return np.stack([np.asarray(inverse(head[j * nf:(j + 1) * nf][0], f, z, st)) for j, f in enumerate(LABELS)])
