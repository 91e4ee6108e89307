"""CPU: the three model-language cases of tests/golden/cond_net.npz (a p_y_in network, L = 2 behind it, no prior_z_y;
tests/golden/make_goldens_cond_net.py ran the reference on them) against the float64 oracle, the architecture helper that
builds them, and the parameter names of p_y_in.  The GPU tests (test_gpu_cond_net*.py) compare the HIP path with both."""
import os

import numpy as np
import pytest

from baryon_painter_amd.models import arch as A
from baryon_painter_amd.models.graph import build_holders
from baryon_painter_amd.utils import synthetic as syn
from golden import make_goldens_cond_net as CN
from golden_util import check
from oracle.cvae_oracle import CVAEOracle

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cond_net.npz"))


def crop_rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((a - ref) ** 2).sum() / (ref ** 2).sum()))


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_oracle_reproduces_the_reference(tag):
    """Tolerances: those tests/test_gpu_model.py states for the same quantities (losses 2e-5, x_mu / samples 1e-4,
    gradients 5e-3 against the fp32 reference, running statistics 2e-5)."""
    arch = CN.architectures()[tag]
    ora = CVAEOracle(arch, dtype=np.float64)
    assert ",".join(ora.param_shapes()) == str(GOLD[f"{tag}/params"])
    ora.load_params(CN.parameters(ora.param_shapes()))
    x, y, aux, eps, eps1 = CN.inputs(arch)
    ora.forward(x, y, aux, eps)
    g = ora.backward(seed=-1.0)
    ref = GOLD[f"{tag}/stats"]
    assert np.abs(np.array(ora.get_stats()) - ref).max() <= 2e-5 * np.abs(ref).max()
    assert tuple(GOLD[f"{tag}/x_mu_shape"]) == ora.x_mu.shape == (arch["L"] * CN.BATCH, 1, CN.SIZE, CN.SIZE)
    assert crop_rel_l2(CN.crop(ora.x_mu), GOLD[f"{tag}/x_mu_crop"]) <= 1e-4
    assert abs(np.sqrt((ora.x_mu ** 2).sum()) - GOLD[f"{tag}/x_mu_l2"]) <= 1e-4 * GOLD[f"{tag}/x_mu_l2"]
    names = str(GOLD[f"{tag}/params"]).split(",")
    assert sorted(g) == sorted(names)
    for k, ref in zip(names, GOLD[f"{tag}/grad_norm"]):
        assert abs(np.sqrt((g[k] ** 2).sum()) - ref) <= 5e-3 * ref, k
    for k in names:
        if k.startswith("p_y_in."):
            check(f"{tag}/grad/{k}", g[k], GOLD, 5e-3, what="grad ")
    for k in ora.buffer_shapes():
        if k.startswith("p_y_in."):
            check(f"{tag}/buf/{k}", ora.P[k], GOLD, 2e-5)
    assert (tag == "c") == (not any(k.startswith("p_y_in.") for k in names))
    # the cases are well conditioned: 2^-20 perturbations of the parameters move no true gradient by more than 1e-2 of
    # its scale (with ReLUs throughout, 6e-2 ... 1 at every data seed tried), p_y_in's by less than 1.25e-3
    rng = np.random.default_rng(7)
    pert = CVAEOracle(arch, dtype=np.float64)
    pert.load_params({k: np.asarray(v, np.float64) * (1.0 + 2.0 ** -20 * rng.uniform(-1, 1, np.shape(v)))
                      for k, v in CN.parameters(ora.param_shapes()).items()})
    pert.forward(x, y, aux, eps)
    gp = pert.backward(seed=-1.0)
    moved = {k: np.abs(gp[k] - g[k]).max() / np.abs(g[k]).max() for k in g}
    assert max(moved.values()) <= 1e-2, sorted(((v, k) for k, v in moved.items()), reverse=True)[:3]
    assert all(v <= 1.25e-3 for k, v in moved.items() if k.startswith("p_y_in.")), moved
    if arch["L"] == 1:
        ora.training = False
        s = ora.sample_P(y, aux, eps=eps1)
        assert crop_rel_l2(CN.crop(s), GOLD[f"{tag}/sample_P_crop"]) <= 1e-4
        assert abs(np.sqrt((s ** 2).sum()) - GOLD[f"{tag}/sample_P_l2"]) <= 1e-4 * GOLD[f"{tag}/sample_P_l2"]


def test_fiducial_architecture_takes_a_conditioning_stem_and_no_prior():
    base = A.fiducial_architecture(64)
    assert base["p_y_in"] is None and "prior_z_y" in base and base["p_y_z_in"][0][1]["in_channels"] == 3
    layers = CN.p_y_in_layers()
    got = A.fiducial_architecture(64, p_y_in=layers, prior=False)
    assert got["p_y_in"] is layers
    assert "prior_z_y" not in got
    assert got["p_y_z_in"][0][1]["in_channels"] == 4 + 1            # h_y's channels beside the one of h_z
    want = dict(base)
    del want["prior_z_y"]
    want["p_y_in"] = layers
    want["p_y_z_in"] = [("conv", dict(base["p_y_z_in"][0][1], in_channels=5))] + list(base["p_y_z_in"][1:])
    assert repr(got) == repr(want)
    assert list(got) == [k for k in base if k != "prior_z_y"]      # key order as before
    # the defaults, spelled out, are today's dict
    assert repr(A.fiducial_architecture(64, p_y_in=None, prior=True)) == repr(base)
    # a stem without a convolution leaves the generator's input as it is
    assert A.fiducial_architecture(64, p_y_in=[])["p_y_z_in"][0][1]["in_channels"] == 3


@pytest.mark.parametrize("tag", ["a", "b"])
def test_p_y_in_parameters_carry_the_reference_names(tag):
    """The containers that hold p_y_in's parameters name them as the reference's nn.Sequential does."""
    arch = CN.architectures()[tag]
    keys = str(GOLD[f"{tag}/state_keys"]).split(",")
    mine = ["p_y_in." + k for k in build_holders(arch["p_y_in"]).state_dict()]
    assert mine == [k for k in keys if k.startswith("p_y_in.")]
    assert mine[:3] == ["p_y_in.0.weight", "p_y_in.1.weight", "p_y_in.1.bias"]
    assert "prior_network.0.weight" in keys
    assert not any(k.startswith("prior_network.") for k in str(GOLD["c/state_keys"]).split(","))


def test_capture_guard_keeps_the_collector_off_and_restores_it():
    """``graph.capture_without_gc`` (around every stream capture): cyclic garbage is collected on entry, the collector is
    off inside -- a dropped model's graphs must not be destroyed from inside a capture -- and back as it was afterwards,
    also after an exception and also when it was off to begin with."""
    import gc
    import weakref
    from baryon_painter_amd.models.graph import capture_without_gc

    class Node:
        pass
    a, b = Node(), Node()
    a.other, b.other = b, a                    # a cycle, as a model and its plans form
    ref = weakref.ref(a)
    del a, b
    assert gc.isenabled()
    with capture_without_gc():
        assert ref() is None and not gc.isenabled()
    assert gc.isenabled()
    with pytest.raises(KeyError):
        with capture_without_gc():
            raise KeyError("x")
    assert gc.isenabled()
    gc.disable()
    try:
        with capture_without_gc():
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()
