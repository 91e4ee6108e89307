"""CPU: the three cases of tests/golden/unary.npz (tests/golden/make_goldens_unary.py ran the reference on them; the
cases themselves are tests/unary_cases.py) against the float64 oracle; the parameter containers' names; ``probe_output``
through tanh / sigmoid / softplus; and the host side of the unary language: which layers ``graph.unary_layers`` turns into
units and what ``check_unary_language`` still refuses, none of which needs a device.  The GPU tests (test_gpu_unary*.py)
compare the HIP path with the same fixture."""
import copy
import os

import numpy as np
import pytest

from baryon_painter_amd.models.graph import build_holders, dense_blocks, probe_output, unary_layers
from oracle.cvae_oracle import CVAEOracle

import unary_cases as UC

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unary.npz"))
TAGS = ["heads", "interior", "ytanh"]


def crop_rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((a - ref) ** 2).sum() / (ref ** 2).sum()))


def test_no_layer_of_the_fixture_is_saturated():
    for tag, arch in UC.architectures().items():
        layers = UC.unary_layers(arch)
        assert len(layers) == {"heads": 2, "interior": 11, "ytanh": 2}[tag]
        for name, kind in layers:
            assert float(GOLD[f"{tag}/unsat/{name}"]) >= 0.5, (tag, name, kind)


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_reproduces_the_reference(tag):
    """Limits of tests/test_dense_host.py: losses 2e-5, x_mu / samples / latent heads 1e-4, gradient norms 5e-3 against
    the fp32 reference; the gradients of the layers in front of a saturating layer, stored whole, to 5e-3 of their scale;
    the stored noise floors re-derived to within a factor of two."""
    arch = UC.architectures()[tag]
    ora = CVAEOracle(arch, dtype=np.float64)
    ora.alpha_var = UC.ALPHA_VAR[tag]
    names = str(GOLD[f"{tag}/params"]).split(",")
    assert sorted(ora.param_shapes()) == sorted(names)
    assert sum(int(np.prod(s)) for s in ora.param_shapes().values()) == int(GOLD[f"{tag}/n_params"])
    P = UC.parameters(ora.param_shapes())
    ora.load_params(P)
    x, y, aux, eps, eps1, zfix = UC.inputs(arch)
    ora.forward(x, y, aux, eps)
    g = ora.backward(seed=-1.0)
    ref = GOLD[f"{tag}/stats"]
    assert np.abs(np.array(ora.get_stats()) - ref).max() <= 2e-5 * np.abs(ref).max()
    L = arch.get("L", 1)
    assert tuple(GOLD[f"{tag}/x_mu_shape"]) == ora.x_mu.shape == (L * UC.BATCH, 1, UC.SIZE, UC.SIZE)
    assert crop_rel_l2(UC.crop(ora.x_mu), GOLD[f"{tag}/x_mu_crop"]) <= 1e-4
    assert abs(np.sqrt((ora.x_mu ** 2).sum()) - GOLD[f"{tag}/x_mu_l2"]) <= 1e-4 * GOLD[f"{tag}/x_mu_l2"]
    assert UC.rel_err(ora.z_mu, GOLD[f"{tag}/z_mu"]) <= 1e-4 and UC.rel_err(ora.z_log_var, GOLD[f"{tag}/z_log_var"]) <= 1e-4
    for k, ref in zip(names, GOLD[f"{tag}/grad_norm"]):
        assert abs(np.sqrt((g[k] ** 2).sum()) - ref) <= 5e-3 * ref, k
    front = UC.front_names(arch, names)
    assert len(front) == {"heads": 2, "interior": 29, "ytanh": 4}[tag], front
    stored = [k for k in front if f"{tag}/grad/{k}" in GOLD.files]
    assert stored
    for k in stored:
        assert UC.rel_err(g[k], GOLD[f"{tag}/grad/{k}"]) <= 5e-3, k
    floor = UC.noise_floors(arch, P, x, y, aux, eps, g, UC.ALPHA_VAR[tag])
    for k in names:
        stored = float(GOLD[f"{tag}/floor/{k}"])
        assert stored / 2 <= floor[k] <= stored * 2, (k, floor[k], stored)
    ora.training = False
    if L == 1:
        s = ora.sample_P(y, aux, eps=eps1)
        assert crop_rel_l2(UC.crop(s), GOLD[f"{tag}/sample_P_crop"]) <= 1e-4
        assert abs(np.sqrt((s ** 2).sum()) - GOLD[f"{tag}/sample_P_l2"]) <= 1e-4 * GOLD[f"{tag}/sample_P_l2"]
    s = ora.sample_P(y, aux, z=zfix)
    assert crop_rel_l2(UC.crop(s), GOLD[f"{tag}/sample_P_z_crop"]) <= 1e-4
    assert abs(np.sqrt((s ** 2).sum()) - GOLD[f"{tag}/sample_P_z_l2"]) <= 1e-4 * GOLD[f"{tag}/sample_P_z_l2"]
    if tag == "heads":
        assert np.abs(ora.x_mu).max() < 1.0                   # the tanh head
        assert (ora.log_x_var >= 0).all()                     # the softplus head


@pytest.mark.parametrize("tag", TAGS)
def test_holders_carry_the_reference_names(tag):
    arch = UC.architectures()[tag]
    keys, count = [], 0
    nets = [(k, a) for k, a in UC.NETS[:6]] + [(0, "p_mu_out"), (1, "p_var_out"), ("prior_z_y", "prior_network")]
    for key, attr in nets:
        if isinstance(key, int):
            seq = arch["p_y_z_out"][key] if len(arch["p_y_z_out"]) > key else None
        else:
            seq = arch.get(key)
        h = build_holders(seq)
        if h is not None:
            keys += [f"{attr}.{k}" for k in h.state_dict()]
            count += sum(p.numel() for p in h.parameters())
    assert keys == str(GOLD[f"{tag}/state_keys"]).split(",")
    assert count == int(GOLD[f"{tag}/n_params"])
    if tag == "interior":
        # the markers keep the indices: the layers behind a tanh / sigmoid / softplus are numbered as in the reference
        assert "p_y_z_in.14.res_block.0.weight" in keys and "q_x_in.3.weight" in keys and "p_z_in.6.weight" in keys


def test_probe_output_passes_the_activations_through():
    conv = ("conv", {"in_channels": 3, "out_channels": 5, "kernel_size": 4, "padding": 1, "stride": 2})
    for act in UC.UNARY:
        assert probe_output([(act,)], 3, 8, 6) == (3, 8, 6)
        assert probe_output([(act,), conv, (act,), (act,)], 3, 8, 6) == (5, 4, 3)
    A = UC.architectures()
    assert probe_output(A["interior"]["q_x_in"], 1, 64, 64) == (32, 2, 2)
    assert probe_output(A["interior"]["p_z_in"], 1, 2, 2) == (1, 64, 64)
    assert probe_output(A["interior"]["prior_z_y"], 2, 64, 64) == (2, 2, 2)
    assert probe_output(A["ytanh"]["p_y_in"], 2, 64, 64) == (4, 64, 64)
    assert probe_output(A["heads"]["p_y_z_out"][0], 16, 64, 64) == (1, 64, 64)


def test_which_layers_become_units():
    A = UC.architectures()
    it = A["interior"]
    assert unary_layers(it["q_x_in"], "q_x_in.", {}) == [2, 5, 8]
    assert unary_layers(it["p_y_z_in"], "p_y_z_in.", {}) == [2, 13]
    assert unary_layers(it["prior_z_y"], "prior_network.", dense_blocks(it["prior_z_y"], "prior_network.", "tail")) == [5]
    mu, var = A["heads"]["p_y_z_out"]
    assert unary_layers(mu, "p_mu_out.", {}, ("softplus",)) == [5] and unary_layers(var, "p_var_out.", {}) == [5]
    # the mean head's trailing softplus stays the fused flag; anywhere else in that head it is a unit
    mu = it["p_y_z_out"][0]
    assert mu[-1] == ("softplus",) and unary_layers(mu, "p_mu_out.", {}, ("softplus",)) == []
    assert unary_layers(mu, "p_mu_out.", {}) == [5]
    assert unary_layers(list(mu) + [("tanh",)], "p_mu_out.", {}, ("softplus",)) == [5, 6]
    assert unary_layers([("softplus",)] + list(mu), "p_mu_out.", {}, ("softplus",)) == [0]


def test_refusals_are_raised_on_the_host():
    """``check_unary_language`` is what ``CVAE.__init__`` runs, behind ``check_dense_language``, before it touches the
    device."""
    from baryon_painter_amd.models import arch as our_arch
    from baryon_painter_amd.models.cvae import check_dense_language, check_unary_language
    from golden import make_goldens_dense as DN
    A = UC.architectures()
    for a in A.values():
        check_dense_language(a)
        check_unary_language(a)
    check_unary_language(our_arch.fiducial_architecture(64))
    check_unary_language(our_arch.fiducial_architecture(64), "bf16")
    check_unary_language(A["heads"], "bf16")                 # the heads' last convolutions write fp32
    check_unary_language(A["ytanh"], "bf16")                 # p_y_in stays fp32
    # bf16: the generator trunk, and a head behind its first convolution (a bf16 slot); behind the second it is fp32
    with pytest.raises(NotImplementedError, match=r"p_y_z_in.*p_y_z_in\.2.*sigmoid.*bf16"):
        check_unary_language(A["interior"], "bf16")
    bad = copy.deepcopy(A["heads"])
    mu, var = bad["p_y_z_out"]
    bad["p_y_z_out"] = (mu[:2] + [("tanh",)] + mu[2:], var)
    check_unary_language(bad)
    with pytest.raises(NotImplementedError, match=r"p_y_z_out\[0\].*p_mu_out\.2.*tanh.*bf16"):
        check_unary_language(bad, "bf16")
    ok = copy.deepcopy(A["heads"])
    mu, var = ok["p_y_z_out"]
    assert mu[2][0].lower() == "conv" and mu[4][0].lower() == "conv"
    ok["p_y_z_out"] = (mu[:4] + [("sigmoid",)] + mu[4:], var)
    check_unary_language(ok, "bf16")
    # inside a residual block's branch
    bad = copy.deepcopy(A["heads"])
    i = [k for k, layer in enumerate(bad["p_y_z_in"]) if layer[0] == "residual block"][0]
    body, tail = bad["p_y_z_in"][i][1]
    bad["p_y_z_in"][i] = ("residual block", (body[:3] + [("sigmoid",)] + body[3:], tail))
    with pytest.raises(NotImplementedError, match=rf"p_y_z_in.*p_y_z_in\.{i}\.res_block\.3.*sigmoid.*residual"):
        check_unary_language(bad)
    # next to a dense block: behind it (graph.dense_blocks, pinned by tests/test_dense_host.py) and in front of it
    D = DN.architectures()
    for act in UC.UNARY:
        bad = copy.deepcopy(D["v"])
        bad["q_x_y_out"] = bad["q_x_y_out"] + [(act,)]
        with pytest.raises(NotImplementedError, match=rf"q_x_y_out.*q_out\.5.*{act}"):
            check_unary_language(bad)
        bad = copy.deepcopy(D["s"])
        bad["prior_z_y"] = bad["prior_z_y"][:9] + [(act,)] + bad["prior_z_y"][9:]
        with pytest.raises(NotImplementedError, match=rf"prior_z_y.*prior_network\.9.*{act}.*dense block"):
            check_unary_language(bad)
        bad = copy.deepcopy(D["v"])
        bad["p_z_in"] = bad["p_z_in"][:2] + [(act,)] + bad["p_z_in"][2:]
        with pytest.raises(NotImplementedError, match=rf"p_z_in.*p_z_in\.2.*{act}"):
            check_unary_language(bad)
    # ... while one convolution away from the block it is a unit like any other
    ok = copy.deepcopy(D["s"])
    ok["prior_z_y"] = ok["prior_z_y"][:6] + [("softplus",)] + ok["prior_z_y"][6:]
    check_dense_language(ok)
    check_unary_language(ok)
