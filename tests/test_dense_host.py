"""CPU: the two dense-bottleneck cases of tests/golden/dense.npz (tests/golden/make_goldens_dense.py ran the reference on
them) against the float64 oracle; the parameter containers' names and counts; and the host side of the dense language:
``probe_output`` through flatten / linear / unflatten, ``dense_blocks`` and the refusals of ``check_dense_language``,
none of which needs a device.  The GPU tests (test_gpu_dense*.py) compare the HIP path with the same fixture."""
import copy
import os

import numpy as np
import pytest

from baryon_painter_amd.models.graph import build_holders, dense_blocks, latent_shape, probe_output, unflatten_shape
from golden import make_goldens_dense as DN
from oracle.cvae_oracle import CVAEOracle

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense.npz"))
NETS = (("q_x_in", "q_x_in"), ("q_y_in", "q_y_in"), ("q_x_y_out", "q_out"), ("p_y_in", "p_y_in"), ("p_z_in", "p_z_in"),
        ("p_y_z_in", "p_y_z_in"), ("prior_z_y", "prior_network"))


def crop_rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((a - ref) ** 2).sum() / (ref ** 2).sum()))


@pytest.mark.parametrize("tag", ["s", "v"])
def test_oracle_reproduces_the_reference(tag):
    """Limits of tests/test_cond_net_host.py: losses 2e-5, x_mu / samples 1e-4, gradient norms 5e-3 against the fp32
    reference; the dense layers' gradients, stored whole, to 5e-3 of their scale; the stored noise floors re-derived to
    within a factor of two."""
    arch = DN.architectures()[tag]
    ora = CVAEOracle(arch, dtype=np.float64)
    names = str(GOLD[f"{tag}/params"]).split(",")
    assert sorted(ora.param_shapes()) == sorted(names)
    assert sum(int(np.prod(s)) for s in ora.param_shapes().values()) == int(GOLD[f"{tag}/n_params"])
    P = DN.parameters(ora.param_shapes())
    ora.load_params(P)
    x, y, aux, eps, eps1 = DN.inputs(arch)
    ora.forward(x, y, aux, eps)
    g = ora.backward(seed=-1.0)
    ref = GOLD[f"{tag}/stats"]
    assert np.abs(np.array(ora.get_stats()) - ref).max() <= 2e-5 * np.abs(ref).max()
    assert tuple(GOLD[f"{tag}/x_mu_shape"]) == ora.x_mu.shape == (DN.BATCH, 1, DN.SIZE, DN.SIZE)
    assert crop_rel_l2(DN.crop(ora.x_mu), GOLD[f"{tag}/x_mu_crop"]) <= 1e-4
    assert abs(np.sqrt((ora.x_mu ** 2).sum()) - GOLD[f"{tag}/x_mu_l2"]) <= 1e-4 * GOLD[f"{tag}/x_mu_l2"]
    for k, ref in zip(names, GOLD[f"{tag}/grad_norm"]):
        assert abs(np.sqrt((g[k] ** 2).sum()) - ref) <= 5e-3 * ref, k
    dense = DN.dense_names(arch, names)
    assert len(dense) == {"s": 4, "v": 7}[tag]
    for k in dense:
        assert DN.rel_err(g[k], GOLD[f"{tag}/grad/{k}"]) <= 5e-3, k
    floor = DN.noise_floors(arch, P, x, y, aux, eps, g)
    for k in names:
        stored = float(GOLD[f"{tag}/floor/{k}"])
        assert stored / 2 <= floor[k] <= stored * 2, (k, floor[k], stored)
    # the cases are well conditioned: the worst floors the fixture was chosen for (6.6e-4 ... 1e-3 in the residual
    # trunk of (s), 1.5e-4 in (v)), nowhere near the 6e-3 of batch 3
    assert max(floor.values()) <= 2e-3, max(floor.items(), key=lambda kv: kv[1])
    ora.training = False
    s = ora.sample_P(y, aux, eps=eps1)
    assert crop_rel_l2(DN.crop(s), GOLD[f"{tag}/sample_P_crop"]) <= 1e-4
    assert abs(np.sqrt((s ** 2).sum()) - GOLD[f"{tag}/sample_P_l2"]) <= 1e-4 * GOLD[f"{tag}/sample_P_l2"]


@pytest.mark.parametrize("tag", ["s", "v"])
def test_holders_carry_the_reference_names_and_counts(tag):
    arch = DN.architectures()[tag]
    keys, count = [], 0
    for key, attr in NETS[:6]:
        h = build_holders(arch[key])
        if h is not None:
            keys += [f"{attr}.{k}" for k in h.state_dict()]
            count += sum(p.numel() for p in h.parameters())
    h = build_holders(arch["p_y_z_out"][0])
    keys += [f"p_mu_out.{k}" for k in h.state_dict()]
    count += sum(p.numel() for p in h.parameters())
    h = build_holders(arch["prior_z_y"])
    keys += [f"prior_network.{k}" for k in h.state_dict()]
    count += sum(p.numel() for p in h.parameters())
    assert keys == str(GOLD[f"{tag}/state_keys"]).split(",")
    assert count == int(GOLD[f"{tag}/n_params"]) == {"s": 1661241, "v": 1672541}[tag]
    assert "q_out.1.weight" in keys and "q_out.1.bias" in keys
    if tag == "v":
        assert "q_out.3.weight" in keys and "q_out.3.bias" not in keys            # bias=False
        assert keys[keys.index("p_z_in.0.weight") + 1] == "p_z_in.0.bias"


def test_probe_output_reads_the_dense_language():
    A = DN.architectures()
    s, v = A["s"], A["v"]
    for a in (s, v):
        assert probe_output(a["q_x_in"], 1, 64, 64) == (32, 2, 2)
    assert probe_output(s["q_x_y_out"], 64, 2, 2) == (2, 2, 2)                    # unflatten (2, 1, 2, 2): 2 channels
    assert probe_output(s["prior_z_y"], 2, 64, 64) == (2, 2, 2)
    assert probe_output(s["p_z_in"], 1, 2, 2) == (1, 64, 64)
    assert probe_output(v["q_x_y_out"], 64, 2, 2) == (24, 1, 1)                   # unflatten (2, 12): flat, mu | log_var
    assert probe_output(v["prior_z_y"], 2, 64, 64) == (24, 1, 1)
    assert probe_output(v["p_z_in"], *latent_shape(v["dim_z"])) == (1, 64, 64)
    assert probe_output(v["p_z_in"][:2], 12, 1, 1) == (1, 2, 2)
    assert probe_output([("flatten",)], 3, 5, 5) == (75, 1, 1)
    assert latent_shape((12,)) == (12, 1, 1) and latent_shape((1, 2, 2)) == (1, 2, 2)
    assert unflatten_shape((2, 3, 2, 2)) == (6, 2, 2) and unflatten_shape((2, 12)) == (24, 1, 1)
    lin = lambda k, o: ("linear", {"in_features": k, "out_features": o})           # noqa: E731
    with pytest.raises(ValueError, match="in_features"):
        probe_output([("flatten",), lin(255, 8)], 64, 2, 2)
    with pytest.raises(ValueError, match="unflatten"):
        probe_output([("flatten",), lin(256, 8), ("unflatten", (2, 1, 2, 3))], 64, 2, 2)
    with pytest.raises(NotImplementedError, match="flat"):
        probe_output([lin(256, 8)], 64, 2, 2)
    with pytest.raises(ValueError):
        latent_shape((2, 2))


def test_dense_blocks_and_their_refusals():
    A = DN.architectures()
    b = dense_blocks(A["v"]["q_x_y_out"], "q_out.", "tail")
    assert b == {0: {"flatten": True, "linears": [(1, 2), (3, None)], "unflatten": (2, 12), "end": 5}}
    b = dense_blocks(A["v"]["p_z_in"], "p_z_in.", "head")
    assert list(b) == [0] and b[0]["linears"] == [(0, None)] and b[0]["end"] == 2 and not b[0]["flatten"]
    b = dense_blocks(A["s"]["prior_z_y"], "prior_network.", "tail")
    assert list(b) == [9] and b[9]["end"] == 12
    assert dense_blocks(A["s"]["p_y_z_in"], "p_y_z_in.", None) == {}
    lin = ("linear", {"in_features": 4, "out_features": 4})
    conv = ("conv", {"in_channels": 1, "out_channels": 1, "kernel_size": 3, "padding": 1})
    with pytest.raises(NotImplementedError, match=r"p_y_in\.1.*linear"):
        dense_blocks([("flatten",), lin], "p_y_in.", None)
    for act in ("tanh", "sigmoid", "softplus"):
        with pytest.raises(NotImplementedError, match=rf"q_out\.2.*{act}"):
            dense_blocks([("flatten",), lin, (act,)], "q_out.", "tail")
    with pytest.raises(NotImplementedError, match=r"q_out\.3.*batchnorm"):
        dense_blocks([("flatten",), lin, ("unflatten", (1, 2, 2)), ("batchnorm", {"num_features": 1})], "q_out.", "tail")
    with pytest.raises(NotImplementedError, match=r"q_out\.1.*in front of a convolution"):
        dense_blocks([("flatten",), lin, ("unflatten", (1, 2, 2)), conv], "q_out.", "tail")
    with pytest.raises(NotImplementedError, match=r"p_z_in\.2.*behind other layers"):
        dense_blocks([conv, ("flatten",), lin], "p_z_in.", "head")


def test_architectures_are_checked_on_the_host():
    """``check_dense_language`` is what ``CVAE.__init__`` runs before it touches the device."""
    from baryon_painter_amd.models import arch as our_arch
    from baryon_painter_amd.models.cvae import check_dense_language
    A = DN.architectures()
    for a in A.values():
        check_dense_language(a)
    check_dense_language(our_arch.fiducial_architecture(64))
    check_dense_language(our_arch.fiducial_architecture(64), sync=object())       # no dense block: nothing to refuse
    lin = ("linear", {"in_features": 4, "out_features": 4})
    for key in ("q_x_in", "q_y_in", "p_y_in", "p_y_z_in"):
        bad = copy.deepcopy(A["s"])
        bad[key] = list(bad[key] or []) + [("flatten",), lin]
        with pytest.raises(NotImplementedError, match=f"{key}.*linear"):
            check_dense_language(bad)
    bad = copy.deepcopy(A["s"])
    bad["p_y_z_out"] = (list(bad["p_y_z_out"][0]) + [("flatten",), lin],)
    with pytest.raises(NotImplementedError, match=r"p_y_z_out\[0\].*linear"):
        check_dense_language(bad)
    bad = copy.deepcopy(A["s"])
    bad["q_x_y_out"] = [bad["q_x_y_out"][1], bad["q_x_y_out"][2]]                   # linear on (64, 2, 2) without flatten
    with pytest.raises(NotImplementedError, match="flat"):
        check_dense_language(bad)
    bad = copy.deepcopy(A["v"])
    bad["q_x_y_out"] = bad["q_x_y_out"][:4] + [("tanh",), bad["q_x_y_out"][4]]
    with pytest.raises(NotImplementedError, match="tanh"):
        check_dense_language(bad)
    bad = copy.deepcopy(A["v"])
    bad["prior_z_y"] = bad["prior_z_y"] + [("batchnorm", {"num_features": 24})]
    with pytest.raises(NotImplementedError, match="batchnorm"):
        check_dense_language(bad)
    with pytest.raises(NotImplementedError, match="data parallel"):
        check_dense_language(A["v"], sync=object())
    bad = copy.deepcopy(A["v"])
    bad["p_z_in"] = bad["p_z_in"][2:]                                               # a convolution on a vector latent
    with pytest.raises(ValueError, match="p_z_in must begin with a linear"):
        check_dense_language(bad)
    bad = copy.deepcopy(A["s"])
    bad["q_x_y_out"][1] = ("linear", {"in_features": 255, "out_features": 8})
    with pytest.raises(ValueError, match="in_features"):
        check_dense_language(bad)
    bad = copy.deepcopy(A["v"])
    bad["dim_z"] = (10,)
    with pytest.raises(ValueError):
        check_dense_language(bad)
