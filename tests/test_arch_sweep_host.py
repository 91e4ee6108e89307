"""CPU: the case list of the layer-language sweep (tests/arch_sweep.py) checked on its own, before any GPU run.

  * every case evaluates in the float64 graph (oracle/torch_ref.py) with a finite ELBO, and the stock fp32 evaluation
    of the same graph lies within 2e-4 of it on every parameter gradient, under the scale floor of the GPU test's
    limits: the condition that makes those limits meaningful (an ill-conditioned case is changed in the list);
  * ``graph.probe_output`` agrees with the shapes torch produces for every net of every case;
  * the list's claims about itself: every (bias, batch-norm, activation) triple in front of every kind of next layer,
    every width / kernel / stride of the axes, the counts of the special cases."""
import numpy as np
import pytest
import torch

from baryon_painter_amd.models.graph import build_holders, probe_output
from oracle.torch_ref import TorchRefCVAE, _seq

import arch_sweep as AS

CASES = AS.cases()
TAGS = [c[0] for c in CASES]


def evaluate(arch, P, x, y, aux, eps, alpha_var, dtype=torch.float64, tap=None, bf16=False, act_tap=None):
    r = TorchRefCVAE(arch, P, dtype=dtype, tap=tap, bf16=bf16)
    r.alpha_var, r.act_tap = alpha_var, act_tap
    (-r.forward(x, y, aux, eps)).backward()
    return r


def grads(r):
    return {k: t.grad.detach().double().numpy() for k, t in r.P.items() if t.requires_grad}


def test_the_list_is_what_the_issue_asks_for():
    assert len(CASES) == 24 and len(set(TAGS)) == 24
    sizes = [a["dim_x"][1] for _, a, _, _ in CASES]
    assert sorted(set(sizes)) == [32, 64] and sizes.count(32) == 3
    assert all(n in (2, 3) for _, _, n, _ in CASES)
    assert len(AS.BF16) >= 6
    archs = [a for _, a, _, _ in CASES]
    two = [len(a["p_y_z_out"]) == 2 for a in archs]
    assert sum(two) >= 6 and {al for (_, _, _, al), t in zip(CASES, two) if t} == {0.3, 1.0}
    assert sum(a["dim_x"][0] // a["dim_y"][0] == 2 for a in archs) == 2          # n_fields 2
    assert sum(a["dim_y"][0] == 2 for a in archs) == 2                           # n_scale 2
    assert sum(a["L"] == 2 for a in archs) == 2
    assert sum(bool(a["p_y_in"]) for a in archs) == 3
    assert any(a["p_y_in"] and a["p_y_in"][-1][0].lower() == "batchnorm" for a in archs)     # ... one without activation
    assert sum("prior_z_y" not in a for a in archs) == 2
    assert {len(h) for a in archs for h in a["p_y_z_out"]} >= {2, 3}
    heads = [AS.blocks(h) for a in archs for h in a["p_y_z_out"]]
    assert {len(h) for h in heads} == {1, 2, 3}
    assert any(f[1] == "n" for h in heads for _, f, _ in h)                       # a batch-norm inside a head
    # the trunk: 0, 1 and 2 residual blocks; first and last conv-like layer; directly behind a block without batch-norm
    trunks = [AS.blocks(a["p_y_z_in"]) for a in archs]
    assert {sum(k == "residual block" for k, _, _ in t) for t in trunks} == {0, 1, 2}
    assert any(t[0][0] == "residual block" for t in trunks) and any(t[-1][0] == "residual block" for t in trunks)
    assert any(b[0] == "residual block" and a[1] is not None and a[1][1] == "-"
               for t in trunks for a, b in zip(t, t[1:]))
    # p_z_in: with and without batch-norm, with a bias, two levels
    pz = [AS.blocks(a["p_z_in"]) for a in archs]
    assert {f[1] for t in pz for _, f, _ in t} == {"n", "-"} and any(f[0] == "b" for t in pz for _, f, _ in t)
    assert {len(t) for t in pz} == {2, 3}
    # recognition / prior nets: the stride orders
    orders = {tuple(cfg["stride"] for _, f, cfg in AS.blocks(a[k]) if f is not None and cfg["kernel_size"] in (4, 8))
              for a in archs for k in ("q_x_in", "q_y_in", "prior_z_y") if k in a}
    assert orders >= {(2, 4, 4), (4, 4, 2), (2, 2, 2, 4), (4, 2, 4)}


def test_every_triple_stands_in_front_of_every_kind_of_layer():
    raw = [a for _, a, _, _ in AS.raw_architectures()]
    table = AS.pair_table(raw)
    missing = [(f, k) for f in AS.TRIPLES for k in AS.NEXT_KINDS if (f, k) not in table]
    assert not missing, missing
    ax = AS.axes(raw)
    assert ax["widths"] == {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 128}
    assert ax["kernels"] == {1, 3, 5, 7, 9}
    assert ax["strided"] == {("conv", 2), ("conv", 4), ("transp conv", 2), ("transp conv", 4)}
    assert len(ax["residual"]) >= 4                                               # tails and branches besides res_block's
    # the softening reaches every ReLU: none is left in what the tests run
    for a in [c[1] for c in CASES]:
        for _, _, seq in AS.net_lists(a):
            assert not [k for k, f, _ in AS.blocks(seq) if f is not None and f[2] == "r"]


@pytest.mark.parametrize("tag", TAGS)
def test_probe_output_agrees_with_torch(tag):
    _, arch, n, _ = AS.case(tag)
    P = {k: torch.from_numpy(v).double() for k, v in AS.parameters(arch).items()}
    r = TorchRefCVAE(arch, P, dtype=torch.float64)
    size, zs = arch["dim_x"][1], arch["dim_z"][1]
    c_hz = probe_output(arch["p_z_in"], 1, zs, zs)[0]
    c_hy = probe_output(arch["p_y_in"], arch["dim_y"][0] + 1, size, size)[0]
    c_h = probe_output(arch["p_y_z_in"], c_hz + c_hy, size, size)[0]
    first = {"q_x_in": (arch["dim_x"][0], size), "q_y_in": (arch["dim_y"][0] + 1, size),
             "prior_z_y": (arch["dim_y"][0] + 1, size), "p_y_in": (arch["dim_y"][0] + 1, size), "p_z_in": (1, zs),
             "p_y_z_in": (c_hz + c_hy, size), "p_y_z_out[0]": (c_h, size), "p_y_z_out[1]": (c_h, size)}
    cq = [probe_output(arch[k], *first[k], first[k][1]) for k in ("q_x_in", "q_y_in")]
    assert cq[0][1:] == cq[1][1:] == (zs, zs)
    first["q_x_y_out"] = (cq[0][0] + cq[1][0], zs)
    for key, prefix, seq in AS.net_lists(arch):
        c, s = first[key]
        with torch.no_grad():
            out = _seq(seq, torch.zeros(n, c, s, s, dtype=torch.float64), r.P, prefix, False)
        want = probe_output(seq, c, s, s)
        got = tuple(out.shape[1:])
        if len(got) == 4:                                   # the latent heads' (2, c, h, w) are 2c channels
            got = (got[0] * got[1], *got[2:])
        assert got == want, (key, out.shape, want)
    assert probe_output(arch["p_z_in"], 1, zs, zs)[1:] == (size, size)
    assert probe_output(arch["p_y_z_out"][0], c_h, size, size) == tuple(arch["dim_x"])
    # the parameter names of the oracle are those of the holders the HIP path builds
    names = []
    for key, prefix, seq in AS.net_lists(arch):
        names += [prefix + k for k, _ in build_holders(seq).named_parameters()]
    assert sorted(names) == sorted(AS.param_shapes(arch))


@pytest.mark.parametrize("tag", TAGS)
def test_float64_graph_is_finite_and_fp32_is_quiet(tag):
    """The stock fp32 evaluation within 2e-4 of the float64 one for every parameter gradient (distance under the scale
    floor of the sweep's limits).  Measured here: worst case 1.1e-4, median case 1e-5."""
    _, arch, n, alpha = AS.case(tag)
    P = AS.parameters(arch)
    x, y, aux, eps, _ = AS.inputs(arch, n, AS.data_seed(tag))
    r64 = evaluate(arch, P, x, y, aux, eps, alpha)
    assert np.isfinite(float(r64.ELBO.detach()))
    g64 = grads(r64)
    assert sorted(g64) == sorted(P) and all(np.isfinite(v).all() for v in g64.values())
    g32 = grads(evaluate(arch, P, x, y, aux, eps, alpha, dtype=torch.float32))
    floors = AS.scale_floors(g64)
    rows = sorted(((AS.distance(g32[k], g64[k], floors[k]), k) for k in g64), reverse=True)
    print("%s: ELBO %.4f, worst fp32 distances" % (tag, float(r64.ELBO)), rows[:3])
    assert rows[0][0] <= 2e-4, rows[:5]


def test_refused_candidates_are_still_valid_graphs():
    """What the HIP path refuses is refused for its own reasons: the same lists evaluate in torch."""
    for tag, arch, n, _, _ in AS.REFUSED + AS.REFUSED_BF16 + AS.REFUSED_BF16_AT_BACKWARD:
        P = AS.parameters(arch)
        x, y, aux, eps, _ = AS.inputs(arch, n)
        assert np.isfinite(float(TorchRefCVAE(arch, P, dtype=torch.float64).forward(x, y, aux, eps))), tag


def test_twin_mapping_restates_the_fiducial_policy():
    """``TorchRefCVAE(bf16=mapping)`` with the fiducial policy written out per layer is ``bf16=True`` bit for bit."""
    from baryon_painter_amd.models import arch as A
    from baryon_painter_amd.utils import synthetic as syn
    arch = syn.softened_architecture(A.fiducial_architecture(64, predict_var=True), AS.SLOPE)
    P = AS.parameters(arch)
    x, y, aux, eps, _ = AS.inputs(arch, 2)
    mapping = {}
    for i, layer in enumerate(arch["p_y_z_in"]):
        if layer[0].lower() in ("conv", "transp conv"):
            mapping[f"p_y_z_in.{i}"] = (True, True, i != 0)
        elif layer[0].lower() == "residual block":
            mapping[f"p_y_z_in.{i}"] = (False, True)
            mapping.update({f"p_y_z_in.{i}.res_block.{j}": (True, True, True) for j in (0, 3)})
    for head in ("p_mu_out", "p_var_out"):
        mapping[head + ".0"], mapping[head + ".2"] = (True, True, True), (True, False, True)
    a, b = (grads(evaluate(arch, P, x, y, aux, eps, 0.3, bf16=m)) for m in (True, mapping))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    c = grads(evaluate(arch, P, x, y, aux, eps, 0.3))
    assert any(not np.array_equal(a[k], c[k]) for k in a)
