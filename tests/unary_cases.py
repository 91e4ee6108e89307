"""The three cases of tests/golden/unary.npz (tests/golden/make_goldens_unary.py ran the reference on them): Type-1
CVAEs at 64^2, batch 2, whose layer lists hold tanh / sigmoid / softplus where the HIP path compiles them to
``graph.UnaryUnit`` s.  Imports without the reference: the host and GPU tests rebuild the cases from here.

  heads     two heads; the mean head ends in tanh, the variance head in softplus; alpha_var = 0.3
  interior  q_x_in = conv_down(activation="sigmoid") (the last sigmoid writes the recognition concat slice); one
            interior softplus in prior_z_y; p_z_in = conv_up(activation="tanh") (the last tanh writes h_z's slice of the
            generator's input); in p_y_z_in a sigmoid between two plain conv blocks and a tanh directly behind the first
            residual block; the variance head ends in tanh (the mean head keeps its fused softplus)
  ytanh     a p_y_in network conv + batchnorm + tanh, L = 2 (the tanh writes the slot that is repeated over L)
Every other part is the softened fiducial network, with seeded weights and injected eps as in make_goldens_dense.py."""
import numpy as np

from baryon_painter_amd.models import arch as our_arch
from baryon_painter_amd.utils import synthetic as syn

SIZE, BATCH = 64, 2
SEED_W, SEED_D, SEED_EPS = 7, 1234, 99
CROP = 16
SLOPE = 0.9
ALPHA_VAR = {"heads": 0.3, "interior": 1.0, "ytanh": 1.0}
UNARY = ("tanh", "sigmoid", "softplus")
NETS = (("q_x_in", "q_x_in"), ("q_y_in", "q_y_in"), ("q_x_y_out", "q_out"), ("p_y_in", "p_y_in"), ("p_z_in", "p_z_in"),
        ("p_y_z_in", "p_y_z_in"), ("prior_z_y", "prior_network"))


def architectures():
    A = our_arch
    heads = A.fiducial_architecture(SIZE, predict_var=True)
    mu, var = heads["p_y_z_out"]
    assert mu[-1] == ("softplus",)
    heads["p_y_z_out"] = (list(mu[:-1]) + [("tanh",)], list(var) + [("softplus",)])

    interior = A.fiducial_architecture(SIZE, predict_var=True)
    interior["q_x_in"] = A.conv_down(in_channel=1, channels=[8, 16, 32], scales=[2, 4, 4], activation="sigmoid")
    interior["prior_z_y"] = (A.conv_down(in_channel=2, channels=[8], scales=[2])
                             + A.conv_down(in_channel=8, channels=[16], scales=[4], activation="softplus")
                             + A.conv_down(in_channel=16, channels=[32], scales=[4])
                             + A.conv_block(32, 2, kernel=5) + [("unflatten", (2, 1, 2, 2))])
    interior["p_z_in"] = A.conv_up(1, channels=[1, 1, 1], scales=[2, 4, 4], bias=False, batchnorm=True, activation="tanh")
    interior["p_y_z_in"] = (A.conv_block(3, 16, kernel=5, activation="sigmoid")
                            + A.conv_down(in_channel=16, channels=[32, 64, 128], scales=[2, 2, 2])
                            + [("residual block", A.res_block(128)), ("tanh",)]
                            + [("residual block", A.res_block(128)) for _ in range(3)]
                            + A.conv_up(128, channels=[64, 32, 16], scales=[2, 2, 2], bias=False, batchnorm=True,
                                        activation="ReLU"))
    mu, var = interior["p_y_z_out"]
    interior["p_y_z_out"] = (list(mu), list(var) + [("tanh",)])

    ytanh = A.fiducial_architecture(SIZE, p_y_in=A.conv_block(2, 4, kernel=3, batchnorm=True, activation="tanh"))
    ytanh["L"] = 2
    return {k: syn.softened_architecture(v, SLOPE) for k, v in (("heads", heads), ("interior", interior),
                                                                 ("ytanh", ytanh))}


def parameters(shapes):
    """Seeded weights for name -> shape, PReLU slopes at SLOPE."""
    return syn.soften_params(syn.fill_params(shapes, SEED_W), SLOPE)


def inputs(arch):
    x, y, aux = syn.synthetic_batch(BATCH, SIZE, SIZE, seed=SEED_D)
    eps = syn.synthetic_eps((arch.get("L", 1), BATCH, *arch["dim_z"]), seed=SEED_EPS)
    eps1 = syn.synthetic_eps((1, BATCH, *arch["dim_z"]), seed=SEED_EPS + 1)
    zfix = syn.synthetic_eps((BATCH, *arch["dim_z"]), seed=101)
    return x, y, aux, eps, eps1, zfix


def crop(a):
    return np.ascontiguousarray(np.asarray(a)[..., :CROP, :CROP], dtype=np.float32)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def net_lists(arch):
    """(architecture key, state-dict prefix, layer list) of every net the architecture has."""
    out = [(key, attr + ".", arch.get(key)) for key, attr in NETS]
    out += [(f"p_y_z_out[{i}]", ("p_mu_out.", "p_var_out.")[i], seq) for i, seq in enumerate(arch["p_y_z_out"][:2])]
    return [(k, p, list(seq)) for k, p, seq in out if seq]


def unary_layers(arch):
    """[(module name as in the reference's state dict, e.g. "q_x_in.2", kind)] of every tanh / sigmoid / softplus."""
    return [(f"{prefix}{i}", layer[0].lower()) for _, prefix, seq in net_lists(arch)
            for i, layer in enumerate(seq) if layer[0].lower() in UNARY]


def front_names(arch, names):
    """The parameters of the layer directly in front of each tanh / sigmoid / softplus among ``names``: the convolution
    and, where there is one, its batch-norm; behind a residual block, the last convolution + batch-norm of its branch."""
    out = []
    for _, prefix, seq in net_lists(arch):
        for i, layer in enumerate(seq):
            if layer[0].lower() not in UNARY or i == 0:
                continue
            j, mods = i - 1, []
            if seq[j][0].lower() == "residual block":
                body = seq[j][1][0]
                k = len(body) - 1
                mods.append(f"{prefix}{j}.res_block.{k}.")
                if body[k][0].lower() == "batchnorm":
                    mods.append(f"{prefix}{j}.res_block.{k - 1}.")
            else:
                mods.append(f"{prefix}{j}.")
                if seq[j][0].lower() == "batchnorm" and j > 0:
                    mods.append(f"{prefix}{j - 1}.")
            out += [n for n in names if any(n.startswith(m) and "." not in n[len(m):] for m in mods) and n not in out]
    return out


def unsaturated(kind, y):
    """Fraction of a layer's elements with f' >= 0.05, from its output y."""
    y = np.asarray(y, np.float64)
    d = {"tanh": 1 - y * y, "sigmoid": y * (1 - y), "softplus": -np.expm1(-y)}[kind]
    return float((d >= 0.05).mean())


def noise_floors(arch, P, x, y, aux, eps, g, alpha_var=1.0):
    """How far the TRUE gradient moves under 2^-20 perturbations of the parameters (make_goldens_dense.noise_floors:
    four draws of default_rng(7)), per parameter, against the float64 oracle's gradient ``g``."""
    from oracle.cvae_oracle import CVAEOracle
    floor = {k: 0.0 for k in g}
    rng = np.random.default_rng(7)
    for _ in range(4):
        pert = CVAEOracle(arch, dtype=np.float64)
        pert.alpha_var = alpha_var
        pert.load_params({k: np.asarray(v, np.float64) * (1.0 + 2.0 ** -20 * rng.uniform(-1, 1, np.shape(v)))
                          for k, v in P.items()})
        pert.forward(x, y, aux, eps)
        gp = pert.backward(seed=-1.0)
        for k in g:
            floor[k] = max(floor[k], rel_err(gp[k], g[k]))
    return floor
