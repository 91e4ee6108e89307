#!/usr/bin/env python3
"""Generate tests/golden/dense.npz by IMPORTING THE REAL REFERENCE (build container only).

    python tests/golden/make_goldens_dense.py

Two small Type-1 CVAEs at 64^2 tiles, batch 2, with a fully connected bottleneck -- the three words of the reference's
layer vocabulary (``linear``, ``flatten``, ``unflatten`` in front of / behind it; utils.py:132-133, 148-157) that its own
configurations leave unused:
  (s) a spatial latent dim_z = (1, 2, 2) behind dense tails of q_x_y_out and prior_z_y;
  (v) a vector latent dim_z = (12,): two linear layers in q_x_y_out, one in the prior's tail, and a linear + unflatten
      in front of p_z_in's transposed convolutions.
Every other part is the softened fiducial network, with seeded weights and injected eps as in make_goldens_cond_net.py.
Nothing from the reference is copied: summaries of what it computes are stored (tens of kB), and the float64 oracle's
gradient noise floor per parameter, so that the GPU tests need one oracle pass instead of five.
"""
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
# (the cases -- architectures(), parameters() and inputs() -- import without the reference: the tests rebuild them)

SIZE, BATCH = 64, 2
SEED_W, SEED_D, SEED_EPS = 7, 1234, 99
CROP = 16
SLOPE = 0.9
DIM_V = 12


def _linear(k, o, bias=True):
    return ("linear", {"in_features": k, "out_features": o, "bias": bias})


def architectures():
    """tag -> architecture dict: "s" (spatial latent, dense tails) and "v" (vector latent).  The rest is the
    WELL-CONDITIONED fiducial network of make_goldens_cond_net.architectures()."""
    def prior_stem():
        return our_arch.conv_down(in_channel=2, channels=[8, 16, 32], scales=[2, 4, 4])      # -> (32, 2, 2) at 64^2

    s = our_arch.fiducial_architecture(SIZE)
    s["q_x_y_out"] = [("flatten",), _linear(256, 8), ("unflatten", (2, 1, 2, 2))]
    s["prior_z_y"] = prior_stem() + [("flatten",), _linear(128, 8), ("unflatten", (2, 1, 2, 2))]
    v = our_arch.fiducial_architecture(SIZE)
    v["dim_z"] = (DIM_V,)
    v["q_x_y_out"] = [("flatten",), _linear(256, 40), ("Leaky ReLU", SLOPE), _linear(40, 2 * DIM_V, bias=False),
                      ("unflatten", (2, DIM_V))]
    v["prior_z_y"] = prior_stem() + [("flatten",), _linear(128, 2 * DIM_V), ("unflatten", (2, DIM_V))]
    v["p_z_in"] = [_linear(DIM_V, 4), ("unflatten", (1, 2, 2))] + list(v["p_z_in"])
    return {"s": syn.softened_architecture(s, SLOPE), "v": syn.softened_architecture(v, SLOPE)}


def parameters(shapes):
    """Seeded weights for name -> shape, PReLU slopes at SLOPE."""
    return syn.soften_params(syn.fill_params(shapes, SEED_W), SLOPE)


def inputs(arch):
    x, y, aux = syn.synthetic_batch(BATCH, SIZE, SIZE, seed=SEED_D)
    eps = syn.synthetic_eps((arch.get("L", 1), BATCH, *arch["dim_z"]), seed=SEED_EPS)
    eps1 = syn.synthetic_eps((1, BATCH, *arch["dim_z"]), seed=SEED_EPS + 1)
    return x, y, aux, eps, eps1


def crop(a):
    return np.ascontiguousarray(np.asarray(a)[..., :CROP, :CROP], dtype=np.float32)


def dense_names(arch, names):
    """The parameters of the linear layers among ``names`` (state_dict keys)."""
    out = []
    for key, prefix in (("q_x_y_out", "q_out."), ("prior_z_y", "prior_network."), ("p_z_in", "p_z_in.")):
        for i, layer in enumerate(arch.get(key) or []):
            if layer[0].lower() == "linear":
                out += [k for k in names if k in (f"{prefix}{i}.weight", f"{prefix}{i}.bias")]
    return out


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def noise_floors(arch, P, x, y, aux, eps, g):
    """How far the TRUE gradient moves under 2^-20 perturbations of the parameters (tests/test_gpu_cond_net.py: four
    draws of default_rng(7)), per parameter, against the float64 oracle's gradient ``g``."""
    from oracle.cvae_oracle import CVAEOracle
    floor = {k: 0.0 for k in g}
    rng = np.random.default_rng(7)
    for _ in range(4):
        pert = CVAEOracle(arch, dtype=np.float64)
        pert.load_params({k: np.asarray(v, np.float64) * (1.0 + 2.0 ** -20 * rng.uniform(-1, 1, np.shape(v)))
                          for k, v in P.items()})
        pert.forward(x, y, aux, eps)
        gp = pert.backward(seed=-1.0)
        for k in g:
            floor[k] = max(floor[k], rel_err(gp[k], g[k]))
    return floor


def case(tag, arch, out):
    from make_goldens import inject_eps, ref_cvae                       # (imports the reference)
    from oracle.cvae_oracle import CVAEOracle
    model = ref_cvae.CVAE(arch, "cpu")
    vals = parameters({k: tuple(v.shape) for k, v in model.named_parameters()})
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(torch.from_numpy(vals[k]))
    x, y, aux, eps, eps1 = inputs(arch)
    xt, yt, at = torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux)
    model.train(True)
    with inject_eps(eps):
        elbo = model(xt, yt, at)
    (-elbo).backward()
    out[f"{tag}/stats"] = np.array(model.get_stats(), np.float64)          # ELBO, -KL, log-likelihood
    xm = model.x_mu.detach().numpy()
    out[f"{tag}/x_mu_shape"] = np.array(xm.shape)
    out[f"{tag}/x_mu_l2"] = np.array(np.sqrt((xm.astype(np.float64) ** 2).sum()))
    out[f"{tag}/x_mu_crop"] = crop(xm)
    names = [k for k, _ in model.named_parameters()]
    grads = {k: p.grad.numpy() for k, p in model.named_parameters()}
    out[f"{tag}/params"] = np.array(",".join(names))
    out[f"{tag}/grad_norm"] = np.array([np.sqrt((grads[k].astype(np.float64) ** 2).sum()) for k in names])
    for k in dense_names(arch, names):
        out[f"{tag}/grad/{k}"] = np.ascontiguousarray(grads[k], np.float32)          # (small: stored whole)
    out[f"{tag}/state_keys"] = np.array(",".join(model.state_dict().keys()))
    out[f"{tag}/n_params"] = np.array(model.count_parameters())
    model.train(False)
    with inject_eps(eps1):
        s = model.sample_P(yt, aux_label=at).numpy()
    out[f"{tag}/sample_P_l2"] = np.array(np.sqrt((s.astype(np.float64) ** 2).sum()))
    out[f"{tag}/sample_P_crop"] = crop(s)
    # the float64 oracle on the same case: its noise floors, and how far the reference's fp32 run lies from it
    ora = CVAEOracle(arch, dtype=np.float64)
    ora.load_params(vals)
    ora.forward(x, y, aux, eps)
    g = ora.backward(seed=-1.0)
    floor = noise_floors(arch, vals, x, y, aux, eps, g)
    for k in names:
        out[f"{tag}/floor/{k}"] = np.array(floor[k])
    worst = sorted(((rel_err(grads[k], g[k]), floor[k], k) for k in names), reverse=True)
    print(tag, "ELBO", float(elbo), "stats", model.get_stats(), "n_params", model.count_parameters())
    print(tag, "reference vs float64 oracle: losses",
          np.abs(np.array(model.get_stats()) - np.array(ora.get_stats())).max() / np.abs(np.array(ora.get_stats())).max(),
          "x_mu", rel_err(xm, ora.x_mu), "worst gradients (error, floor, name)", worst[:3],
          "worst floor", max(floor.items(), key=lambda kv: kv[1]))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    out = {}
    for tag, arch in architectures().items():
        case(tag, arch, out)
    path = os.path.join(HERE, "dense.npz")
    np.savez_compressed(path, **out)
    print("dense.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
