#!/usr/bin/env python3
"""Generate tests/golden/cond_net.npz by IMPORTING THE REAL REFERENCE (build container only).

    python tests/golden/make_goldens_cond_net.py

Three small Type-1 CVAEs at 64^2 tiles, batch 2, that differ from the reference's own configurations in the parts of
the model language those leave unused: a ``p_y_in`` network (cvae.py:106-109), ``L = 2`` behind it, and no
``prior_z_y`` (the standard-normal prior of cvae.py:83-85).  Seeded weights and injected eps as in make_goldens.py;
nothing from the reference is copied, only summaries of what it computes are stored (tens of kB).
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
from golden_util import summarize                           # noqa: E402
# (the cases -- architectures() and inputs() -- import without the reference: the tests rebuild them from here)

SIZE, BATCH = 64, 2
SEED_W, SEED_D, SEED_EPS = 7, 1234, 99
CROP = 16


def p_y_in_layers():
    return [("conv", {"in_channels": 2, "out_channels": 4, "kernel_size": 3, "padding": 1, "stride": 1, "bias": False}),
            ("batchnorm", {"num_features": 4}), ("ReLU",)]


SLOPE = 0.9


def architectures():
    """tag -> architecture dict: (a) p_y_in + prior, L = 1; (b) the same, L = 2; (c) p_y_in=None, no prior_z_y.

    The networks around p_y_in are the WELL-CONDITIONED form of the fiducial one (synthetic.softened_architecture: every
    ReLU a LeakyReLU(0.9), PReLU slopes 0.9 -- same layers, kernels and wiring): with ReLUs some unit of ~1.5 million
    always sits within float32 rounding of zero and puts a ~1e-2 floor under any fp32 gradient comparison of two-tile
    cases, and these fixtures are there to hold gradients to 5e-3.  p_y_in itself keeps its ReLU."""
    def build(**kw):
        arch = syn.softened_architecture(our_arch.fiducial_architecture(SIZE, **kw), SLOPE)
        if kw.get("p_y_in") is not None:
            arch["p_y_in"] = p_y_in_layers()
        return arch
    a = build(p_y_in=p_y_in_layers())
    b = build(p_y_in=p_y_in_layers())
    b["L"] = 2
    c = build(prior=False)
    return {"a": a, "b": b, "c": c}


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


def case(tag, arch, out):
    from make_goldens import inject_eps, ref_cvae                       # (imports the reference)
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
    out[f"{tag}/params"] = np.array(",".join(names))
    out[f"{tag}/grad_norm"] = np.array([np.sqrt((p.grad.numpy().astype(np.float64) ** 2).sum())
                                        for _, p in model.named_parameters()])
    for k, p in model.named_parameters():
        if k.startswith("p_y_in."):
            summarize(f"{tag}/grad/{k}", p.grad.numpy(), out)                # (small: stored whole)
    for k, b in model.named_buffers():
        if k.startswith("p_y_in."):
            summarize(f"{tag}/buf/{k}", b.numpy(), out)
    out[f"{tag}/state_keys"] = np.array(",".join(model.state_dict().keys()))
    out[f"{tag}/n_params"] = np.array(model.count_parameters())
    if arch.get("L", 1) == 1:
        # (with L > 1 the reference's sample_P draws L latents per input and then fails to concatenate them with one
        #  h_y per input, cvae.py:100,109,155: there is nothing to record)
        model.train(False)
        with inject_eps(eps1):
            s = model.sample_P(yt, aux_label=at).numpy()
        out[f"{tag}/sample_P_l2"] = np.array(np.sqrt((s.astype(np.float64) ** 2).sum()))
        out[f"{tag}/sample_P_crop"] = crop(s)
    print(tag, "ELBO", float(elbo), "stats", model.get_stats())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    out = {}
    for tag, arch in architectures().items():
        case(tag, arch, out)
    path = os.path.join(HERE, "cond_net.npz")
    np.savez_compressed(path, **out)
    print("cond_net.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
