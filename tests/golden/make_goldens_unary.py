#!/usr/bin/env python3
"""Generate tests/golden/unary.npz by IMPORTING THE REAL REFERENCE (build container only).

    python tests/golden/make_goldens_unary.py

The three cases of tests/unary_cases.py -- tanh / sigmoid / softplus layers at the heads, inside the nets and at the end
of a p_y_in network -- run through the reference's CVAE at 64^2, batch 2, with seeded weights and injected eps, by the
recipe of make_goldens_dense.py.  Nothing from the reference is copied: summaries and crops of what it computes are
stored (tens of kB), the float64 oracle's gradient noise floor per parameter (``floor/<name>``), and, per saturating
layer, the fraction of its elements whose derivative is at least 0.05 in the reference's training forward
(``unsat/<module>``).  A layer that is saturated everywhere would test nothing: the generator refuses to write a fixture
in which any of these fractions is below one half.  The archive is written with fixed time stamps, so the same inputs
give the same bytes.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import unary_cases as UC                                      # noqa: E402

FULL_GRAD_MAX = 4096          # gradients of the layers in front of a unary layer are stored whole up to this size


def case(tag, arch, out):
    from make_goldens import inject_eps, ref_cvae                       # (imports the reference)
    from oracle.cvae_oracle import CVAEOracle
    model = ref_cvae.CVAE(arch, "cpu")
    model.alpha_var = UC.ALPHA_VAR[tag]
    vals = UC.parameters({k: tuple(v.shape) for k, v in model.named_parameters()})
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(torch.from_numpy(vals[k]))
    x, y, aux, eps, eps1, zfix = UC.inputs(arch)
    xt, yt, at = torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux)
    # what every saturating layer puts out in the training forward
    seen, hooks = {}, []
    mods = dict(model.named_modules())
    for name, kind in UC.unary_layers(arch):
        hooks.append(mods[name].register_forward_hook(
            lambda m, i, o, name=name: seen.__setitem__(name, o.detach().numpy().copy())))
    model.train(True)
    with inject_eps(eps):
        elbo = model(xt, yt, at)
    (-elbo).backward()
    for h in hooks:
        h.remove()
    for name, kind in UC.unary_layers(arch):
        frac = UC.unsaturated(kind, seen[name])
        print(tag, name, kind, "unsaturated fraction", frac)
        assert frac >= 0.5, (tag, name, kind, frac)
        out[f"{tag}/unsat/{name}"] = np.array(frac)
    out[f"{tag}/stats"] = np.array(model.get_stats(), np.float64)
    xm = model.x_mu.detach().numpy()
    out[f"{tag}/x_mu_shape"] = np.array(xm.shape)
    out[f"{tag}/x_mu_l2"] = np.array(np.sqrt((xm.astype(np.float64) ** 2).sum()))
    out[f"{tag}/x_mu_crop"] = UC.crop(xm)
    out[f"{tag}/z_mu"] = np.ascontiguousarray(model.z_mu.detach().numpy(), np.float32)
    out[f"{tag}/z_log_var"] = np.ascontiguousarray(model.z_log_var.detach().numpy(), np.float32)
    names = [k for k, _ in model.named_parameters()]
    grads = {k: p.grad.numpy() for k, p in model.named_parameters()}
    out[f"{tag}/params"] = np.array(",".join(names))
    out[f"{tag}/grad_norm"] = np.array([np.sqrt((grads[k].astype(np.float64) ** 2).sum()) for k in names])
    for k in UC.front_names(arch, names):
        if grads[k].size <= FULL_GRAD_MAX:
            out[f"{tag}/grad/{k}"] = np.ascontiguousarray(grads[k], np.float32)
    out[f"{tag}/state_keys"] = np.array(",".join(model.state_dict().keys()))
    out[f"{tag}/n_params"] = np.array(model.count_parameters())
    # batch-norm running statistics after the step, end to end in the order of ``buffer_names``
    bufs = [(k, b.detach().numpy().astype(np.float64).reshape(-1)) for k, b in model.named_buffers()]
    out[f"{tag}/buffer_names"] = np.array(",".join(k for k, _ in bufs))
    out[f"{tag}/buffers"] = np.concatenate([b for _, b in bufs])
    model.train(False)
    if arch.get("L", 1) == 1:
        # (with L > 1 the reference's sample_P draws L latents per input and then fails to concatenate them with one
        #  h_y per input, cvae.py:100,109,155: only the fixed-z sample below exists there)
        with inject_eps(eps1):
            s = model.sample_P(yt, aux_label=at).numpy()
        out[f"{tag}/sample_P_l2"] = np.array(np.sqrt((s.astype(np.float64) ** 2).sum()))
        out[f"{tag}/sample_P_crop"] = UC.crop(s)
    s = model.sample_P(yt, aux_label=at, z=torch.from_numpy(zfix)).numpy()
    out[f"{tag}/sample_P_z_l2"] = np.array(np.sqrt((s.astype(np.float64) ** 2).sum()))
    out[f"{tag}/sample_P_z_crop"] = UC.crop(s)
    # the float64 oracle on the same case: its noise floors, and how far the reference's fp32 run lies from it
    ora = CVAEOracle(arch, dtype=np.float64)
    ora.alpha_var = UC.ALPHA_VAR[tag]
    ora.load_params(vals)
    ora.forward(x, y, aux, eps)
    g = ora.backward(seed=-1.0)
    floor = UC.noise_floors(arch, vals, x, y, aux, eps, g, UC.ALPHA_VAR[tag])
    for k in names:
        out[f"{tag}/floor/{k}"] = np.array(floor[k])
    worst = sorted(((UC.rel_err(grads[k], g[k]), floor[k], k) for k in names), reverse=True)
    print(tag, "ELBO", float(elbo), "stats", model.get_stats(), "n_params", model.count_parameters())
    print(tag, "reference vs float64 oracle: losses",
          np.abs(np.array(model.get_stats()) - np.array(ora.get_stats())).max() / np.abs(np.array(ora.get_stats())).max(),
          "x_mu", UC.rel_err(xm, ora.x_mu), "worst gradients (error, floor, name)", worst[:3],
          "worst floor", max(floor.items(), key=lambda kv: kv[1]))


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps (numpy stamps each member with the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    out = {}
    for tag, arch in UC.architectures().items():
        case(tag, arch, out)
    path = os.path.join(HERE, "unary.npz")
    write_npz(path, out)
    print("unary.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
