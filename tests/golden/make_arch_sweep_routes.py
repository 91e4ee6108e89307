"""Writes tests/golden/arch_sweep_routes.json: ``ConvUnit.route()`` of every convolution unit of every case of
tests/arch_sweep.py after one training step under the default routing of the statistics (needs the GPU: the fusion
decisions fall at the first backward pass).  tests/test_gpu_arch_sweep.py compares against it, so a later change of a
decision of the plan compiler shows up as a diff of that file.

    python tests/golden/make_arch_sweep_routes.py [output path]
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import arch_sweep as AS                                         # noqa: E402
from plan_units import conv_units                               # noqa: E402


def main(path):
    from baryon_painter_amd.models.cvae import CVAE
    out = {}
    for tag, arch, n, alpha in AS.cases():
        P = AS.parameters(arch)
        x, y, aux, eps, _ = AS.inputs(arch, n, AS.data_seed(tag))
        m = CVAE(arch, "cuda:0")
        with torch.no_grad():
            for k, p in m.named_parameters():
                p.copy_(torch.from_numpy(P[k]))
        m.alpha_var = alpha
        m._eps_override = eps
        (-m(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(aux))).backward()
        torch.cuda.synchronize()
        out[tag] = {u.name: u.route() for u in conv_units(m._last) if hasattr(u, "route")}
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, sum(len(v) for v in out.values()), "units of", len(out), "cases")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "arch_sweep_routes.json"))
