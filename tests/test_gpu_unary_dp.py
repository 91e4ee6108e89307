"""GPU: data parallelism (sync=) with tanh / sigmoid / softplus layers (graph.UnaryUnit) in the plan.  Two gloo ranks share
the one GPU, as in tests/test_gpu_painter.py::test_two_rank_data_parallel_equals_single_device, whose criteria these are:
the sharded batch with global batch-norm statistics and averaged gradients equals the single-device global batch.

Cases of tests/unary_cases.py, batch 4 (two samples per rank):
  interior  units stand in q_x_in and prior_z_y, so the level-by-level schedule of the recognition / prior branches
            gives way to per-layer collectives (``_Plan._build_levels`` returns None); in p_z_in and the generator a unit
            stands between two batch-norm layers whose statistics are global
  heads     units behind the last convolution of both heads
``transport``: how the statistics travel (peer memory inside the finalize kernels / the process group's all-reduce);
``early``: the trunk's gradients reduced on the weight-gradient stream through a second communicator."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch, torch.distributed as dist
import unary_cases as UC
from baryon_painter_amd.dist import Sync
from baryon_painter_amd.models.cvae import CVAE
from baryon_painter_amd.models.graph import UnaryUnit
from baryon_painter_amd.utils import synthetic as syn
tag, early, transport = sys.argv[3], sys.argv[4], sys.argv[5]
r = int(os.environ["RANK"])
dev = "cuda:0"
torch.cuda.set_device(dev)
dist.init_process_group("gloo")
w = dist.get_world_size()
n = 4
arch = UC.architectures()[tag]
x, y, aux = syn.synthetic_batch(n, UC.SIZE, UC.SIZE, seed=UC.SEED_D)
eps = syn.synthetic_eps((1, n, *arch["dim_z"]), seed=UC.SEED_EPS)
def run(sync, sl):
    m = CVAE(arch, dev, sync=sync)
    m.alpha_var = UC.ALPHA_VAR[tag]
    P = UC.parameters({k: tuple(p.shape) for k, p in m.named_parameters()})
    with torch.no_grad():
        for k, p in m.named_parameters(): p.copy_(torch.from_numpy(P[k]))
    m._eps_override = eps[:, sl]
    e = m(torch.from_numpy(x[sl]), torch.from_numpy(y[sl]), torch.from_numpy(aux[sl]))
    (-e).backward()
    torch.cuda.synchronize()
    return m, float(e.detach())
h = n // w
sync = Sync(grad_group="new" if early == "1" else None)
assert sync.active and sync.sync_bn and sync.overlap == (early == "1")
if early == "1":
    os.environ["BP_EARLY_ALLREDUCE"] = "1"
dp, e_dp = run(sync, slice(r * h, (r + 1) * h))
plan = dp._last
units = plan.flat_units([u for us in plan.q_units + [plan.p_units] + plan.g_units + [plan.mu_units, plan.var_units]
                         for u in us])
assert sorted(u.name for u in units if isinstance(u, UnaryUnit)) == sorted(
    k for k, kind in UC.unary_layers(arch) if not (k.startswith("p_mu_out.") and kind == "softplus"))
assert sync.n_grad == (3 if early == "1" else 1), sync.n_grad
if transport == "peer":
    assert sync.peer is not None and sync.peer.world == w and sync.n_fused > 0, sync.n_fused
else:
    assert sync.peer is None and sync.n_fused == 0
    assert plan.levels is None      # a unit among the recognition / prior branches: no level shares one collective
sync.check()
t = torch.tensor([e_dp], dtype=torch.float64); dist.all_reduce(t); e_mean = t.item() / w
if r == 0:
    ref, e_ref = run(None, slice(0, n))
    assert abs(e_mean - e_ref) <= 2e-6 * abs(e_ref), (e_mean, e_ref)
    errs = []
    for (k, a), (_, b) in zip(dp.named_parameters(), ref.named_parameters()):
        ga, gb = a.grad.double(), b.grad.double()
        errs.append((float((ga - gb).abs().max() / gb.abs().max().clamp_min(1e-30)), k))
    errs.sort(reverse=True)
    print("worst:", errs[:6])
    for (k, a), (_, b) in zip(dp.named_buffers(), ref.named_buffers()):
        assert torch.allclose(a.double(), b.double(), rtol=1e-5, atol=1e-7), k
    # fp32: the sharded sums differ from the single-device ones in summation order only
    assert errs[0][0] < 2e-4, errs[:6]
    open(os.path.join(sys.argv[2], "dp.ok"), "w").write(str(errs[0][0]))
dist.barrier()
dist.destroy_process_group()
"""


@pytest.mark.parametrize("tag,early,transport", [("interior", "0", "peer"), ("interior", "0", "group"),
                                                 ("interior", "1", "peer"), ("heads", "0", "peer")])
def test_two_rank_data_parallel_equals_single_device(tmp_path, tag, early, transport):
    script = tmp_path / "dp_worker.py"
    script.write_text(_WORKER)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("BP_EARLY_ALLREDUCE", "BP_PEER_SYNC", "BP_PEER_FUSED", "BP_LEVEL_SYNC"):
        env.pop(k, None)
    if transport == "group":
        env["BP_PEER_SYNC"] = "0"
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), str(script), ROOT, str(tmp_path),
                          tag, early, transport],
                         capture_output=True, text=True, env=env, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert (tmp_path / "dp.ok").exists()
