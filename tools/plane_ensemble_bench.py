"""What a plane ensemble costs: the fiducial 512^2 CVAE with synthetic weights (``tools/plane_bench.py``'s painter) on a
4096^2 plane of 512^2 tiles at half a tile of overlap (225 tiles), batches of 64 generator samples, all in one process.
One JSON line per measurement:

  plane_moments         bp_plane_moments alone over K accumulator pairs of the plane (count = 4096^2, with weights,
                        without the planes): ``--rounds`` rounds of ``--launches`` launches between two device events;
                        every round, the median, the bytes (2 K + 2 doubles per element) and GB/s, beside the streaming
                        rate of HBM (6.3 TB/s achievable on an MI355X)
  paint_plane_ensemble  ``paint_plane_ensemble(on_device=True, draws=K)``: host delta in, mean and variance out
  paint_plane_k_seeds   ``paint_plane(on_device=True)`` under K seeds, then NumPy's float64 mean and variance over the K
                        downloaded planes on the host -- what a user did before.  The two legs alternate,
                        ``--repeats`` times each, for every K of ``--draws``; every repeat is reported

No figure is fixed in advance.  Usage: python tools/plane_ensemble_bench.py [--draws 4,16] [--repeats 3] [--batch 64]
[--launches 20] [--rounds 5] [--n-plane 4096]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from baryon_painter_amd import lightcone as LC  # noqa: E402
from plane_bench import TILE, make_painter  # noqa: E402

HBM_GB_PER_S = 6300.0


def kernel_times(K, count, launches, rounds):
    """ms per bp_plane_moments launch over (K, count) accumulators and weights: one figure per round."""
    import ctypes as C

    from baryon_painter_amd import _lib as L
    lib = L.load()
    acc = torch.rand((K, count), dtype=torch.float64, device="cuda") + 0.5
    wsum = torch.rand((K, count), dtype=torch.float64, device="cuda") + 0.5
    mean, var = (torch.empty(count, dtype=torch.float64, device="cuda") for _ in range(2))
    sm = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch():
        L.check(lib.bp_plane_moments(L.ptr(acc), L.ptr(wsum), K, count, L.ptr(mean), L.ptr(var), None, sm), "moments")
    for _ in range(3):
        launch()
    times = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            launch()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / launches)
    p = acc[:, :65536] / wsum[:, :65536]                         # (the kernel's own order is pinned by the tests)
    assert torch.allclose(mean[:65536], p.mean(0), rtol=1e-12) and \
        torch.allclose(var[:65536], p.var(0, unbiased=False), rtol=1e-9, atol=1e-15)
    return times


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", default="4,16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n-plane", type=int, default=4096)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plane_ensemble_bench.py measures on a GPU: none found")
    draws = [int(k) for k in args.draws.split(",")]
    n_plane = args.n_plane
    count = n_plane * n_plane
    for K in draws:
        ms = kernel_times(K, count, args.launches, args.rounds)
        nbytes = (2 * K + 2) * 8 * count
        med = float(np.median(ms))
        print(json.dumps({"measurement": "plane_moments", "draws": K, "count": count, "launches_per_round": args.launches,
                          "ms": [round(v, 4) for v in ms], "median_ms": round(med, 4), "bytes": nbytes,
                          "GB_per_s": round(nbytes / (med * 1e-3) / 1e9, 1),
                          "share_of_hbm_streaming_rate": round(nbytes / (med * 1e-3) / 1e9 / HBM_GB_PER_S, 3)}),
              flush=True)
        torch.cuda.empty_cache()
    pt = make_painter("f32", torch.device("cuda:0"))
    rel, z = TILE / n_plane, 0.5
    rng = np.random.Generator(np.random.PCG64(n_plane))
    delta = (np.exp(rng.standard_normal((n_plane, n_plane), dtype=np.float32) * 0.5) * 0.05).astype(np.float32)
    n_tiles = len(LC.plane_geometry(n_plane, rel, TILE)["origins"])
    common = {"n_plane": n_plane, "tile": TILE, "tiles": n_tiles, "batch": args.batch}

    def ensemble(K):
        return LC.paint_plane_ensemble(pt, delta, rel, TILE, z, K, batch_size=args.batch, seed=5, on_device=True)

    def k_seeds(K):
        runs = np.stack([LC.paint_plane(pt, delta, rel, TILE, z, batch_size=args.batch, seed=5 + k, on_device=True)
                         for k in range(K)])
        return runs.mean(axis=0, dtype=np.float64), runs.var(axis=0, dtype=np.float64)
    with torch.no_grad():
        for K in draws:
            for r in range(-1, args.repeats):                    # repeat -1: capture and first launches, not reported
                for name, fn in (("paint_plane_ensemble", ensemble), ("paint_plane_k_seeds", k_seeds)):
                    dt, (mean, var) = timed(lambda: fn(K if r >= 0 or fn is ensemble else 1))
                    ok = np.isfinite(mean)
                    assert ok.mean() > 0.9 and (var[ok] >= 0).all()
                    if r >= 0:
                        print(json.dumps({"measurement": name, "draws": K, "repeat": r, "seconds": round(dt, 4),
                                          "draws_per_s": round(n_tiles * K / dt, 1), **common}), flush=True)
            pt.release_paint_buffers()                           # (the K accumulator pairs of this K)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
