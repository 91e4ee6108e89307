"""Compton-y map of a light cone: lightcone.paint_light_cone on the host path (paint_plane + SciPy's zoom per plane)
against the device path (on_device=True: painted planes stay on the GPU and csrc/ymap.hip projects them), and the
projection alone.  Fiducial 512^2 architecture with synthetic weights (as tools/plane_bench.py builds it).  The light
cone: ``--planes`` (3) periodic delta planes of ``--delta``^2 (4096) float32 pixels, painted as ``--delta``^2 planes of
512^2 tiles at 0.5 overlap, into a ``--res``^2 (4096) map, resampled with splines of ``--order`` (3; 2 to 5, the orders
the device path has) on both paths.  One JSON line:

  projection_host_s            the painted planes downloaded from the device and projected by project_planes (SciPy, one
                               core), one run; ``_download_s`` is the download's share
  projection_device_s          project_planes(on_device=True, out=...) on the same planes, resident: HIP events around
                               the whole light cone's projection, median / min / max over ``--reps`` after one warm-up
  projection_bytes             algorithmic bytes of the projection per light cone: every plane read once, the map read
                               and written once per plane, float64; ``projection_kernel_bytes`` adds what the kernels
                               move beyond that (two coefficient images written and read back)
  projection_hbm_fraction      projection_bytes / median time / 8 TB/s
  light_cone_host_s, _device_s paint_light_cone end to end on either path (one run each after a warm-up of the device
                               path, which captures the graphs both use)
  host_link_bytes              bytes over the host link per light cone, from the sizes: host path the float32 tiles up
                               and down; device path the deltas up and the map down

Usage: python tools/ymap_bench.py [--dtype f32] [--planes 3] [--delta 4096] [--res 4096] [--reps 5] [--batch 64]
       [--order 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from baryon_painter_amd import lightcone as LC  # noqa: E402
from plane_bench import TILE, make_painter  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--planes", type=int, default=3)
    ap.add_argument("--delta", type=int, default=4096)
    ap.add_argument("--res", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--order", type=int, default=3, choices=(2, 3, 4, 5))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ymap_bench needs a GPU")
    n, res, k = args.delta, args.res, args.planes
    pt = make_painter(args.dtype, torch.device("cuda:0"))
    tile_size = 100.0
    delta_size = [tile_size * n / TILE] * k                      # tile_relative_size = 512 / n: no resampling
    z = list(np.linspace(0.3, 0.9, k))
    chi = np.linspace(900.0, 2200.0, k)
    geo = LC.plane_geometry(n, tile_size / delta_size[0], TILE)
    n_plane, n_tiles = geo["n_plane"], len(geo["origins"])
    scales = LC.y_map_scales([n_plane] * k, res, 10.0, chi, lambda c: 1 / (1 + c / 3300.0), 0.69)
    deltas = []
    for i in range(k):
        rng = np.random.Generator(np.random.PCG64(100 + i))
        deltas.append((np.exp(rng.standard_normal((n, n), dtype=np.float32) * 0.5) * 0.05).astype(np.float32))
    kw = dict(tile_size=tile_size, n_pixel_tile=TILE, resolution=res, scales=scales, batch_size=args.batch, seed=11,
              order=args.order)

    # ---- whole light cone, both paths
    LC.paint_light_cone(pt, deltas, z, delta_size, on_device=True, **kw)                   # capture + warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y_dev = LC.paint_light_cone(pt, deltas, z, delta_size, on_device=True, **kw)
    t_cone_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    y_host = LC.paint_light_cone(pt, deltas, z, delta_size, **kw)
    t_cone_host = time.perf_counter() - t0
    diff = float(np.abs(y_dev - y_host).max() / np.abs(y_host).max())

    # ---- the projection alone, on painted planes that are resident
    planes = []
    for i in range(k):
        out = torch.empty((n_plane, n_plane), dtype=torch.float64, device="cuda")
        LC.paint_plane(pt, deltas[i], tile_size / delta_size[i], TILE, z[i], batch_size=args.batch, seed=11,
                       first_tile_id=i * n_tiles, on_device=True, out=out)
        planes.append(out)
    y = torch.zeros((res, res), dtype=torch.float64, device="cuda")
    LC.project_planes(planes, scales, res, order=args.order, on_device=True, out=y)       # warm-up (scratch allocated)
    times = []
    for _ in range(args.reps):
        y.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        LC.project_planes(planes, scales, res, order=args.order, on_device=True, out=y)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    t_proj_dev = float(np.median(times))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_planes = [p.cpu().numpy() for p in planes]
    t_down = time.perf_counter() - t0
    y_ref = LC.project_planes(host_planes, scales, res, order=args.order)
    t_proj_host = time.perf_counter() - t0
    proj_diff = float(np.abs(y.cpu().numpy() - y_ref).max() / np.abs(y_ref).max())

    alg = k * (8 * n_plane * n_plane + 16 * res * res)
    moved = alg + k * 32 * n_plane * n_plane
    tile_bytes = TILE * TILE * 4
    print(json.dumps({
        "metric": "ymap_light_cone", "dtype": args.dtype, "planes": k, "delta": [n, n], "n_plane": n_plane,
        "tiles_per_plane": n_tiles, "resolution": res, "batch": args.batch, "order": args.order,
        "projection_host_s": round(t_proj_host, 4), "projection_host_download_s": round(t_down, 4),
        "projection_device_s": {"median": round(t_proj_dev, 6), "min": round(min(times), 6),
                                "max": round(max(times), 6), "reps": args.reps},
        "projection_device_s_per_plane": round(t_proj_dev / k, 6),
        "projection_speedup": round(t_proj_host / t_proj_dev, 1),
        "projection_device_faster_than_host": bool(t_proj_dev < t_proj_host),
        "projection_bytes": alg, "projection_kernel_bytes": moved,
        "projection_hbm_fraction": round(alg / t_proj_dev / HBM_PEAK, 4),
        "projection_kernel_hbm_fraction": round(moved / t_proj_dev / HBM_PEAK, 4),
        "projection_device_vs_host_max_rel_diff": proj_diff,
        "light_cone_host_s": round(t_cone_host, 3), "light_cone_device_s": round(t_cone_dev, 3),
        "light_cone_speedup": round(t_cone_host / t_cone_dev, 2),
        "light_cone_device_vs_host_max_rel_diff": diff,
        "host_link_bytes": {"host": k * n_tiles * 2 * tile_bytes,
                            "device": int(sum(d.nbytes for d in deltas) + res * res * 8)}}), flush=True)
    pt.release_paint_buffers()
    LC.release_projection_buffers()
    if not t_proj_dev < t_proj_host:
        raise SystemExit("the device projection is not faster than the host projection: the kernel is wrong")


if __name__ == "__main__":
    main()
