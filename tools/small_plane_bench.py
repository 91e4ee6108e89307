"""The low-redshift planes of a light cone: lightcone.paint_small_plane on the host path (wrapped gather, SciPy's mirror
zoom on one core, one tile through paint_stream, host crop) against the device path (on_device=True: csrc/window.hip
around the captured paint graph, one stream), and a light cone with and without ``small_planes_on_device``.

Geometry of the reference's driver: a ``--mass``^2 (12288) float32 mass plane of size 505, tiles of size 100 and 512
pixels, and the two planes of a 10 degree field that are smaller than a tile, ``delta_size`` 22 and 66: each a 2433^2
window resampled to 512^2.  The plane is synthetic, smooth and positive (a sum of plane waves, exponentiated); the
painter is the fiducial 512^2 architecture with synthetic weights (as tools/plane_bench.py builds it).  One JSON line:

  small_plane_host_s           paint_small_plane on the host path, per plane, host clock (the call ends synchronised);
                               ``host_gather_s`` / ``host_zoom_s``: get_tile and scipy.ndimage.zoom alone on the same window
  small_plane_device_s         on_device=True from the host plane (the window is gathered on the host and uploaded, the
                               plane downloaded), host clock around ``--reps`` calls that end in a synchronise
  small_plane_resident_s       on_device=True from a resident CUDA plane into ``out=``: nothing crosses the host link
  window_zoom_s                bp_window_zoom alone on the resident plane, HIP events, median / min / max over ``--reps``
                               after a warm-up
  light_cone_s                 paint_light_cone(on_device=True) of the two small planes and one tiled ``--delta``^2 (4096)
                               plane into a ``--res``^2 (4096) map, with and without small_planes_on_device (one run each
                               after a warm-up of both)
  *_max_rel_diff               device against host, of the plane's (map's) maximum

Exits non-zero if the device small plane is not faster than the host one in the same run.

Usage: python tools/small_plane_bench.py [--dtype f32] [--mass 12288] [--delta 4096] [--res 4096] [--reps 5] [--batch 64]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from baryon_painter_amd import _lib as L  # noqa: E402
from baryon_painter_amd import lightcone as LC  # noqa: E402
from plane_bench import TILE, make_painter, timed  # noqa: E402

MASS_SIZE, TILE_SIZE, SMALL = 505.0, 100.0, (22.0, 66.0)


def smooth_plane(n, seed, dev):
    """A smooth positive periodic (n, n) float32 plane on ``dev``: 0.05 exp(f / 2 std f), f a sum of 12 plane waves
    of up to 40 periods across the plane (cos(a + b) as two outer products: one matrix product)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    k = rng.integers(-40, 41, size=(12, 2))
    amp, phase = rng.standard_normal(12), rng.uniform(0, 2 * np.pi, 12)
    x = torch.arange(n, dtype=torch.float64, device=dev) * (2 * np.pi / n)
    a = torch.from_numpy(k[:, 0].astype(np.float64)).to(dev)[:, None] * x[None, :] + torch.from_numpy(phase).to(dev)[:, None]
    b = torch.from_numpy(k[:, 1].astype(np.float64)).to(dev)[:, None] * x[None, :]
    w = torch.from_numpy(amp).to(dev)[:, None]
    u = torch.cat([w * torch.cos(a), -w * torch.sin(a)]).float()                 # (24, n)
    v = torch.cat([torch.cos(b), torch.sin(b)]).float()
    f = u.t() @ v
    return (torch.exp(f * (0.5 / f.std())) * 0.05).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--mass", type=int, default=12288)
    ap.add_argument("--delta", type=int, default=4096)
    ap.add_argument("--res", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("small_plane_bench needs a GPU")
    dev = torch.device("cuda:0")
    pt = make_painter(args.dtype, dev)
    n, reps = args.mass, args.reps
    mass_d = smooth_plane(n, 7, dev)
    mass_h = mass_d.cpu().numpy()
    shift, z_small, seed = (0.93, 0.41), (0.03, 0.09), 11
    geos = [LC.small_plane_geometry(n, shift, d, TILE_SIZE, MASS_SIZE, TILE) for d in SMALL]
    lib = L.load()

    per_plane = []
    for i, (d, geo) in enumerate(zip(SMALL, geos)):
        a = (shift, d, TILE_SIZE, MASS_SIZE, TILE, z_small[i])
        kw = dict(seed=seed, tile_id=i)
        out = torch.empty((geo["crop"], geo["crop"]), dtype=torch.float64, device=dev)
        dev_fn = lambda: LC.paint_small_plane(pt, mass_h, *a, on_device=True, **kw)          # noqa: E731
        res_fn = lambda: LC.paint_small_plane(pt, mass_d, *a, on_device=True, out=out, **kw)  # noqa: E731
        host_fn = lambda: LC.paint_small_plane(pt, mass_h, *a, **kw)                        # noqa: E731
        dev_fn()                                                  # capture + warm-up (the host path replays the same graph)
        host_fn()
        t_dev, plane_dev = timed(dev_fn, reps)
        t_res, _ = timed(res_fn, reps)
        t_host, plane_host = timed(host_fn, 1)
        assert np.array_equal(out.cpu().numpy(), plane_dev)       # both routes: the same bits
        # the host stages alone
        import scipy.ndimage
        t0 = time.perf_counter()
        window = LC.get_tile(mass_h, shift, tile_relative_size=d / MASS_SIZE, expansion_factor=TILE_SIZE / d)
        t_gather = time.perf_counter() - t0
        t0 = time.perf_counter()
        tile_host = scipy.ndimage.zoom(window, zoom=TILE / window.shape[0], mode="mirror")
        t_zoom = time.perf_counter() - t0
        # bp_window_zoom alone, on the resident plane
        cut = geo["cut"]
        ws = int(lib.bp_window_zoom_workspace(cut, TILE))
        scratch = torch.empty(ws // 8, dtype=torch.float64, device=dev)
        tile_d = torch.empty((TILE, TILE), dtype=torch.float32, device=dev)

        def zoom():
            sm = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            L.check(lib.bp_window_zoom(L.ptr(mass_d), L.F32, n, n, geo["x0"], geo["y0"], cut, None, TILE, L.ptr(scratch),
                                       ws, L.ptr(tile_d), sm), "window zoom")
        zoom()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            zoom()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        tile_dev = tile_d.cpu().numpy()
        per_plane.append({
            "delta_size": d, "window": cut, "crop": geo["crop"],
            "small_plane_host_s": round(t_host, 4), "host_gather_s": round(t_gather, 4), "host_zoom_s": round(t_zoom, 4),
            "small_plane_device_s": round(t_dev, 5), "small_plane_resident_s": round(t_res, 5),
            "window_zoom_s": {"median": round(float(np.median(times)), 6), "min": round(min(times), 6),
                              "max": round(max(times), 6), "reps": reps},
            "speedup_from_host_plane": round(t_host / t_dev, 1), "speedup_resident": round(t_host / t_res, 1),
            "tile_bit_equal_share": float((tile_dev == tile_host).mean()),
            "tile_max_ulp32_diff": float(np.abs(tile_dev.view(np.int32).astype(np.int64)
                                                - tile_host.view(np.int32).astype(np.int64)).max()),
            "plane_max_rel_diff": float(np.abs(plane_dev - plane_host).max() / np.abs(plane_host).max()),
            "host_link_bytes": {"host": int(2 * TILE * TILE * 4), "device_from_host_plane": int(window.nbytes
                                                                                               + 8 * geo["crop"] ** 2),
                                "resident": 0}})

    # ---- a light cone: the two small planes and one tiled plane
    nd_ = args.delta
    rng = np.random.Generator(np.random.PCG64(100))
    delta = (np.exp(rng.standard_normal((nd_, nd_), dtype=np.float32) * 0.5) * 0.05).astype(np.float32)
    delta_size = list(SMALL) + [TILE_SIZE * nd_ / TILE]            # tile_relative_size = 512 / delta: no resampling
    z = list(z_small) + [0.5]
    n_plane = LC.plane_geometry(nd_, TILE_SIZE / delta_size[2], TILE)["n_plane"]
    scales = LC.y_map_scales([g["crop"] for g in geos] + [n_plane], args.res, 10.0, np.array([80.0, 250.0, 1300.0]),
                             lambda c: 1 / (1 + c / 3300.0), 0.69)
    kw = dict(tile_size=TILE_SIZE, n_pixel_tile=TILE, resolution=args.res, scales=scales, batch_size=args.batch,
              seed=seed, on_device=True)
    for name, m in (("host_planes", mass_h), ("resident_planes", mass_d)):
        planes = [(m, shift, MASS_SIZE), (m, shift, MASS_SIZE), delta]
        if name == "host_planes":
            LC.paint_light_cone(pt, planes, z, delta_size, **kw)                            # warm-up of both
            LC.paint_light_cone(pt, planes, z, delta_size, small_planes_on_device=True, **kw)
            t_off, y_off = timed(lambda: LC.paint_light_cone(pt, planes, z, delta_size, **kw), 1)
        t_on, y_on = timed(lambda: LC.paint_light_cone(pt, planes, z, delta_size, small_planes_on_device=True, **kw), 1)
        if name == "host_planes":
            cone = {"small_planes_on_host_s": round(t_off, 3), "small_planes_on_device_s": round(t_on, 3)}
            cone["map_max_rel_diff"] = float(np.abs(y_on - y_off).max() / np.abs(y_off).max())
        else:
            cone["small_planes_on_device_resident_s"] = round(t_on, 3)
    cone.update(planes=["small 22", "small 66", f"tiled {nd_}^2"], resolution=args.res, batch=args.batch)

    faster = all(p["small_plane_device_s"] < p["small_plane_host_s"] for p in per_plane)
    print(json.dumps({"metric": "small_plane", "dtype": args.dtype, "mass_plane": [n, n], "tile": TILE,
                      "planes": per_plane, "light_cone_s": cone, "device_faster_than_host": bool(faster)}), flush=True)
    pt.release_paint_buffers()
    LC.release_projection_buffers()
    if not faster:
        raise SystemExit("the device small plane is not faster than the host small plane")


if __name__ == "__main__":
    main()
