"""CGAN paint throughput: CGANPainter.paint tile by tile, paint_batch and paint_stream on 512^2 tiles (nine residual
blocks, synthetic weights), one 4096^2 light-cone plane on the host path against the device path, and the device
memory of the inference plan against the training plan.  One JSON line per measurement:

  paint_tiles_per_s          paint(tile, z), one call per tile (host transforms, inference plan of one tile)
  paint_training_plan_...    the same call through the training plan (_GanPlan: generator + two discriminator unit sets +
                             gradient buffers), launch for launch what paint() ran before the inference plan existed
  paint_batch_tiles_per_s    paint_batch: host transforms, eager forward of ``--batch`` tiles
  paint_stream_tiles_per_s   paint_stream: device transforms, captured graph, pinned double-buffered copies
  paint_plane_tiles_per_s    lightcone.paint_plane of a 4096^2 plane (225 tiles at 0.5 overlap), host and on_device
  plan_memory                torch.cuda.max_memory_allocated over building a plan for ``--mem-n`` tiles and one eval
                             forward through it, inference plan and training plan

``--paint-dtype bf16``: the same lines for the bf16 inference plan (CGAN(paint_dtype="bf16"): the 128-channel trunk on the
bf16 matrix-core kernels); every line carries the dtype.

Usage: python tools/cgan_paint_bench.py [--batch 64] [--tiles 256] [--reps 3] [--mem-n 6] [--skip plane,memory]
                                        [--paint-dtype fp32|bf16]"""
import argparse
import contextlib
import ctypes as C
import gc
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from baryon_painter_amd import _lib as L  # noqa: E402
from baryon_painter_amd import lightcone as LC  # noqa: E402

TILE, N_RES, N_PLANE = 512, 9, 4096


def make_painter(dev, paint_dtype="fp32"):
    from baryon_painter_amd.painter import CGANPainter
    from baryon_painter_amd.utils.datasets import SyntheticTileDataset
    torch.manual_seed(1234)
    ds = SyntheticTileDataset(n_sample=8, tile_size=TILE, seed=3)
    with contextlib.redirect_stdout(sys.stderr):
        pt = CGANPainter(training_data_set=ds, tile_size=TILE, compute_device=dev, n_res=N_RES, paint_dtype=paint_dtype)
    pt.model.train(False)
    return pt, ds


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, r


def paint_through_training_plan(pt, tile, z):
    """CGANPainter.paint as it ran on the training plan: transform, _GanPlan(1).generate in eval mode, bp_view_to_nchw
    of the fake half's pressure channel, inverse transform."""
    m = pt.model
    y = pt.transform(tile, "dm", z)
    with torch.no_grad():
        yd, zc = m._inputs(torch.from_numpy(y.reshape(1, 1, TILE, TILE)), torch.tensor([z]))
        plan = m._plan(1)
        plan.generate(yd, zc, False)
        out = torch.empty((1, 1, TILE, TILE), device=m.device)
        L.check(m._lib.bp_view_to_nchw(C.byref(plan.v_fake_x), None, 0, L.ptr(out),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), "fake layout")
    return pt.inverse_transform(out.cpu().numpy()[0, 0], "pressure", z)


def plan_memory(pt, n):
    from baryon_painter_amd.models.cgan import _GanPaintPlan, _GanPlan
    m = pt.model
    y = torch.zeros((n, 1, TILE, TILE), device=m.device)
    zc = torch.zeros(n, device=m.device)
    res = {}
    for name, cls in (("inference_plan", _GanPaintPlan), ("training_plan", _GanPlan)):
        gc.collect()                              # (cycles holding device tensors would be freed inside the measurement)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.no_grad():
            plan = cls(m, n, m.paint_dtype) if cls is _GanPaintPlan else cls(m, n)
            if cls is _GanPaintPlan:
                plan.generate(y, zc, torch.empty_like(y))
            else:
                plan.generate(y, zc, False)
        torch.cuda.synchronize()
        res[name + "_MiB"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        del plan
    return {"metric": "plan_memory", "n": n, "tile": TILE, "n_res": N_RES, "paint_dtype": m.paint_dtype, **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--per-tile", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mem-n", type=int, default=6)
    ap.add_argument("--skip", default="")
    ap.add_argument("--paint-dtype", default="fp32", choices=("fp32", "bf16"))
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    if not torch.cuda.is_available():
        raise SystemExit("cgan_paint_bench needs a GPU")
    pt, ds = make_painter("cuda:0", args.paint_dtype)
    B, z = args.batch, 0.5
    base = np.stack([ds.raw_fields(i)[0] for i in range(8)])
    tiles = np.ascontiguousarray(np.resize(base, (args.tiles, TILE, TILE)))
    common = {"tile": TILE, "n_res": N_RES, "paint_dtype": args.paint_dtype}

    few = tiles[:args.per_tile]
    pt.paint(few[0], z=z)
    t, _ = timed(lambda: [pt.paint(x, z=z) for x in few], 1)
    print(json.dumps({"metric": "paint_tiles_per_s", **common, "tiles": len(few),
                      "tiles_per_s": round(len(few) / t, 1)}), flush=True)
    paint_through_training_plan(pt, few[0], z)
    t, _ = timed(lambda: [paint_through_training_plan(pt, x, z) for x in few], 1)
    print(json.dumps({"metric": "paint_training_plan_tiles_per_s", **common, "tiles": len(few),
                      "tiles_per_s": round(len(few) / t, 1)}), flush=True)
    pt.model._plans.clear()

    some = tiles[:2 * B]
    pt.paint_batch(some[:B], z, batch_size=B)
    t, _ = timed(lambda: pt.paint_batch(some, z, batch_size=B), 1)
    print(json.dumps({"metric": "paint_batch_tiles_per_s", **common, "batch": B, "tiles": len(some),
                      "tiles_per_s": round(len(some) / t, 1)}), flush=True)

    pt.paint_stream(tiles[:B], z, batch_size=B)                          # capture + warm-up
    t, out = timed(lambda: pt.paint_stream(tiles, z, batch_size=B), args.reps)
    assert np.isfinite(out).all()
    print(json.dumps({"metric": "paint_stream_tiles_per_s", **common, "batch": B, "tiles": len(tiles),
                      "tiles_per_s": round(len(tiles) / t, 1), "reps": args.reps}), flush=True)

    if "plane" not in skip:
        rel = TILE / N_PLANE
        rng = np.random.Generator(np.random.PCG64(N_PLANE))
        delta = (np.exp(rng.standard_normal((N_PLANE, N_PLANE), dtype=np.float32) * 0.5) * 0.05).astype(np.float32)
        n_tiles = len(LC.plane_geometry(N_PLANE, rel, TILE)["origins"])
        dev_fn = lambda: LC.paint_plane(pt, delta, rel, TILE, z, batch_size=B, on_device=True)          # noqa: E731
        dev_fn()
        t_dev, plane_dev = timed(dev_fn, args.reps)
        t_host, plane_host = timed(lambda: LC.paint_plane(pt, delta, rel, TILE, z, batch_size=B), 1)
        ok = np.isfinite(plane_host)
        assert np.array_equal(np.isfinite(plane_dev), ok)
        print(json.dumps({"metric": "paint_plane_tiles_per_s", **common, "n_plane": N_PLANE, "tiles": n_tiles,
                          "batch": B, "host_tiles_per_s": round(n_tiles / t_host, 1),
                          "device_tiles_per_s": round(n_tiles / t_dev, 1),
                          "speedup_device_over_host": round(t_host / t_dev, 2),
                          "device_vs_host_max_rel_diff":
                              float(np.abs(plane_dev[ok] - plane_host[ok]).max() / np.abs(plane_host[ok]).max())}),
              flush=True)

    if "memory" not in skip:
        pt.release_paint_buffers()
        print(json.dumps(plan_memory(pt, args.mem_n)), flush=True)


if __name__ == "__main__":
    main()
