"""Multi-scale painter throughput: a CVAE whose transform chains hold the split-scale (Gaussian pyramid) transform
(n_scale=3, step_size=4, original kept: 4 channels) on 512^2 tiles in batches of 64, fiducial architecture widened by
``fiducial_architecture(n_scale=4)``, synthetic weights and statistics.  One JSON line per measurement:

  paint_stream       raw host tiles in, physical host tiles out through the device pipeline (bp_paint_load_scales2 /
                     bp_paint_store_scales around the captured graph)
  paint_batch        the same tiles through paint_batch: host transforms (SciPy's gaussian_filter per tile) around the
                     captured forward
  single_scale       paint_stream of the single-scale fiducial painter on the same tiles, for scale
  split_scale        bp_split_scale alone on 64 resident tiles: tiles/s and GB/s of its algorithmic traffic (one
                     float32 read and `levels` float32 writes per pixel)

``--profile``: only a few multi-scale paint_stream batches and nothing else -- the run to put under
``rocprofv3 --kernel-trace --stats`` for the share of the load / pyramid / store kernels in the paint graph.

Usage: python tools/scales_bench.py [--tiles 256] [--batch 64] [--host-tiles 64] [--profile]"""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE, N_SCALE, STEP, INCLUDE_ORIGINAL = 512, 3, 4, True
LEVELS = N_SCALE + int(INCLUDE_ORIGINAL)


def make_painter(dev, multi):
    from baryon_painter_amd.models import arch as A
    from baryon_painter_amd.models.cvae import CVAE
    from baryon_painter_amd.painter import CVAEPainter
    from baryon_painter_amd.utils import data_transforms as T
    from baryon_painter_amd.utils.datasets import SyntheticTileDataset, compile_transform
    ds = SyntheticTileDataset(n_sample=8, tile_size=TILE, seed=3)
    arch = A.fiducial_architecture(TILE, n_scale=LEVELS if multi else 1)
    torch.manual_seed(1234)
    with contextlib.redirect_stdout(sys.stderr):
        model = CVAE(arch, dev)
    model.train(False)
    pt = CVAEPainter.__new__(CVAEPainter)
    pt.model, pt.compute_device, pt.sync, pt.dtype = model, dev, None, "f32"
    pt.input_field, pt.label_fields = ds.input_field, ds.label_fields
    if multi:
        fwd, inv = T.create_range_compress_transforms({"dm": 4.0, "pressure": 4}, {"dm": "shift-log",
                                                                                  "pressure": "shift-log"})
        split, unsplit = T.create_split_scale_transform(N_SCALE, STEP, INCLUDE_ORIGINAL)
        pt.transform = compile_transform(T.chain_transformations([fwd, T.as_float32, split, T.atleast_3d]), ds.stats)
        pt.inverse_transform = compile_transform(T.chain_transformations([unsplit, inv, T.squeeze]), ds.stats)
    else:
        pt.transform, pt.inverse_transform = ds.transform, ds.inverse_transform
    return pt, ds


def tiles_of(ds, n):
    raw = np.stack([ds.raw_fields(i)[0] for i in range(8)])
    zs = np.array([ds.raw_fields(i)[2] for i in range(8)])
    reps = (n + 7) // 8
    return np.tile(raw, (reps, 1, 1))[:n], np.tile(zs, reps)[:n]


def stream_rate(pt, raw, zs, batch):
    tin = torch.from_numpy(raw).pin_memory()
    tout = torch.empty(raw.shape, dtype=torch.float32).pin_memory()
    with torch.no_grad():
        pt.paint_stream(tin[:2 * batch], zs[:2 * batch], batch_size=batch, out=tout[:2 * batch])      # capture
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pt.paint_stream(tin, zs, batch_size=batch, out=tout)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    assert np.isfinite(tout.numpy()).all()
    return len(raw) / dt, dt


def split_scale_alone(dev, n, reps=20):
    from baryon_painter_amd import _lib as L
    from baryon_painter_amd.utils import data_transforms as T
    lib = L.load()
    x = torch.rand((n, TILE, TILE), device=dev)
    out = torch.empty((n, TILE, TILE, LEVELS), device=dev)
    view = L.view(out, n, TILE, TILE, LEVELS)
    sig = T.split_scale_sigmas(N_SCALE, STEP)
    radii = [0] + [T.gaussian_radius(s) for s in sig[1:]]
    w = torch.from_numpy(np.concatenate([T.gaussian_weights(s) for s in sig[1:]])).to(dev)
    ws = int(lib.bp_split_scale_workspace(n, TILE, TILE))
    scratch = torch.empty(ws // 4, device=dev)
    rad = (C.c_int32 * len(radii))(*radii)
    sm = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        L.check(lib.bp_split_scale(L.ptr(x), n, TILE, TILE, N_SCALE, int(INCLUDE_ORIGINAL), L.ptr(w), rad,
                                   L.ptr(scratch), ws, C.byref(view), sm), "split scale")
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    return n / dt, n * TILE * TILE * 4 * (1 + LEVELS) / dt / 1e9, dt, radii[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--host-tiles", type=int, default=64)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    dev = "cuda:0"
    common = {"tile": TILE, "batch": args.batch, "n_scale": N_SCALE, "step_size": STEP,
              "include_original": INCLUDE_ORIGINAL, "levels": LEVELS}
    pt, ds = make_painter(dev, multi=True)
    assert pt.can_paint_stream()
    if args.profile:
        raw, zs = tiles_of(ds, 3 * args.batch)
        rate, dt = stream_rate(pt, raw, zs, args.batch)
        print(json.dumps({"measurement": "profile", "tiles": len(raw), "tiles_per_s": round(rate, 1), **common}))
        return
    raw, zs = tiles_of(ds, args.tiles)
    rate, dt = stream_rate(pt, raw, zs, args.batch)
    print(json.dumps({"measurement": "paint_stream", "tiles": len(raw), "tiles_per_s": round(rate, 1),
                      "ms_per_batch": round(dt / (len(raw) / args.batch) * 1e3, 2), **common}), flush=True)
    m = min(args.host_tiles, len(raw))
    with torch.no_grad():
        pt.paint_batch(raw[:args.batch], zs[:args.batch], batch_size=args.batch)              # capture
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pt.paint_batch(raw[:m], zs[:m], batch_size=args.batch)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    assert out.shape == (m, TILE, TILE)
    print(json.dumps({"measurement": "paint_batch", "tiles": m, "tiles_per_s": round(m / dt, 1),
                      "ms_per_batch": round(dt / (m / args.batch) * 1e3, 2), "transforms": "host (SciPy)", **common}),
          flush=True)
    pt.release_paint_buffers()
    del pt
    torch.cuda.empty_cache()
    single, ds1 = make_painter(dev, multi=False)
    rate, dt = stream_rate(single, raw, zs, args.batch)
    print(json.dumps({"measurement": "single_scale", "tiles": len(raw), "tiles_per_s": round(rate, 1),
                      "ms_per_batch": round(dt / (len(raw) / args.batch) * 1e3, 2), "tile": TILE, "batch": args.batch}),
          flush=True)
    del single
    torch.cuda.empty_cache()
    tps, gbs, dt, radii = split_scale_alone(dev, args.batch)
    print(json.dumps({"measurement": "split_scale", "tiles": args.batch, "tiles_per_s": round(tps, 1),
                      "algorithmic_GB_per_s": round(gbs, 1), "ms_per_call": round(dt * 1e3, 3), "radii": radii,
                      "launches": 2 * (N_SCALE - 1), **common}))


if __name__ == "__main__":
    main()
