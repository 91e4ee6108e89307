"""Paint throughput of painters whose fields use a range-compression mode other than "shift-log": single-scale fiducial
CVAE on 512^2 tiles in batches of 64, synthetic weights and statistics, all in one run.  One JSON line per measurement:

  paint_stream       raw host tiles in, physical host tiles out through the device pipeline (bp_paint_load2_mode /
                     bp_paint_store_mode around the captured graph), for a (dm "log", pressure "log-tanh") painter
  shift_log          paint_stream of the shift-log painter on the same tiles (bp_paint_load2 / bp_paint_store)
  paint_batch        the "log" / "log-tanh" painter through paint_batch: NumPy transforms per tile around the captured
                     forward -- what such a painter was left with before its modes had a device form

Usage: python tools/modes_bench.py [--tiles 256] [--batch 64] [--host-tiles 64] [--tile 512]"""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = {"dm": "log", "pressure": "log-tanh"}
K_VALUES = {"dm": 2.0, "pressure": 6.0}


def make_painter(dev, tile, modes, k_values):
    from baryon_painter_amd.models import arch as A
    from baryon_painter_amd.models.cvae import CVAE
    from baryon_painter_amd.painter import CVAEPainter
    from baryon_painter_amd.utils import data_transforms as T
    from baryon_painter_amd.utils.datasets import SyntheticTileDataset, compile_transform
    ds = SyntheticTileDataset(n_sample=8, tile_size=tile, seed=3)
    torch.manual_seed(1234)
    with contextlib.redirect_stdout(sys.stderr):
        model = CVAE(A.fiducial_architecture(tile), dev)
    model.train(False)
    pt = CVAEPainter.__new__(CVAEPainter)
    pt.model, pt.compute_device, pt.sync, pt.dtype = model, dev, None, "f32"
    pt.input_field, pt.label_fields = ds.input_field, ds.label_fields
    fwd, inv = T.create_range_compress_transforms(k_values, modes)
    pt.transform = compile_transform(T.chain_transformations([fwd, T.atleast_3d, T.as_float32]), ds.stats)
    pt.inverse_transform = compile_transform(T.chain_transformations([T.squeeze, inv]), ds.stats)
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
    return len(raw) / dt, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--host-tiles", type=int, default=64)
    ap.add_argument("--tile", type=int, default=512)
    args = ap.parse_args()
    dev = "cuda:0"
    common = {"tile": args.tile, "batch": args.batch}
    pt, ds = make_painter(dev, args.tile, MODES, K_VALUES)
    assert pt.can_paint_stream()
    raw, zs = tiles_of(ds, args.tiles)
    rate, dt = stream_rate(pt, raw, zs, args.batch)
    print(json.dumps({"measurement": "paint_stream", "modes": MODES, "tiles": len(raw), "tiles_per_s": round(rate, 1),
                      "ms_per_batch": round(dt / (len(raw) / args.batch) * 1e3, 2), **common}), flush=True)
    m = min(args.host_tiles, len(raw))
    with torch.no_grad(), np.errstate(all="ignore"):
        pt.paint_batch(raw[:args.batch], zs[:args.batch], batch_size=args.batch)              # capture
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pt.paint_batch(raw[:m], zs[:m], batch_size=args.batch)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    assert out.shape[0] == m
    print(json.dumps({"measurement": "paint_batch", "modes": MODES, "tiles": m, "tiles_per_s": round(m / dt, 1),
                      "ms_per_batch": round(dt / (m / args.batch) * 1e3, 2), "transforms": "host (NumPy)", **common}),
          flush=True)
    pt.release_paint_buffers()
    del pt
    torch.cuda.empty_cache()
    plain = {"dm": "shift-log", "pressure": "shift-log"}
    single, _ = make_painter(dev, args.tile, plain, {"dm": 4.0, "pressure": 4})
    rate, dt = stream_rate(single, raw, zs, args.batch)
    print(json.dumps({"measurement": "shift_log", "modes": plain, "tiles": len(raw), "tiles_per_s": round(rate, 1),
                      "ms_per_batch": round(dt / (len(raw) / args.batch) * 1e3, 2), **common}))


if __name__ == "__main__":
    main()
