"""Light-cone plane throughput: lightcone.paint_plane on the host path (get_tile / scipy zoom / NumPy blend around
paint_stream) against the device path (on_device=True: csrc/plane.hip cut, zoom and blend around the same captured
graph), with paint_stream alone on the same number of tiles for reference.  Fiducial 512^2 architecture with synthetic
weights (as bench.py builds it), fp32 and bf16.  One JSON line per (dtype, case):

  nozoom  4096^2 plane of 512^2 tiles at 0.5 overlap (225 tiles), delta 4096^2 float32: cuts are 512 pixels wide
  zoom    the same tiling of a 5000^2 float32 delta: 625-pixel cuts resampled to 512

``host_link_bytes_per_tile``: bytes that cross the host link per painted tile, from the sizes (host path: the float32
tile up and the float32 painted tile down; device path: the delta up once and the float64 plane down once, over the
tile count).  ``device_resident_tiles_per_s``: the device path with delta already on the GPU and ``out=`` a device
tensor (nothing crosses the link).

Usage: python tools/plane_bench.py [--dtypes f32,bf16] [--cases nozoom,zoom] [--reps 3] [--batch 64]"""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from baryon_painter_amd import lightcone as LC  # noqa: E402

TILE, N_PLANE = 512, 4096
CASES = {"nozoom": 4096, "zoom": 5000}


def make_painter(dtype, dev):
    from baryon_painter_amd.models import arch as A
    from baryon_painter_amd.models.cvae import CVAE
    from baryon_painter_amd.painter import CVAEPainter
    from baryon_painter_amd.utils.datasets import SyntheticTileDataset
    arch = A.fiducial_architecture(TILE)
    torch.manual_seed(1234)
    with contextlib.redirect_stdout(sys.stderr):
        model = CVAE(arch, dev, dtype=dtype)
    model.train(False)
    ds = SyntheticTileDataset(n_sample=8, tile_size=TILE, seed=3)
    pt = CVAEPainter.__new__(CVAEPainter)
    pt.model, pt.compute_device, pt.sync, pt.dtype = model, dev, None, dtype
    pt.input_field, pt.label_fields = ds.input_field, ds.label_fields
    pt.transform, pt.inverse_transform = ds.transform, ds.inverse_transform
    return pt


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, r


def run_case(pt, dtype, case, n_delta, reps, batch, z=0.5, seed=11):
    rel = TILE / N_PLANE
    rng = np.random.Generator(np.random.PCG64(n_delta))
    delta = (np.exp(rng.standard_normal((n_delta, n_delta), dtype=np.float32) * 0.5) * 0.05).astype(np.float32)
    geo = LC.plane_geometry(n_delta, rel, TILE)
    n_tiles = len(geo["origins"])
    kw = dict(seed=seed, batch_size=batch)
    dev_fn = lambda: LC.paint_plane(pt, delta, rel, TILE, z, on_device=True, **kw)          # noqa: E731
    dev_fn()                                                                                # capture + warm-up
    t_dev, plane_dev = timed(dev_fn, reps)
    d_res = torch.from_numpy(delta).cuda()
    out = torch.empty((N_PLANE, N_PLANE), dtype=torch.float64, device="cuda")
    t_res, _ = timed(lambda: LC.paint_plane(pt, d_res, rel, TILE, z, on_device=True, out=out, **kw), reps)
    host_fn = lambda: LC.paint_plane(pt, delta, rel, TILE, z, **kw)                       # noqa: E731
    t_host, plane_host = timed(host_fn, 1)                                                  # (seconds per call)
    tiles = np.stack([np.asarray(LC.get_tile(delta, (0.0, 0.0), rel), np.float32)] * 1)
    if tiles.shape[-1] != TILE:
        import scipy.ndimage as nd
        tiles = nd.zoom(tiles[0], TILE / tiles.shape[-1], mode="reflect")[None].astype(np.float32)
    tiles = np.ascontiguousarray(np.broadcast_to(tiles, (n_tiles, TILE, TILE)))
    ids = np.arange(n_tiles, dtype=np.int64)
    pt.paint_stream(tiles, z, batch_size=batch, tile_ids=ids, seed=seed)
    t_ps, _ = timed(lambda: pt.paint_stream(tiles, z, batch_size=batch, tile_ids=ids, seed=seed), reps)
    ok = np.isfinite(plane_host)
    assert np.array_equal(np.isfinite(plane_dev), ok)
    rel_err = float(np.abs(plane_dev[ok] - plane_host[ok]).max() / np.abs(plane_host[ok]).max())
    tile_bytes = TILE * TILE * 4
    return {"metric": "paint_plane_tiles_per_s", "dtype": dtype, "case": case, "delta": [n_delta, n_delta],
            "cut": geo["cut"], "tile": TILE, "n_plane": N_PLANE, "tiles": n_tiles, "batch": batch,
            "host_tiles_per_s": round(n_tiles / t_host, 1), "device_tiles_per_s": round(n_tiles / t_dev, 1),
            "device_resident_tiles_per_s": round(n_tiles / t_res, 1),
            "paint_stream_tiles_per_s": round(n_tiles / t_ps, 1),
            "speedup_device_over_host": round(t_host / t_dev, 2),
            "host_link_bytes_per_tile": {"host": 2 * tile_bytes,
                                         "device": round((delta.nbytes + N_PLANE * N_PLANE * 8) / n_tiles)},
            "device_vs_host_max_rel_diff": rel_err, "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--cases", default="nozoom,zoom")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plane_bench needs a GPU")
    for dtype in args.dtypes.split(","):
        pt = make_painter(dtype, torch.device("cuda:0"))
        for case in args.cases.split(","):
            print(json.dumps(run_case(pt, dtype, case, CASES[case], args.reps, args.batch)), flush=True)
        pt.release_paint_buffers()
        del pt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
