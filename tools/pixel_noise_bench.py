"""What painting draws from the likelihood costs: a two-head fiducial CVAE (``fiducial_architecture(predict_var=True)``)
on 512^2 tiles in batches of 64, synthetic weights and statistics, all in one process.  One JSON line per measurement:

  paint_stream_noise   raw host tiles in, physical host tiles out with ``pixel_noise=True``: the captured pipeline with
                       bp_likelihood_draw between the generator and the store
  paint_stream_mean    the same painter and tiles without it, in the same run; the two are timed alternately,
                       ``--repeats`` times each, and every repeat is reported
  likelihood_draw      bp_likelihood_draw alone on one batch's heads (three floats moved per element), beside
                       bp_paint_store on the same head: the two alternate for ``--rounds`` rounds of ``--launches``
                       launches between two device events; every round, the medians and the draw's bytes and GB/s

No figure is fixed in advance.  Usage: python tools/pixel_noise_bench.py [--tiles 256] [--batch 64] [--tile 512]
[--repeats 3] [--launches 200] [--rounds 5]"""
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


def make_painter(dev, tile):
    from baryon_painter_amd.models import arch as A
    from baryon_painter_amd.models.cvae import CVAE
    from baryon_painter_amd.painter import CVAEPainter
    from baryon_painter_amd.utils import data_transforms as T
    from baryon_painter_amd.utils.datasets import SyntheticTileDataset, compile_transform
    ds = SyntheticTileDataset(n_sample=8, tile_size=tile, seed=3)
    torch.manual_seed(1234)
    with contextlib.redirect_stdout(sys.stderr):
        model = CVAE(A.fiducial_architecture(tile, predict_var=True), dev)
    model.train(False)
    pt = CVAEPainter.__new__(CVAEPainter)
    pt.model, pt.compute_device, pt.sync, pt.dtype = model, dev, None, "f32"
    pt.input_field, pt.label_fields = ds.input_field, ["pressure"]
    fwd, inv = T.create_range_compress_transforms({"dm": 4.0, "pressure": 4.0}, {"dm": "shift-log", "pressure": "shift-log"})
    pt.transform = compile_transform(T.chain_transformations([fwd, T.atleast_3d, T.as_float32]), ds.stats)
    pt.inverse_transform = compile_transform(T.chain_transformations([T.squeeze, inv]), ds.stats)
    return pt, ds


def tiles_of(ds, n):
    raw = np.stack([ds.raw_fields(i)[0] for i in range(8)])
    zs = np.array([ds.raw_fields(i)[2] for i in range(8)])
    reps = (n + 7) // 8
    return np.tile(raw, (reps, 1, 1))[:n], np.tile(zs, reps)[:n]


def stream_time(pt, tin, zs, batch, tout, noise):
    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pt.paint_stream(tin, zs, batch_size=batch, out=tout, seed=5, pixel_noise=noise)
        torch.cuda.synchronize()
        return time.perf_counter() - t0


def kernel_times(n, tile, launches, rounds):
    """(ms per bp_likelihood_draw launch, ms per bp_paint_store launch) on (n, tile, tile, 1) heads: one figure per
    round, each the mean over ``launches`` launches between two events."""
    from baryon_painter_amd import _lib as L
    lib = L.load()
    mu = torch.randn((n, tile, tile, 1), device="cuda")
    lv = torch.randn((n, tile, tile, 1), device="cuda") - 4.0
    out = torch.empty((n, tile, tile, 1), device="cuda")
    dst = torch.empty((n, 1, tile, tile), device="cuda")
    views = [L.View(t.data_ptr(), n, tile, tile, 1, 1, 0) for t in (mu, lv, out)]
    seed = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
    ids = torch.arange(n, dtype=torch.int64, device="cuda")
    org = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    k_sigma = torch.tensor([[4.0, 1.0]] * n, dtype=torch.float64, device="cuda")
    sm = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def draw():
        L.check(lib.bp_likelihood_draw(C.byref(views[0]), 1, C.byref(views[1]), L.ptr(seed), L.ptr(ids), L.ptr(org),
                                       C.byref(views[2]), sm), "draw")

    def store():
        L.check(lib.bp_paint_store(C.byref(views[2]), None, 0, L.ptr(k_sigma), L.ptr(dst), sm), "store")
    times = {draw: [], store: []}
    for fn in (draw, store):                                     # first launches
        for _ in range(5):
            fn()
    for _ in range(rounds):                                      # the two alternate: clocks and neighbours drift
        for fn in (draw, store):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[fn].append(a.elapsed_time(b) / launches)
    assert torch.isfinite(out).all() and float((out - torch.nn.functional.softplus(mu)).std()) > 0.05
    return times[draw], times[store]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pixel_noise_bench.py measures on a GPU: none found")
    common = {"tile": args.tile, "batch": args.batch}
    pt, ds = make_painter("cuda:0", args.tile)
    assert pt.can_paint_stream()
    raw, zs = tiles_of(ds, args.tiles)
    tin = torch.from_numpy(raw).pin_memory()
    tout = torch.empty(raw.shape, dtype=torch.float32).pin_memory()
    warm = 2 * args.batch
    for noise in (True, False):                                  # capture, page-lock, first launches
        stream_time(pt, tin[:warm], zs[:warm], args.batch, tout[:warm], noise)
    for r in range(args.repeats):
        for name, noise in (("paint_stream_noise", True), ("paint_stream_mean", False)):
            dt = stream_time(pt, tin, zs, args.batch, tout, noise)
            print(json.dumps({"measurement": name, "repeat": r, "tiles": len(raw), "tiles_per_s": round(len(raw) / dt, 1),
                              "ms_per_batch": round(dt / (len(raw) / args.batch) * 1e3, 2), **common}), flush=True)
    pt.release_paint_buffers()
    del pt, tin, tout
    torch.cuda.empty_cache()
    ms_draw, ms_store = kernel_times(args.batch, args.tile, args.launches, args.rounds)
    nbytes = 3 * 4 * args.batch * args.tile * args.tile
    med = float(np.median(ms_draw))
    print(json.dumps({"measurement": "likelihood_draw", "launches_per_round": args.launches,
                      "ms_likelihood_draw": [round(v, 4) for v in ms_draw],
                      "ms_paint_store": [round(v, 4) for v in ms_store],
                      "median_ms": [round(med, 4), round(float(np.median(ms_store)), 4)],
                      "draw_bytes": nbytes, "draw_GB_per_s": round(nbytes / (med * 1e-3) / 1e9, 1), **common}))


if __name__ == "__main__":
    main()
