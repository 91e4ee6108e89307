"""What an ensemble costs: a two-head fiducial CVAE (``fiducial_architecture(predict_var=True)``) on 512^2 tiles in
batches of 64 generator samples, synthetic weights and statistics, all in one process.  One JSON line per measurement:

  store_moments        bp_paint_store_moments alone on the head of one batch (K draws of 64 / K tiles, one channel)
                       beside bp_paint_store_fields on the same head: the moments kernel reads the same bytes and
                       writes 2 / K of them.  The two alternate for ``--rounds`` rounds of ``--launches`` launches
                       between two device events; every round, the medians, and the bytes and GB/s of both
  paint_ensemble       raw host tiles in, mean and variance out: ``paint_ensemble(draws=K)``
  paint_stream_k_seeds the same tiles through ``paint_stream`` under K seeds, then NumPy's float64 mean and variance
                       over the K results on the host -- what a user did before.  The two are timed alternately,
                       ``--repeats`` times each, for every K of ``--draws``; every repeat is reported

No figure is fixed in advance.  Usage: python tools/ensemble_bench.py [--tiles 32] [--batch 64] [--tile 512]
[--draws 4,16] [--repeats 3] [--launches 100] [--rounds 5]"""
import argparse
import copy
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pixel_noise_bench import make_painter, tiles_of  # noqa: E402


def kernel_times(K, batch, tile, launches, rounds):
    """(ms per bp_paint_store_moments launch, ms per bp_paint_store_fields launch) on one (batch, tile, tile, 1) head of
    K draws of batch / K tiles: one figure per round, each the mean over ``launches`` launches between two events."""
    from baryon_painter_amd import _lib as L
    lib = L.load()
    n = batch // K
    head = torch.rand((batch, tile, tile, 1), device="cuda") * 1.4 + 0.1
    view = L.View(head.data_ptr(), batch, tile, tile, 1, 1, 0)
    rec = torch.tensor([[[0.3, 4.0, 0.0, 0.0]]] * n, dtype=torch.float64, device="cuda")
    rec_k = rec.repeat(K, 1, 1)
    mean, var = torch.empty((n, 1, tile, tile), device="cuda"), torch.empty((n, 1, tile, tile), device="cuda")
    dst = torch.empty((batch, 1, tile, tile), device="cuda")
    modes = (C.c_int32 * 1)(L.RC_SHIFT_LOG)
    sm = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def moments():
        L.check(lib.bp_paint_store_moments(modes, 1, 1, 0, C.byref(view), None, 0, L.ptr(rec), K, L.ptr(mean), L.ptr(var),
                                           None, sm), "moments")

    def fields():
        L.check(lib.bp_paint_store_fields(modes, 1, 1, 0, C.byref(view), None, 0, L.ptr(rec_k), L.ptr(dst), sm), "fields")
    times = {moments: [], fields: []}
    for fn in (moments, fields):                                 # first launches
        for _ in range(5):
            fn()
    for _ in range(rounds):                                      # the two alternate: clocks and neighbours drift
        for fn in (moments, fields):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[fn].append(a.elapsed_time(b) / launches)
    # the moments are those of the stored draws (float64 on the device; the kernel's own order is pinned by the tests)
    d = dst.view(K, n, tile, tile).double()
    assert torch.allclose(mean[:, 0].double(), d.mean(0), rtol=1e-6) and \
        torch.allclose(var[:, 0].double(), d.var(0, unbiased=False), rtol=1e-5, atol=1e-12)
    return times[moments], times[fields]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=32)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--draws", default="4,16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench.py measures on a GPU: none found")
    draws = [int(k) for k in args.draws.split(",")]
    common = {"tile": args.tile, "batch": args.batch}
    for K in draws:
        ms_m, ms_f = kernel_times(K, args.batch, args.tile, args.launches, args.rounds)
        px = args.batch * args.tile * args.tile
        b_m, b_f = 4 * px + 8 * px // K, 8 * px
        med_m, med_f = float(np.median(ms_m)), float(np.median(ms_f))
        print(json.dumps({"measurement": "store_moments", "draws": K, "launches_per_round": args.launches,
                          "ms_store_moments": [round(v, 4) for v in ms_m], "ms_store_fields": [round(v, 4) for v in ms_f],
                          "median_ms": [round(med_m, 4), round(med_f, 4)], "bytes": [b_m, b_f],
                          "GB_per_s": [round(b_m / (med_m * 1e-3) / 1e9, 1), round(b_f / (med_f * 1e-3) / 1e9, 1)],
                          **common}), flush=True)
    torch.cuda.empty_cache()
    pt, ds = make_painter("cuda:0", args.tile)
    # (a painter keeps the page-locked staging buffers of ONE pipeline shape: the two legs get a painter each over the one
    #  model, so that neither pays for page-locking again every time the other has run)
    pe = copy.copy(pt)
    raw, zs = tiles_of(ds, args.tiles)

    def ensemble(K, n=len(raw)):
        return pe.paint_ensemble(raw[:n], zs[:n], draws=K, batch_size=args.batch, seed=5)

    def k_seeds(K, n=len(raw)):
        runs = np.stack([pt.paint_stream(raw[:n], zs[:n], batch_size=args.batch, seed=5 + k) for k in range(K)])
        return runs.mean(axis=0, dtype=np.float64), runs.var(axis=0, dtype=np.float64)
    with torch.no_grad():
        for K in draws:                                          # capture, page-lock, first launches
            ensemble(K, min(len(raw), 2 * args.batch // K))
        k_seeds(1, min(len(raw), 2 * args.batch))
        for K in draws:
            for r in range(args.repeats):
                for name, fn in (("paint_ensemble", ensemble), ("paint_stream_k_seeds", k_seeds)):
                    dt, (mean, var) = timed(lambda: fn(K))
                    assert np.isfinite(mean).all() and (var >= 0).all()
                    print(json.dumps({"measurement": name, "draws": K, "repeat": r, "tiles": len(raw),
                                      "seconds": round(dt, 4), "tiles_per_s": round(len(raw) / dt, 2),
                                      "draws_per_s": round(len(raw) * K / dt, 1), **common}), flush=True)


if __name__ == "__main__":
    main()
